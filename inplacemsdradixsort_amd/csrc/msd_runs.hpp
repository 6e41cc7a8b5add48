// msd_runs.hpp -- run-length encode: msd_run_encode.
//
// A run is a maximal stretch of consecutive elements with equal bit patterns; head(i) = (i == 0) || data[i] != data[i-1].
// Three stream-ordered steps, and no workgroup ever waits for another one (stream order is the only barrier between them):
//   1. runs_count_kernel: one workgroup per tile counts the tile's heads, one word per tile.
//   2. runs_scan_pieces_kernel: one workgroup per piece of kRunsScanTile tile counts scans its piece in place (exclusive)
//      and writes the piece's total; runs_scan_top_kernel: ONE workgroup scans the piece totals in place, looping with a
//      carry, and writes the number of runs.  A tile's base is then its own word plus its piece's word.
//   3. runs_write_kernel: reads each tile again, finds the heads again and stores: a head its value and its index at its
//      run number (compacted in the LDS first: coalesced stores), every element its run number (the inverse), directly or
//      through the positions.
//
// Tiles lie on the 16-byte grid of memory: with m = the elements between the last 16-byte boundary and data, element i has
// the VIRTUAL index i + m, tile t holds the virtual indices [t * TILE, (t + 1) * TILE) and every 16 bytes of a tile are
// one aligned load.  The 16 bytes that lie only partly inside [m, m + n) -- the first and the last, at most -- are read
// element by element; index -1 and index n are never read.
//
// Inside a tile wave w owns the virtual indices [w * WAVE, (w + 1) * WAVE), lane l the V elements of the 16 bytes
// k * 64 + l for k = 0 .. kRunsVecs-1.  The element in front of a lane's first one is the last one of the lane below
// (a shuffle); for lane 0 the last one of lane 63 one k earlier (a shuffle), and in front of the wave's first element one
// extra predicated load.  The head flags of a (k, e) are one ballot: the heads in front of an element are popcounts --
// uniform words -- plus the count of the lower lanes' bits.
#pragma once

#include <type_traits>

#include "msd_device.hpp"
#include "msd_keycodec.hpp"

namespace msd {

constexpr int kRunsTh = 256;  // threads of the tile kernels
constexpr int kRunsVecs = 4;  // 16-byte loads in flight per lane: 16 KiB per workgroup
template <typename E> struct RunsCfg {
	static constexpr uint32_t V = Vec16<E>::N;                // elements per 16 bytes
	static constexpr uint32_t WAVE = 64u * kRunsVecs * V;     // elements of one wave
	static constexpr uint32_t TILE = (kRunsTh / 64u) * WAVE;  // elements of one workgroup: 4096 (4-byte), 2048 (8-byte)
};
constexpr int kRunsScanTh = 256, kRunsScanPer = 8;
constexpr uint32_t kRunsScanTile = kRunsScanTh * kRunsScanPer; // tile counts one workgroup of the scan takes at once

template <typename E> __host__ __device__ inline uint32_t runs_misalign(const E *data) { return (uint32_t)(((uintptr_t)data & 15u) / sizeof(E)); }
template <typename E> inline uint64_t runs_tiles(const E *data, uint64_t n) { return (runs_misalign(data) + n + RunsCfg<E>::TILE - 1) / RunsCfg<E>::TILE; }

// ---- the run grid's shared pieces: every tile algorithm on this grid (msd_reduce.hpp, msd_scan.hpp, msd_compact.hpp) and
// every reader of scanned tile counts (msd_setops.hpp, msd_join.hpp) takes them from here

// the first place in its tile of lane `lane` of wave `w` in vector k, and its virtual index in tile `tile`
template <typename E> __device__ __forceinline__ uint32_t runs_place(uint32_t w, uint32_t lane, int k)
{
	return w * RunsCfg<E>::WAVE + (uint32_t)(k * 64 + lane) * RunsCfg<E>::V;
}
template <typename E> __device__ __forceinline__ uint64_t runs_vindex(uint64_t tile, uint32_t w, uint32_t lane, int k)
{
	return tile * RunsCfg<E>::TILE + w * RunsCfg<E>::WAVE + (uint64_t)((k * 64 + lane) * RunsCfg<E>::V);
}

// This lane's elements of tile `tile` from the 16-byte-grid base vbase (the array's pointer minus its misalignment: 16-byte
// aligned, dereferenced inside the virtual indices [lo, hi) only).  x[k][e]: virtual index runs_vindex(k) + e, 0 outside
// [lo, hi).  The 16 bytes that lie inside are one aligned load, the partly covered ones are read element by element.
template <typename E>
__device__ __forceinline__ void runs_load_keys(const E *__restrict__ vbase, uint64_t lo, uint64_t hi, uint64_t tile, uint32_t w, uint32_t lane, E (&x)[kRunsVecs][RunsCfg<E>::V])
{
	constexpr uint32_t V = RunsCfg<E>::V;
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint64_t v0 = runs_vindex<E>(tile, w, lane, k);
		if (v0 >= lo && v0 + V <= hi) {
			vec16_unpack<E>(*reinterpret_cast<const u32x4 *>(vbase + v0), x[k]);
		} else {
#pragma unroll
			for (uint32_t e = 0; e < V; ++e) x[k][e] = (v0 + e >= lo && v0 + e < hi) ? vbase[v0 + e] : (E)0;
		}
	}
}

// What the ballots of a tile's flags (heads, kept elements: one per (k, e)) say about ranks.  before_k[k]: the flags of the
// wave in front of vector k (uniform); wpre: those of the lower waves; total: the tile's.
struct RunsRank {
	uint32_t before_k[kRunsVecs], wpre, total;
};
// The workgroup's half of it: r.wpre and r.total from c, the wave's flags.  (Every thread of the workgroup calls it: one
// barrier.  wsum: kRunsTh / 64 words of LDS.)
__device__ __forceinline__ void runs_rank_waves(RunsRank &r, uint32_t c, uint32_t w, uint32_t lane, uint32_t *wsum)
{
	if (lane == 0) wsum[w] = c;
	__syncthreads();
	r.wpre = 0;
#pragma unroll
	for (uint32_t ww = 0; ww < kRunsTh / 64 - 1; ++ww)
		if (ww < w) r.wpre += wsum[ww];
	r.total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// All of it.  (reduce_tile_kernel counts before_k inside its own loop over the ballots and calls runs_rank_waves.)
template <uint32_t V> __device__ __forceinline__ RunsRank runs_rank(const uint64_t (&bb)[kRunsVecs][V], uint32_t w, uint32_t lane, uint32_t *wsum)
{
	RunsRank r;
	uint32_t c = 0;
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		r.before_k[k] = c;
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) c += (uint32_t)__popcll(bb[k][e]);
	}
	runs_rank_waves(r, c, w, lane, wsum);
	return r;
}

// step 1 of every algorithm that counts per tile: the tile's flags, one word per tile
template <uint32_t V> __device__ __forceinline__ void runs_store_count(const uint64_t (&bb)[kRunsVecs][V], uint64_t *__restrict__ tile_counts)
{
	__shared__ uint32_t wsum[kRunsTh / 64];
	const RunsRank r = runs_rank<V>(bb, threadIdx.x >> 6, threadIdx.x & 63u, wsum);
	if (threadIdx.x == 0) tile_counts[blockIdx.x] = (uint64_t)r.total;
}

// where tile t's output begins: its scanned count plus its piece's
__device__ __forceinline__ uint64_t tile_out_base(const uint64_t *__restrict__ tile_base, const uint64_t *__restrict__ piece_base, uint64_t t)
{
	return tile_base[t] + piece_base[t / kRunsScanTile];
}

// The values of this lane's elements of tile `tile` as accumulators of the policy P (msd_reduce.hpp), once, directly or
// (POS) through the positions: what lies outside the array counts as the identity.  A policy whose conv looks at no value
// says so by specialising ReadsValue, and no value is loaded for it.
template <typename P> struct ReadsValue : std::true_type {};
template <typename E, typename P, bool POS>
__device__ __forceinline__ void runs_load_values(uint64_t n, uint32_t m, uint64_t tile, const typename P::V *__restrict__ vals,
	const uint64_t *__restrict__ positions, KeyCodec<typename P::R::O> cd, typename P::R::A (&a)[kRunsVecs][RunsCfg<E>::V])
{
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6; // (worked out here again: handing them in costs the scan kernels registers)
	const uint64_t lo = m, hi = (uint64_t)m + n;
	const typename P::R::A ident = P::R::id(cd);
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint64_t v0 = runs_vindex<E>(tile, w, lane, k);
#pragma unroll
		for (uint32_t e = 0; e < RunsCfg<E>::V; ++e) {
			const uint64_t v = v0 + e;
			a[k][e] = ident;
			if (v >= lo && v < hi) {
				const uint64_t i = v - lo;
				if constexpr (ReadsValue<P>::value)
					a[k][e] = P::conv(vals[POS ? positions[i] : i], cd);
				else
					a[k][e] = P::conv(typename P::V(), cd);
			}
		}
	}
}

// This lane's elements of tile `tile` (runs_load_keys) and the ballots of their head flags
template <typename E>
__device__ __forceinline__ void runs_load_heads(const E *__restrict__ data, uint64_t n, uint32_t m, uint64_t tile, E (&x)[kRunsVecs][RunsCfg<E>::V],
	uint64_t (&hb)[kRunsVecs][RunsCfg<E>::V])
{
	typedef RunsCfg<E> C;
	constexpr uint32_t V = C::V;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint64_t lo = m, hi = m + n;                     // the array in virtual indices
	const uint64_t wv0 = tile * C::TILE + w * C::WAVE;     // the wave's first virtual index
	const E *const vbase = data - m;                       // (16-byte aligned; dereferenced inside [lo, hi) only)
	E before = 0;
	if (lane == 0 && wv0 > lo && wv0 <= hi) before = vbase[wv0 - 1];
	runs_load_keys<E>(vbase, lo, hi, tile, w, lane, x);
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint64_t v0 = runs_vindex<E>(tile, w, lane, k);
		E prev = __shfl_up(x[k][V - 1], 1);
		const E edge = k == 0 ? before : __shfl(x[k == 0 ? 0 : k - 1][V - 1], 63);
		if (lane == 0) prev = edge;
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			const uint64_t v = v0 + e;
			const bool head = v >= lo && v < hi && (v == lo || x[k][e] != (e ? x[k][e - 1] : prev));
			hb[k][e] = __ballot(head);
		}
	}
}

// ---- step 1
template <typename E> __global__ __launch_bounds__(kRunsTh) void runs_count_kernel(const E *__restrict__ data, uint64_t n, uint64_t *__restrict__ tile_counts)
{
	typedef RunsCfg<E> C;
	E x[kRunsVecs][C::V];
	uint64_t hb[kRunsVecs][C::V];
	runs_load_heads<E>(data, n, runs_misalign(data), blockIdx.x, x, hb);
	runs_store_count<C::V>(hb, tile_counts);
}

// ---- step 2
// Exclusive scan of the `count` <= kRunsScanTile words load(0 .. count - 1), on top of `carry`, to w; returns their sum.
// (Every thread of the workgroup calls it: barriers.  tmp: 4 words of LDS.)
template <typename L> __device__ __forceinline__ uint64_t runs_scan_piece(uint64_t *__restrict__ w, uint32_t count, uint64_t carry, uint64_t *tmp, L &&load)
{
	uint64_t v[kRunsScanPer], sum = 0;
#pragma unroll
	for (int j = 0; j < kRunsScanPer; ++j) {
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		v[j] = idx < count ? load(idx) : 0;
		sum += v[j];
	}
	uint64_t total;
	uint64_t ex = block_excl_scan256_64(sum, tmp, total) + carry;
#pragma unroll
	for (int j = 0; j < kRunsScanPer; ++j) {
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		if (idx < count) w[idx] = ex;
		ex += v[j];
	}
	return total;
}
// (in place)
__device__ __forceinline__ uint64_t runs_scan_piece(uint64_t *__restrict__ w, uint32_t count, uint64_t carry, uint64_t *tmp)
{
	return runs_scan_piece(w, count, carry, tmp, [&](uint32_t idx) { return w[idx]; });
}

__global__ __launch_bounds__(kRunsScanTh) void runs_scan_pieces_kernel(uint64_t *__restrict__ tile_counts, uint64_t tiles, uint64_t *__restrict__ piece_sums)
{
	__shared__ uint64_t tmp[4];
	const uint64_t first = (uint64_t)blockIdx.x * kRunsScanTile;
	const uint32_t count = tiles - first < kRunsScanTile ? (uint32_t)(tiles - first) : kRunsScanTile;
	const uint64_t total = runs_scan_piece(tile_counts + first, count, 0, tmp);
	if (threadIdx.x == 0) piece_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kRunsScanTh) void runs_scan_top_kernel(uint64_t *__restrict__ piece_sums, uint64_t pieces, uint64_t *__restrict__ num_runs)
{
	__shared__ uint64_t tmp[4];
	uint64_t carry = 0;
	for (uint64_t first = 0; first < pieces; first += kRunsScanTile)
		carry += runs_scan_piece(piece_sums + first, pieces - first < kRunsScanTile ? (uint32_t)(pieces - first) : kRunsScanTile, carry, tmp);
	if (threadIdx.x == 0) *num_runs = carry;
}

// An empty input, of every entry point that counts: a count of zero, and with starts the terminator of no run
__global__ __launch_bounds__(64) void runs_empty_kernel(uint64_t *__restrict__ num_runs, uint64_t *__restrict__ starts)
{
	if (threadIdx.x != 0) return;
	*num_runs = 0;
	if (starts) starts[0] = 0;
}

// ---- step 3
// The heads of the tile -- value and place -- are compacted in the LDS at their run number within the tile and stored from
// there in the order of the runs: d_values and d_starts get coalesced stores however sparse the heads are.
// INV: every element stores its run number (POS: at the place its position names).  The run numbers cross the LDS, so
// that the stores -- and the loads of the positions -- are coalesced 8-byte accesses in the order of the elements.
template <typename E, bool INV, bool POS>
__global__ __launch_bounds__(kRunsTh) void runs_write_kernel(const E *__restrict__ data, uint64_t n, uint64_t cap, const uint64_t *__restrict__ tile_base,
	const uint64_t *__restrict__ piece_base, E *__restrict__ values, uint64_t *__restrict__ starts, const uint64_t *__restrict__ positions,
	uint64_t *__restrict__ inverse)
{
	typedef RunsCfg<E> C;
	constexpr uint32_t V = C::V;
	__shared__ uint32_t wsum[kRunsTh / 64];
	__shared__ __attribute__((aligned(16))) uint32_t rel[INV ? C::TILE : 1]; // heads of the tile up to and including the element
	__shared__ E head_val[C::TILE];                                            // the tile's heads, compacted: value ...
	__shared__ uint16_t head_at[C::TILE];                                      // ... and place in the tile
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, m = runs_misalign(data);
	const uint64_t tile = blockIdx.x, lo = m, hi = (uint64_t)m + n;
	const bool out = values || starts;
	E x[kRunsVecs][V];
	uint64_t hb[kRunsVecs][V];
	runs_load_heads<E>(data, n, m, tile, x, hb);
	const RunsRank rk = runs_rank<V>(hb, w, lane, wsum);
	const uint64_t base = tile_out_base(tile_base, piece_base, tile); // heads in front of the tile
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint32_t p0 = runs_place<E>(w, lane, k);
		const uint64_t v0 = tile * C::TILE + p0;
		uint32_t incl = rk.wpre + rk.before_k[k];
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) incl += popc_below_lane(hb[k][e]);
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			const uint64_t v = v0 + e;
			const bool head = lane_bit(hb[k][e]);
			incl += head ? 1u : 0u;
			if constexpr (INV) rel[p0 + e] = incl;
			if (head && out) { // (a head is inside the array; incl - 1 < the tile's heads <= TILE)
				head_val[incl - 1] = x[k][e];
				head_at[incl - 1] = (uint16_t)(p0 + e);
			}
			// the element that closes the array (element 0 is a head: base + incl >= 1)
			if (v == hi - 1 && base + incl <= cap && starts) starts[base + incl] = n;
		}
	}
	__syncthreads();
	if (out) { // the heads in the order of their runs: coalesced stores; run == cap is the terminator of a full output
		for (uint32_t j = threadIdx.x; j < rk.total; j += kRunsTh) {
			const uint64_t run = base + j;
			if (run > cap) break;
			if (starts) starts[run] = tile * C::TILE + head_at[j] - lo;
			if (run < cap && values) values[run] = head_val[j];
		}
	}
	if constexpr (INV) {
#pragma unroll 4
		for (uint32_t p = threadIdx.x; p < C::TILE; p += kRunsTh) {
			const uint64_t v = tile * C::TILE + p;
			if (v >= lo && v < hi) {
				const uint64_t i = v - lo;
				inverse[POS ? positions[i] : i] = base + rel[p] - 1;
			}
		}
	}
}

} // namespace msd

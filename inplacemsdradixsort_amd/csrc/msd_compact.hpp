// msd_compact.hpp -- stream compaction and stable partition: msd_compact.
//
// keep(i) = [ (no mask || mask[i] != 0) && (no range || lo <= code(keys[i]) <= hi) ] XOR invert.  The kept elements leave in
// their order (stable), with REST the rejected ones follow them in theirs.  Three stream-ordered steps, and no workgroup
// ever waits for another one (stream order is the only barrier between them):
//   1. compact_count_kernel: one workgroup per tile evaluates keep per element and counts, one word per tile.
//   2. runs_scan_pieces_kernel / runs_scan_top_kernel of msd_runs.hpp: the tile counts scanned in place, the
//      number of kept elements written to *d_count.
//   3. compact_write_kernel: reads each tile again, evaluates keep again, ranks every kept element (REST: every element) in
//      the tile, stages key and place in the LDS at that rank and stores from there in output order: coalesced stores
//      whatever the selectivity.  The values are loaded in the keys' lane layout and cross the same LDS buffer in a second
//      sweep; nothing is gathered from global memory.
//
// The geometry is that of msd_runs.hpp (RunsCfg<E>, virtual indices on the 16-byte grid, the partial 16 bytes at either end
// read element by element: runs_load_keys), and so are the count word, the ranks and the tile's base (runs_store_count,
// runs_rank, tile_out_base).  The grid is the keys' when keys are read, else the mask's with the 4-byte geometry.  The mask
// and the values lie at any phase of that grid: a lane's V mask bytes (V values) are one load where their address is
// aligned for it and lies inside the array, else one load per element; mask[-1] and mask[n] are never read.
#pragma once

#include <type_traits>

#include "msd_keycodec.hpp"
#include "msd_runs.hpp"

namespace msd {

// (the values of MSD_COMPACT_* in include/msd_compact_hip.h)
enum { kCompactRange = 1, kCompactInvert = 2, kCompactRest = 4 };

// What both kernels read.  keys: null where no kernel needs them (the count without a range test; the write without a
// range test and without d_out_keys).  lo, hi: CODES, looked at with RANGE only.
template <typename E> struct CompactIn {
	const E *keys;
	const uint8_t *mask;
	uint64_t n;
	uint32_t m; // elements between the last 16-byte boundary and element 0: the grid's phase
	uint32_t invert;
	KeyCodec<E> cd;
	E lo, hi;
};

// V elements that one lane loads at once where they are aligned for it
template <typename T, uint32_t V> struct alignas(V * sizeof(T) < 16 ? V * sizeof(T) : 16) CompactPack { T v[V]; };

// y[e] = base[v0 + e] for the virtual indices of [lo, hi), 0 for the others; base + v0 is never dereferenced outside
template <typename T, uint32_t V> __device__ __forceinline__ void compact_load_lane(const T *__restrict__ base, uint64_t v0, uint64_t lo, uint64_t hi, T (&y)[V])
{
	typedef CompactPack<T, V> Pack;
	const T *const p = base + v0;
	if (v0 >= lo && v0 + V <= hi && ((uintptr_t)p & (alignof(Pack) - 1)) == 0) {
		const Pack q = *reinterpret_cast<const Pack *>(p);
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) y[e] = q.v[e];
	} else {
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) y[e] = (v0 + e >= lo && v0 + e < hi) ? p[e] : (T)0;
	}
}

// This lane's keys of tile `tile` (runs_load_keys of msd_runs.hpp; zeros without keys) and the ballots of keep, one per (k, e)
template <typename E, bool RANGE, bool MASK>
__device__ __forceinline__ void compact_load_keep(const CompactIn<E> &in, uint64_t tile, uint32_t w, uint32_t lane, E (&x)[kRunsVecs][RunsCfg<E>::V],
	uint64_t (&kb)[kRunsVecs][RunsCfg<E>::V])
{
	constexpr uint32_t V = RunsCfg<E>::V;
	const uint64_t lo = in.m, hi = (uint64_t)in.m + in.n; // the array in virtual indices
	uint8_t mb[kRunsVecs][V];
	if (in.keys) {
		runs_load_keys<E>(in.keys - in.m, lo, hi, tile, w, lane, x);
	} else {
#pragma unroll
		for (int k = 0; k < kRunsVecs; ++k)
#pragma unroll
			for (uint32_t e = 0; e < V; ++e) x[k][e] = 0;
	}
	if constexpr (MASK) {
#pragma unroll
		for (int k = 0; k < kRunsVecs; ++k) compact_load_lane<uint8_t, V>(in.mask - in.m, runs_vindex<E>(tile, w, lane, k), lo, hi, mb[k]);
	}
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint64_t v0 = runs_vindex<E>(tile, w, lane, k);
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			const uint64_t v = v0 + e;
			bool pass = true;
			if constexpr (MASK) pass = mb[k][e] != 0;
			if constexpr (RANGE) {
				const E code = in.cd.enc(x[k][e]);
				pass = pass && code >= in.lo && code <= in.hi;
			}
			kb[k][e] = __ballot(v >= lo && v < hi && pass != (in.invert != 0));
		}
	}
}

// ---- step 1
template <typename E, bool RANGE, bool MASK>
__global__ __launch_bounds__(kRunsTh) void compact_count_kernel(CompactIn<E> in, uint64_t *__restrict__ tile_counts)
{
	typedef RunsCfg<E> C;
	E x[kRunsVecs][C::V];
	uint64_t kb[kRunsVecs][C::V];
	compact_load_keep<E, RANGE, MASK>(in, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63u, x, kb);
	runs_store_count<C::V>(kb, tile_counts);
}

// ---- step 3
// f(k, e, slot) for every element of this lane that is staged: a kept one at its rank among the tile's kept elements; with
// REST a rejected one behind the `kept` kept ones, at its rank among the rejected.  The elements of the array are the places
// [pstart, pend) of the tile, so the rejected in front of place p are (p - pstart) minus the kept in front of it.
template <typename E, bool REST, typename F>
__device__ __forceinline__ void compact_for_slots(const uint64_t (&kb)[kRunsVecs][RunsCfg<E>::V], const RunsRank &rk, uint32_t pstart, uint32_t pend, F &&f)
{
	constexpr uint32_t V = RunsCfg<E>::V;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, kept = rk.total;
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint32_t p0 = runs_place<E>(w, lane, k);
		uint32_t r = rk.wpre + rk.before_k[k]; // kept elements of the tile in front of the element
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) r += popc_below_lane(kb[k][e]);
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			const uint32_t p = p0 + e;
			const bool keep = lane_bit(kb[k][e]); // (a kept element is inside the array; r < kept <= TILE)
			if (keep)
				f(k, e, r, p);
			else if (REST && p >= pstart && p < pend)
				f(k, e, kept + (p - pstart - r), p); // (< pend - pstart <= TILE)
			r += keep ? 1u : 0u;
		}
	}
}

// The staged elements of the tile -- key and place, then the value -- leave the LDS in output order: slot j of the kept ones
// to index (kept in front of the tile) + j, stopping at cap; with REST slot kept + j to (all kept) + (rejected in front of
// the tile) + j.  VB: the values' width, 0 without values.
template <typename E, bool RANGE, bool MASK, int VB, bool REST>
__global__ __launch_bounds__(kRunsTh) void compact_write_kernel(CompactIn<E> in, const void *__restrict__ vals, uint64_t cap, const uint64_t *__restrict__ tile_base,
	const uint64_t *__restrict__ piece_base, const uint64_t *__restrict__ total, E *__restrict__ out_keys, void *__restrict__ out_vals, uint64_t *__restrict__ out_idx)
{
	typedef RunsCfg<E> C;
	typedef typename std::conditional<VB == 8, uint64_t, uint32_t>::type VT;
	constexpr uint32_t V = C::V;
	constexpr uint32_t SB = sizeof(E) > (size_t)VB ? sizeof(E) : (size_t)VB; // bytes of a staged key or value
	__shared__ uint32_t wsum[kRunsTh / 64];
	__shared__ __attribute__((aligned(16))) unsigned char stage[C::TILE * SB]; // the keys at their slots, then the values
	__shared__ uint16_t at[C::TILE];                                           // the place in the tile of the element at a slot
	E *const skey = reinterpret_cast<E *>(stage);
	VT *const sval = reinterpret_cast<VT *>(stage);
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint64_t tile = blockIdx.x, t0 = tile * C::TILE, lo = in.m, hi = (uint64_t)in.m + in.n;
	E x[kRunsVecs][V];
	uint64_t kb[kRunsVecs][V];
	compact_load_keep<E, RANGE, MASK>(in, tile, w, lane, x, kb);
	VT y[VB ? kRunsVecs : 1][V];
	if constexpr (VB != 0) { // (in flight while the keys are staged)
#pragma unroll
		for (int k = 0; k < kRunsVecs; ++k) compact_load_lane<VT, V>(static_cast<const VT *>(vals) - in.m, runs_vindex<E>(tile, w, lane, k), lo, hi, y[k]);
	}
	const RunsRank rk = runs_rank<V>(kb, w, lane, wsum);
	const uint32_t kept = rk.total;
	const uint32_t pstart = lo > t0 ? (uint32_t)(lo - t0) : 0u, pend = hi - t0 < C::TILE ? (uint32_t)(hi - t0) : C::TILE; // (tile < tiles: hi > t0)
	const uint32_t staged = REST ? pend - pstart : kept;
	const uint64_t base = tile_out_base(tile_base, piece_base, tile);         // kept elements in front of the tile
	uint64_t rest_base = 0;                                                   // where slot `kept` goes
	if constexpr (REST) rest_base = *total + ((t0 + pstart - lo) - base);
	const auto dst_of = [&](uint32_t j) { return j < kept ? base + j : rest_base + (j - kept); };

	compact_for_slots<E, REST>(kb, rk, pstart, pend, [&](int k, uint32_t e, uint32_t slot, uint32_t p) {
		if (out_keys) skey[slot] = x[k][e];
		at[slot] = (uint16_t)p;
	});
	__syncthreads();
	if (out_keys || out_idx) {
		for (uint32_t j = threadIdx.x; j < staged; j += kRunsTh) {
			const uint64_t dst = dst_of(j);
			if (!REST && dst >= cap) break; // (REST: cap >= n)
			if (out_keys) out_keys[dst] = skey[j];
			if (out_idx) out_idx[dst] = t0 + at[j] - lo;
		}
	}
	if constexpr (VB != 0) {
		__syncthreads(); // (the keys have left the buffer)
		compact_for_slots<E, REST>(kb, rk, pstart, pend, [&](int k, uint32_t e, uint32_t slot, uint32_t) { sval[slot] = y[k][e]; });
		__syncthreads();
		for (uint32_t j = threadIdx.x; j < staged; j += kRunsTh) {
			const uint64_t dst = dst_of(j);
			if (!REST && dst >= cap) break;
			static_cast<VT *>(out_vals)[dst] = sval[j];
		}
	}
}

} // namespace msd

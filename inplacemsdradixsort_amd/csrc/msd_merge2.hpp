// msd_merge2.hpp -- merge of two sorted arrays: msd_merge_sorted, and the pieces every tile kernel
// of the merge path shares (msd_setops.hpp, msd_join.hpp): lds_count_per, merge_store, tile_out_window, ballot_compact.
//
// a (n keys) and b (m keys) are ascending by CODE (msd_keycodec.hpp); the output is the stable sort of the concatenation
// [a; b] by code: among equal codes all of a's come before all of b's, and within one side equal keys keep their order.
// Think of the merged sequence with the tie rule "b after every a that is not larger" -- the RIGHT rule of msd_search.hpp,
// with b in the role of the needles.  Two kernels, no atomics, and no workgroup ever waits for another one:
//   1. search_split_kernel (msd_search.hpp) with the RIGHT rule: one thread per diagonal d_i = min(i * TILE, n + m) finds by
//      binary search (the merge path) how many elements of a (a_i) and of b (b_i = d_i - a_i) the first d_i elements of the
//      merged sequence hold, and writes a_i.
//   2. merge_tile_kernel: one workgroup per tile i loads a[a_i, a_{i+1}) and b[b_i, b_{i+1}) -- together at most TILE
//      elements -- as codes into the LDS and RANKS every one of them inside the tile:
//         local a element e goes to e + |{ b in tile : code(b) <  code(a_e) }|
//         local b element j goes to j + |{ a in tile : code(a) <= code(b_j) }|
//      which is a bijection onto [0, na + nb) for ascending inputs (the stable merge of the tile).  The DECODED key goes to
//      its rank in a second LDS array, with VALS or ORIGIN the element's local index to a third one; behind a barrier the
//      tile's slice out[d_i, d_{i+1}) is stored coalesced (whole aligned 16 bytes where the slice covers them: merge_store is
//      the mirror of search_stage), and position p loads its 8-byte value from vals_a / vals_b through the local index --
//      ascending per side -- and stores it and the origin coalesced.  Stream order is the only barrier between the launches.
// Every extent is CLAMPED (merge_tile_extent of msd_search.hpp, and merge_tile_kernel): inputs that are not ascending give
// unspecified output VALUES, but every load stays inside its input array and every store inside [0, n + m) of its output.
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"
#include "msd_runs.hpp"   // tile_out_base: the scanned tile counts
#include "msd_search.hpp" // search_split_kernel, merge_tile_extent, search_stage, search_counts

namespace msd {

constexpr int kMergeTh = kSearchTh; // threads of both kernels (search_stage strides by kSearchTh)
constexpr int kMergePer = 4;        // elements one lane ranks side by side: their dependent LDS reads overlap
template <typename K> struct MergeCfg {
	static constexpr uint32_t V = Vec16<K>::N;            // elements per 16 bytes
	static constexpr uint32_t TILE = kMergeTh * 4u * V;   // elements of a plus b of one workgroup: 4096 (4-byte), 2048 (8-byte): 2 x 16 KiB of LDS for codes and keys
};

// lds_count (msd_search.hpp) for kMergePer elements side by side: base[v] = |{ k in other[0, len) : k counts for x[v] }|.
// All reads of a step come first, so the dependent LDS reads of the kMergePer searches overlap.
template <typename K>
__device__ __forceinline__ void lds_count_per(const K *__restrict__ other, uint32_t len, const K (&x)[kMergePer], bool right, uint32_t (&base)[kMergePer])
{
#pragma unroll
	for (int v = 0; v < kMergePer; ++v) base[v] = 0;
	if (len) { // (uniform)
		uint32_t l = len; // invariant: the count lies in [base, base + l], base + l <= len
		while (l > 1) {
			const uint32_t half = l >> 1;
			K k[kMergePer];
#pragma unroll
			for (int v = 0; v < kMergePer; ++v) k[v] = other[base[v] + half - 1];
#pragma unroll
			for (int v = 0; v < kMergePer; ++v) base[v] += search_counts(k[v], x[v], right) ? half : 0u;
			l -= half;
		}
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) base[v] += search_counts(other[base[v]], x[v], right) ? 1u : 0u; // (base < len)
	}
}

// The `count` codes at codes[self0 ..] against the `len` codes at codes[other0 ..] (both ascending), kMergePer per lane:
// f(e, x, base) for every element e < count, x its code and base the number of the others that count for it (RIGHT: <=,
// else <).  What every tile kernel of the merge path decides, it decides in f.  (Every thread of the workgroup calls it.)
template <typename K, bool RIGHT, typename F>
__device__ __forceinline__ void merge_for_counts(const K *__restrict__ codes, uint32_t self0, uint32_t count, uint32_t other0, uint32_t len, F &&f)
{
	for (uint32_t e0 = threadIdx.x; e0 < count; e0 += kMergeTh * kMergePer) {
		K x[kMergePer];
		uint32_t base[kMergePer];
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) {
			const uint32_t e = e0 + (uint32_t)v * kMergeTh;
			x[v] = codes[self0 + (e < count ? e : count - 1)]; // (a lane beyond the end searches the last element again and f is not called)
		}
		lds_count_per<K>(codes + other0, len, x, RIGHT, base);
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) {
			const uint32_t e = e0 + (uint32_t)v * kMergeTh;
			if (e < count) f(e, x[v], base[v]);
		}
	}
}

// Element e of merge_for_counts goes to e + base, clamped to `last`; its decoded key goes there in outk, its local index
// self0 + e in src.
template <typename K, bool RIGHT, bool SRC>
__device__ __forceinline__ void merge_rank(const K *__restrict__ codes, uint32_t self0, uint32_t count, uint32_t other0, uint32_t len, uint32_t last, KeyCodec<K> cd,
	K *__restrict__ outk, uint16_t *__restrict__ src)
{
	merge_for_counts<K, RIGHT>(codes, self0, count, other0, len, [&](uint32_t e, K x, uint32_t base) {
		const uint32_t r = e + base < last ? e + base : last;
		outk[r] = cd.dec(x);
		if constexpr (SRC) src[r] = (uint16_t)(self0 + e); // (< TILE <= 4096)
	});
}

// `count` elements from the LDS at from to dst (element alignment only): the mirror of search_stage.  Every 16 bytes that lie
// wholly inside the range are one aligned store, the partly covered 16 bytes at its two ends are written element by
// element; nothing outside [dst, dst + count) is written.  (Every thread of the workgroup calls it.)
template <typename K> __device__ __forceinline__ void merge_store(const K *__restrict__ from, uint32_t count, K *__restrict__ dst)
{
	constexpr uint32_t V = MergeCfg<K>::V;
	const uint32_t mis = (uint32_t)(((uintptr_t)dst & 15u) / sizeof(K)); // elements between the last 16-byte boundary and dst
	K *const vbase = dst - mis;                                            // (16-byte aligned; dereferenced inside the range only)
	for (uint32_t v0 = threadIdx.x * V; v0 < mis + count; v0 += kMergeTh * V) { // virtual index: element e has v = e + mis
		if (v0 >= mis && v0 + V <= mis + count) {
			const K *const f = from + (v0 - mis);
			u32x4 q;
			if constexpr (sizeof(K) == 4) {
				q = u32x4{ f[0], f[1], f[2], f[3] };
			} else {
				q = u32x4{ (uint32_t)f[0], (uint32_t)(f[0] >> 32), (uint32_t)f[1], (uint32_t)(f[1] >> 32) };
			}
			*reinterpret_cast<u32x4 *>(vbase + v0) = q;
		} else {
#pragma unroll
			for (uint32_t e = 0; e < V; ++e)
				if (v0 + e >= mis && v0 + e < mis + count) vbase[v0 + e] = from[v0 + e - mis];
		}
	}
}

// ---- step 2
// The clamps of merge_tile_extent (vals_a and vals_b are read where a and b are), and: cnt = the positions stored, at most
// the tile's slice d_{i+1} - d_i, so every store is at d_i + p < d_{i+1} <= n + m.  Every rank is clamped to na + nb - 1
// before it indexes the LDS, and every staged local index on read, so a position that no element was ranked to (inputs
// that are not ascending) stores whatever the LDS held -- but loads inside the inputs.  For ascending inputs the clamps
// change nothing: na + nb = d_{i+1} - d_i <= TILE and the ranks are a bijection.
template <typename K, bool VALS, bool ORIGIN>
__global__ __launch_bounds__(kMergeTh) void merge_tile_kernel(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd,
	const uint64_t *__restrict__ splits, const uint64_t *__restrict__ vals_a, const uint64_t *__restrict__ vals_b, K *__restrict__ out, uint64_t *__restrict__ out_vals,
	uint64_t *__restrict__ out_origin)
{
	constexpr uint32_t TILE = MergeCfg<K>::TILE;
	constexpr bool SRC = VALS || ORIGIN;
	__shared__ K codes[TILE];                // the tile's a as codes, the tile's b as codes behind them
	__shared__ K outk[TILE];                 // the merged keys, decoded
	__shared__ uint16_t src[SRC ? TILE : 1]; // per position the local index of its element: < na from a, else from b
	const MergeTileExtent t = merge_tile_extent<TILE>(blockIdx.x, n, m, splits);
	const uint64_t d0 = t.d0, a0 = t.a0, b0 = t.b0;
	const uint32_t na = t.na, nb = t.nb;
	const uint32_t cnt = na + nb < t.d1 - d0 ? na + nb : (uint32_t)(t.d1 - d0);
	if (cnt == 0) return; // (uniform: the barriers below are never reached by a part of the workgroup)
	const uint32_t last = na + nb - 1;
	search_stage<K>(a + a0, na, cd, codes);
	search_stage<K>(b + b0, nb, cd, codes + na);
	__syncthreads();
	merge_rank<K, false, SRC>(codes, 0, na, na, nb, last, cd, outk, src);  // a: the b that are smaller
	merge_rank<K, true, SRC>(codes, na, nb, 0, na, last, cd, outk, src);   // b: the a that are not larger
	__syncthreads();
	merge_store<K>(outk, cnt, out + d0);
	if constexpr (SRC) {
		for (uint32_t p = threadIdx.x; p < cnt; p += kMergeTh) {
			const uint32_t s = src[p] < last ? src[p] : last;
			const bool from_a = s < na;
			const uint64_t at = from_a ? a0 + s : b0 + (s - na); // (< n, < m)
			if constexpr (VALS) out_vals[d0 + p] = from_a ? vals_a[at] : vals_b[at];
			if constexpr (ORIGIN) out_origin[d0 + p] = from_a ? at : n + at;
		}
	}
}

// ---- what the writers behind a count and a scan share (msd_setops.hpp, msd_join.hpp)

// Tile blockIdx.x stores to [base, lim): base = its scanned count, lim = min(the next tile's base -- *total for the last
// tile --, cap): at most the number the count kernel counted, whatever the writer decides.  base >= lim: nothing to store,
// and the writer leaves before it loads anything (uniform).
struct TileOutWindow {
	uint64_t base, lim;
};
__device__ __forceinline__ TileOutWindow tile_out_window(const uint64_t *__restrict__ tile_base, const uint64_t *__restrict__ piece_base, const uint64_t *__restrict__ total,
	uint64_t cap)
{
	const uint64_t i = blockIdx.x;
	const uint64_t next = i + 1 < gridDim.x ? tile_out_base(tile_base, piece_base, i + 1) : *total;
	return TileOutWindow{ tile_out_base(tile_base, piece_base, i), next < cap ? next : cap };
}

constexpr uint16_t kSetNone = 0xFFFFu; // in place of a 16-bit word of a tile (< TILE <= 4096): the place holds no kept element

// The compaction: mark[r], r < count <= 64 * 4 * PER, is kSetNone or the word of a kept element.  Wave w owns the places
// [w * 64 * PER, (w + 1) * 64 * PER), 64 at a time; the places that hold a kept element are one ballot, the kept ones in front
// of a place are popcounts -- of the ballots of the places in front of the wave's, which the wave forms itself (no word of
// LDS), of the wave's own earlier ballots, and of the lower lanes' bits.  place(r, to, mark[r]) for every kept element whose
// rank `to` among the kept is below cnt.  INPLACE: place may overwrite mark -- all of it is read in front of a barrier.
// (Every thread of the workgroup calls it.)
template <uint32_t PER, bool INPLACE, typename F>
__device__ __forceinline__ void ballot_compact(const uint16_t *mark, uint32_t count, uint32_t cnt, F &&place)
{
	const uint32_t lane = threadIdx.x & 63u, first = (threadIdx.x >> 6) * PER; // the wave's first ballot
	uint32_t before = 0; // kept elements in front of the ballot at hand (uniform)
	for (uint32_t c = 0; c < first; ++c) {
		const uint32_t r = c * 64u + lane;
		before += (uint32_t)__popcll(__ballot(r < count && mark[r] != kSetNone));
	}
	uint16_t s[PER];
	uint64_t bits[PER];
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k) {
		const uint32_t r = (first + k) * 64u + lane;
		s[k] = r < count ? mark[r] : kSetNone;
		bits[k] = __ballot(s[k] != kSetNone);
	}
	if constexpr (INPLACE) __syncthreads();
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k) {
		const uint32_t r = (first + k) * 64u + lane, to = before + popc_below_lane(bits[k]);
		if (s[k] != kSetNone && to < cnt) place(r, to, s[k]);
		before += (uint32_t)__popcll(bits[k]);
	}
}

} // namespace msd

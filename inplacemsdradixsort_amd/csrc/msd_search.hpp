// msd_search.hpp -- sorted search: msd_search_sorted.
//
// For every needle the number of keys of a sorted array whose CODE (msd_keycodec.hpp) is < the needle's (LEFT, the lower
// bound) or <= it (RIGHT, the upper bound).  `side` is a run-time argument: a key counts iff code(key) < code(needle) + side,
// written below as (k < x) | (right & (k == x)) so that an all-ones needle needs no special case.
//
// Two paths, no atomics, and no workgroup ever waits for another one:
//   DIRECT (any needles): search_direct_kernel.  Every lane searches kSearchPer needles at once by a branch-free binary search
//      whose trip count depends on n only; the kSearchPer loads of a step are independent of each other, so the latency of a
//      dependent load is overlapped kSearchPer times.  Needles are loaded and results stored coalesced.
//   MERGE (needles ascending in the same order): think of keys and needles merged into ONE sequence in which a needle goes
//      before every key that is not smaller (LEFT) or after every key that is not larger (RIGHT).  The keys in front of needle
//      j in that sequence are exactly the keys it counts, so r_j = the number of keys consumed when needle j is reached.
//      1. search_split_kernel: one thread per diagonal d_i = min(i * TILE, n + m) finds by binary search (the merge path) how
//         many keys a_i and needles b_i = d_i - a_i the first d_i elements of the sequence hold, and writes a_i.
//      2. search_tile_kernel: one workgroup per tile i loads key[a_i, a_{i+1}) and needle[b_i, b_{i+1}) -- together at most
//         TILE elements -- as codes into the LDS; every needle of the tile binary-searches the tile's keys there and stores
//         a_i + local.  Stream order is the only barrier between the two launches.
//      Every extent is CLAMPED (see merge_tile_extent): needles that are not ascending give unspecified results, but every load
//      stays inside the two arrays and every store inside d_out[0, m).
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"

namespace msd {

constexpr int kSearchTh = 256;  // threads of every kernel of this file
constexpr int kSearchPer = 4;   // direct: needles per lane, searched side by side
constexpr uint32_t kSearchDirectTile = kSearchTh * kSearchPer; // direct: needles of one workgroup
template <typename K> struct SearchCfg {
	static constexpr uint32_t V = Vec16<K>::N;             // elements per 16 bytes
	static constexpr uint32_t TILE = kSearchTh * 4u * V;   // merge: keys plus needles of one workgroup: 4096 (4-byte), 2048 (8-byte); 16 KiB of LDS
};

// (search_counts, lds_count and merge_tile_extent -- and join_global_upper of msd_join.hpp -- are __host__ as well for one
// caller: tests/clamp_main.hip runs these index functions on the host, on inputs that are not ascending.)
// does a key with code k count for a needle with code x?
template <typename K> __host__ __device__ __forceinline__ bool search_counts(K k, K x, bool right) { return (k < x) | (right & (k == x)); }

// |{ k in codes[0, len) : k counts for x }| over ascending codes in the LDS: the branch-free search of the direct kernel,
// whose trip count depends on len only.  (The kMergePer searches side by side: lds_count_per of msd_merge2.hpp.)
template <typename K> __host__ __device__ __forceinline__ uint32_t lds_count(const K *__restrict__ codes, uint32_t len, K x, bool right)
{
	uint32_t base = 0;
	if (len) {
		uint32_t l = len; // invariant: the count lies in [base, base + l], base + l <= len
		while (l > 1) {
			const uint32_t half = l >> 1;
			base += search_counts(codes[base + half - 1], x, right) ? half : 0u;
			l -= half;
		}
		base += search_counts(codes[base], x, right) ? 1u : 0u; // (base < len)
	}
	return base;
}

// ---- direct
template <typename K, bool POS>
__global__ __launch_bounds__(kSearchTh) void search_direct_kernel(const K *__restrict__ keys, uint64_t n, const K *__restrict__ needles, uint64_t m, uint32_t right,
	KeyCodec<K> cd, const uint64_t *__restrict__ positions, uint64_t *__restrict__ out)
{
	const uint64_t j0 = (uint64_t)blockIdx.x * kSearchDirectTile + threadIdx.x; // (m > 0: the host launches nothing otherwise)
	K x[kSearchPer];
	uint64_t base[kSearchPer];
#pragma unroll
	for (int v = 0; v < kSearchPer; ++v) {
		const uint64_t j = j0 + (uint64_t)v * kSearchTh;
		x[v] = cd.enc(needles[j < m ? j : m - 1]); // (a lane beyond the end searches the last needle again and stores nothing)
		base[v] = 0;
	}
	if (n) {
		uint64_t len = n; // invariant: the result lies in [base, base + len], base + len <= n
		while (len > 1) {
			const uint64_t half = len >> 1;
			K k[kSearchPer];
#pragma unroll
			for (int v = 0; v < kSearchPer; ++v) k[v] = keys[base[v] + half - 1]; // (all loads of the step first)
#pragma unroll
			for (int v = 0; v < kSearchPer; ++v) base[v] += search_counts(cd.enc(k[v]), x[v], right != 0) ? half : 0;
			len -= half;
		}
		K k[kSearchPer];
#pragma unroll
		for (int v = 0; v < kSearchPer; ++v) k[v] = keys[base[v]]; // (base < n)
#pragma unroll
		for (int v = 0; v < kSearchPer; ++v) base[v] += search_counts(cd.enc(k[v]), x[v], right != 0) ? 1u : 0u;
	}
#pragma unroll
	for (int v = 0; v < kSearchPer; ++v) {
		const uint64_t j = j0 + (uint64_t)v * kSearchTh;
		if (j < m) out[POS ? positions[j] : j] = base[v];
	}
}

// ---- merge, step 1 (and step 1 of msd_merge2.hpp, msd_setops.hpp and msd_join.hpp: the RIGHT rule, b in the role of the
// needles -- "b[mid] precedes a[d - mid - 1] iff it is strictly smaller" is the RIGHT case below, code for code)
// splits[i] = a_i for i = 0 .. tiles (tiles + 1 words).  b counts the needles among the first d elements of the merged
// sequence: needle b is among them iff it PRECEDES key[d - b - 1] (<= for LEFT, < for RIGHT), which is monotone in b for
// ascending needles.  The search stays inside [max(0, d - n), min(d, m)] whatever the needles hold: mid < m and
// 0 <= d - mid - 1 < n for every probe, and 0 <= a_i <= n, 0 <= d - a_i <= m for every result.
template <typename K, uint32_t TILE>
__global__ __launch_bounds__(kSearchTh) void search_split_kernel(const K *__restrict__ keys, uint64_t n, const K *__restrict__ needles, uint64_t m, uint32_t right,
	KeyCodec<K> cd, uint64_t tiles, uint64_t *__restrict__ splits)
{
	const uint64_t i = (uint64_t)blockIdx.x * kSearchTh + threadIdx.x;
	if (i > tiles) return;
	const uint64_t total = n + m, d = i * TILE < total ? i * TILE : total;
	uint64_t lo = d > n ? d - n : 0, hi = d < m ? d : m;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		const K x = cd.enc(needles[mid]), k = cd.enc(keys[d - mid - 1]);
		const bool precedes = right ? x < k : x <= k;
		if (precedes) lo = mid + 1;
		else hi = mid;
	}
	splits[i] = d - lo;
}

// `count` elements from src (element alignment only) as codes to the LDS at dst: every 16 bytes that lie wholly inside the
// range are one aligned load, the partly covered 16 bytes at its two ends are read element by element; nothing outside
// [src, src + count) is read.  (Every thread of the workgroup calls it.)
template <typename K> __device__ __forceinline__ void search_stage(const K *__restrict__ src, uint32_t count, KeyCodec<K> cd, K *__restrict__ dst)
{
	constexpr uint32_t V = SearchCfg<K>::V;
	const uint32_t mis = (uint32_t)(((uintptr_t)src & 15u) / sizeof(K)); // elements between the last 16-byte boundary and src
	const K *const vbase = src - mis;                                      // (16-byte aligned; dereferenced inside the range only)
	for (uint32_t v0 = threadIdx.x * V; v0 < mis + count; v0 += kSearchTh * V) { // virtual index: element e has v = e + mis
		if (v0 >= mis && v0 + V <= mis + count) {
			K x[V];
			vec16_unpack<K>(*reinterpret_cast<const u32x4 *>(vbase + v0), x);
			K *const to = dst + (v0 - mis);
#pragma unroll
			for (uint32_t e = 0; e < V; ++e) to[e] = cd.enc(x[e]);
		} else {
#pragma unroll
			for (uint32_t e = 0; e < V; ++e)
				if (v0 + e >= mis && v0 + e < mis + count) dst[v0 + e - mis] = cd.enc(vbase[v0 + e]);
		}
	}
}

// ---- merge, step 2
// Tile i of the merged sequence of a (n elements: the keys) and b (m elements: the needles), as the splits cut it, for every
// tile kernel of the merge path.  The clamps: na = the tile's a, at most TILE and 0 if the splits are not ascending; nb = its
// b, at most what is left of TILE and 0 if b_{i+1} < b_i.  With 0 <= a_i <= a_{i+1} <= n the loads are a[a0, a0 + na)
// inside [0, n); with 0 <= b_i <= b_{i+1} <= m the loads and stores are at [b0, b0 + nb) inside [0, m).  For ascending inputs
// the clamps change nothing: na + nb = d1 - d0 <= TILE.  (All uniform.)
struct MergeTileExtent {
	uint64_t d0, d1, a0, b0;
	uint32_t na, nb;
};
template <uint32_t TILE> __host__ __device__ __forceinline__ MergeTileExtent merge_tile_extent(uint64_t i, uint64_t n, uint64_t m, const uint64_t *__restrict__ splits)
{
	MergeTileExtent t;
	const uint64_t total = n + m;
	t.d0 = i * TILE < total ? i * TILE : total;
	t.d1 = (i + 1) * TILE < total ? (i + 1) * TILE : total;
	const uint64_t a1 = splits[i + 1], b1 = t.d1 - a1;
	t.a0 = splits[i];
	t.b0 = t.d0 - t.a0;
	t.na = a1 > t.a0 ? (uint32_t)(a1 - t.a0 < TILE ? a1 - t.a0 : TILE) : 0u;
	t.nb = b1 > t.b0 ? (uint32_t)(b1 - t.b0 < TILE - t.na ? b1 - t.b0 : TILE - t.na) : 0u;
	return t;
}

template <typename K, bool POS>
__global__ __launch_bounds__(kSearchTh) void search_tile_kernel(const K *__restrict__ keys, uint64_t n, const K *__restrict__ needles, uint64_t m, uint32_t right,
	KeyCodec<K> cd, const uint64_t *__restrict__ splits, const uint64_t *__restrict__ positions, uint64_t *__restrict__ out)
{
	constexpr uint32_t TILE = SearchCfg<K>::TILE;
	__shared__ K lds[TILE]; // the tile's keys as codes, the tile's needles as codes behind them
	const MergeTileExtent t = merge_tile_extent<TILE>(blockIdx.x, n, m, splits);
	const uint64_t a0 = t.a0, b0 = t.b0;
	const uint32_t na = t.na, nb = t.nb;
	if (nb == 0) return; // a tile of keys only: nothing to store (uniform: the barrier below is never reached by a part of the workgroup)
	search_stage<K>(keys + a0, na, cd, lds);
	search_stage<K>(needles + b0, nb, cd, lds + na);
	__syncthreads();
	for (uint32_t j = threadIdx.x; j < nb; j += kSearchTh) {
		// lds_count(lds, na, x, right), spelled out: the one exception to "one definition" (DESIGN.md 1.1).  Called as a
		// function the same search compiles to other tests around the loop, and the call was measured 2.5 % slower.
		const K x = lds[na + j];
		uint32_t base = 0;
		if (na) { // (uniform)
			uint32_t len = na;
			while (len > 1) {
				const uint32_t half = len >> 1;
				base += search_counts(lds[base + half - 1], x, right != 0) ? half : 0u;
				len -= half;
			}
			base += search_counts(lds[base], x, right != 0) ? 1u : 0u;
		}
		const uint64_t at = b0 + j;
		out[POS ? positions[at] : at] = a0 + base;
	}
}

} // namespace msd

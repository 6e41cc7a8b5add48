// msd_merge2.hpp -- merge of two sorted arrays: msd_merge_sorted.
//
// a (n keys) and b (m keys) are ascending by CODE (msd_keycodec.hpp); the output is the stable sort of the concatenation
// [a; b] by code: among equal codes all of a's come before all of b's, and within one side equal keys keep their order.
// Think of the merged sequence with the tie rule "b after every a that is not larger" -- the RIGHT rule of msd_search.hpp,
// with b in the role of the needles.  Two kernels, no atomics, and no workgroup ever waits for another one:
//   1. merge_split_kernel: one thread per diagonal d_i = min(i * TILE, n + m) finds by binary search (the merge path) how many
//      elements of a (a_i) and of b (b_i = d_i - a_i) the first d_i elements of the merged sequence hold, and writes a_i.
//   2. merge_tile_kernel: one workgroup per tile i loads a[a_i, a_{i+1}) and b[b_i, b_{i+1}) -- together at most TILE
//      elements -- as codes into the LDS and RANKS every one of them inside the tile:
//         local a element e goes to e + |{ b in tile : code(b) <  code(a_e) }|
//         local b element j goes to j + |{ a in tile : code(a) <= code(b_j) }|
//      which is a bijection onto [0, na + nb) for ascending inputs (the stable merge of the tile).  The DECODED key goes to
//      its rank in a second LDS array, with VALS or ORIGIN the element's local index to a third one; behind a barrier the
//      tile's slice out[d_i, d_{i+1}) is stored coalesced (whole aligned 16 bytes where the slice covers them: merge_store is
//      the mirror of search_stage), and position p loads its 8-byte value from vals_a / vals_b through the local index --
//      ascending per side -- and stores it and the origin coalesced.  Stream order is the only barrier between the launches.
// Every extent is CLAMPED (see merge_tile_kernel): inputs that are not ascending give unspecified output VALUES, but every
// load stays inside its input array and every store inside [0, n + m) of its output.
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"
#include "msd_search.hpp" // search_stage, search_counts

namespace msd {

constexpr int kMergeTh = kSearchTh; // threads of both kernels (search_stage strides by kSearchTh)
constexpr int kMergePer = 4;        // elements one lane ranks side by side: their dependent LDS reads overlap
template <typename K> struct MergeCfg {
	static constexpr uint32_t V = Vec16<K>::N;            // elements per 16 bytes
	static constexpr uint32_t TILE = kMergeTh * 4u * V;   // elements of a plus b of one workgroup: 4096 (4-byte), 2048 (8-byte): 2 x 16 KiB of LDS for codes and keys
};

// ---- step 1
// splits[i] = a_i for i = 0 .. tiles (tiles + 1 words): search_split_kernel with the RIGHT rule and the merge's own TILE.
// b counts the elements of b among the first d of the merged sequence: b[mid] is among them iff it PRECEDES a[d - mid - 1],
// i.e. is strictly smaller.  The search stays inside [max(0, d - n), min(d, m)] whatever the arrays hold: mid < m and
// 0 <= d - mid - 1 < n for every probe, and 0 <= a_i <= n, 0 <= d - a_i <= m for every result.
template <typename K>
__global__ __launch_bounds__(kMergeTh) void merge_split_kernel(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd, uint64_t tiles,
	uint64_t *__restrict__ splits)
{
	const uint64_t i = (uint64_t)blockIdx.x * kMergeTh + threadIdx.x;
	if (i > tiles) return;
	const uint64_t total = n + m, d = i * MergeCfg<K>::TILE < total ? i * MergeCfg<K>::TILE : total;
	uint64_t lo = d > n ? d - n : 0, hi = d < m ? d : m;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if (cd.enc(b[mid]) < cd.enc(a[d - mid - 1])) lo = mid + 1;
		else hi = mid;
	}
	splits[i] = d - lo;
}

// The `count` codes at codes[self0 ..] are ranked against the `len` codes at codes[other0 ..] (both ascending): element e goes
// to e + the number of the others that count for it (RIGHT: <=, else <), clamped to `last`; its decoded key goes there in
// outk, its local index self0 + e in src.  kMergePer branch-free searches per lane whose trip count depends on len only.
// (Every thread of the workgroup calls it.)
template <typename K, bool RIGHT, bool SRC>
__device__ __forceinline__ void merge_rank(const K *__restrict__ codes, uint32_t self0, uint32_t count, uint32_t other0, uint32_t len, uint32_t last, KeyCodec<K> cd,
	K *__restrict__ outk, uint16_t *__restrict__ src)
{
	const K *const other = codes + other0;
	for (uint32_t e0 = threadIdx.x; e0 < count; e0 += kMergeTh * kMergePer) {
		K x[kMergePer];
		uint32_t base[kMergePer];
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) {
			const uint32_t e = e0 + (uint32_t)v * kMergeTh;
			x[v] = codes[self0 + (e < count ? e : count - 1)]; // (a lane beyond the end ranks the last element again and places nothing)
			base[v] = 0;
		}
		if (len) { // (uniform)
			uint32_t l = len; // invariant: the count lies in [base, base + l], base + l <= len
			while (l > 1) {
				const uint32_t half = l >> 1;
				K k[kMergePer];
#pragma unroll
				for (int v = 0; v < kMergePer; ++v) k[v] = other[base[v] + half - 1]; // (all reads of the step first)
#pragma unroll
				for (int v = 0; v < kMergePer; ++v) base[v] += search_counts(k[v], x[v], RIGHT) ? half : 0u;
				l -= half;
			}
#pragma unroll
			for (int v = 0; v < kMergePer; ++v) base[v] += search_counts(other[base[v]], x[v], RIGHT) ? 1u : 0u; // (base < len)
		}
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) {
			const uint32_t e = e0 + (uint32_t)v * kMergeTh;
			if (e < count) {
				const uint32_t r = e + base[v] < last ? e + base[v] : last;
				outk[r] = cd.dec(x[v]);
				if constexpr (SRC) src[r] = (uint16_t)(self0 + e); // (< TILE <= 4096)
			}
		}
	}
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
// The clamps: na = the tile's elements of a, at most TILE and 0 if the splits are not ascending; nb = those of b, at most what
// is left of TILE and 0 if b_{i+1} < b_i.  With 0 <= a_i <= n and na <= a_{i+1} - a_i the loads are a[a_i, a_i + na) inside
// [0, n) and vals_a likewise; with 0 <= b_i <= m and nb <= b_{i+1} - b_i they are b[b_i, b_i + nb) inside [0, m).  cnt = the
// positions stored, at most the tile's slice d_{i+1} - d_i, so every store is at d_i + p < d_{i+1} <= n + m.  Every rank is
// clamped to na + nb - 1 before it indexes the LDS, and every staged local index on read, so a position that no element
// was ranked to (inputs that are not ascending) stores whatever the LDS held -- but loads inside the inputs.  For ascending
// inputs the clamps change nothing: na + nb = d_{i+1} - d_i <= TILE and the ranks are a bijection.
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
	const uint64_t i = blockIdx.x, total = n + m;
	const uint64_t d0 = i * TILE < total ? i * TILE : total, d1 = (i + 1) * TILE < total ? (i + 1) * TILE : total;
	const uint64_t a0 = splits[i], a1 = splits[i + 1], b0 = d0 - a0, b1 = d1 - a1;
	const uint32_t na = a1 > a0 ? (uint32_t)(a1 - a0 < TILE ? a1 - a0 : TILE) : 0u;
	const uint32_t nb = b1 > b0 ? (uint32_t)(b1 - b0 < TILE - na ? b1 - b0 : TILE - na) : 0u;
	const uint32_t cnt = na + nb < d1 - d0 ? na + nb : (uint32_t)(d1 - d0);
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

} // namespace msd

// msd_setops.hpp -- set operations on two sorted arrays: msd_set_sorted.
//
// a (n keys) and b (m keys) are ascending by CODE (msd_keycodec.hpp); the result is a SET: the distinct codes that are in
// both (intersection), in either (union), in a and not in b (difference) or in exactly one (symmetric difference), ascending.
// Think of the merged sequence of msd_merge2.hpp -- among equal codes all of a's before all of b's -- in which every value
// is represented by the HEAD of its run: the first a that holds it or, where no a does, the first b.  Four stream-ordered
// steps, no atomics, and no workgroup ever waits for another one:
//   1. merge_split_kernel (msd_merge2.hpp, unchanged): the merge path's cut of the merged sequence into tiles.
//   2. set_count_kernel: one workgroup per tile loads a[a_i, a_{i+1}) and b[b_i, b_{i+1}) as codes into the LDS, DECIDES for
//      every element whether it is kept, and writes the number of kept ones to tile_counts[i].
//   3. runs_scan_pieces_kernel, runs_scan_top_kernel (msd_runs.hpp, unchanged): the tile counts become the tiles' bases and
//      *d_num_out.
//   4. set_write_kernel: stages and decides again, places every kept element's DECODED key and local index at its merged
//      rank in the LDS, compacts the ranks that hold a kept element -- ballots, wave by wave -- and stores the tile's slice
//      out[base, base + kept) clipped to cap, coalesced (merge_store), the origins beside it.
//
// THE DECISION needs nothing but the tile and three elements around it (the halo: a[a_i - 1], b[b_i - 1], b[b_{i+1}], each
// only where it exists):
//   an a is a CANDIDATE iff it is the head of its run in a: its predecessor in a differs (the halo for local element 0);
//   it is MATCHED iff the first b that is not below it equals it.  Every b in front of the tile precedes the a in the merged
//      sequence and is therefore strictly smaller (an equal b would come behind it), so that b sits at
//      b_i + |{ b in tile : b < a }| -- inside the tile, or it is exactly b[b_{i+1}];
//   a b is a CANDIDATE iff it is the head of its run in b (the halo b[b_i - 1] for local element 0);
//   it is MATCHED iff the last a that is not above it equals it.  Every a behind the tile follows the b in the merged sequence
//      and is therefore strictly larger (an equal a would come in front of it), so that a sits at
//      a_i + |{ a in tile : a <= b }| - 1 -- inside the tile, or it is exactly a[a_i - 1].
// The two counts are those of merge_rank.  Kept are: the matched a candidates (intersection), the unmatched a candidates
// (difference), all a candidates and the unmatched b candidates (union), the unmatched candidates of both sides (symmetric
// difference): `keep` is a three-bit run-time mask, one kernel text for the four operations.  A matched b is never kept: the
// a it matches stands for the value, which is why origins name A wherever both sides hold a value.
//
// Every extent is CLAMPED as in merge_tile_kernel: inputs that are not ascending give unspecified values and counts, but
// every load stays inside its input array and every store inside [base_i, min(base_{i+1}, cap)) of its output, where
// base_{tiles} = *d_num_out.
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"
#include "msd_merge2.hpp" // MergeCfg, merge_split_kernel, merge_store
#include "msd_runs.hpp"   // kRunsScanTile: the scan of the tile counts
#include "msd_search.hpp" // search_stage, search_counts

namespace msd {

constexpr uint32_t kSetKeepMatchedA = 1u, kSetKeepUnmatchedA = 2u, kSetKeepUnmatchedB = 4u; // the bits of `keep`
constexpr uint16_t kSetNone = 0xFFFFu; // in place of a local index (< TILE <= 4096): the rank holds no kept element

// `keep` of MSD_SET_INTERSECTION, _UNION, _DIFFERENCE, _SYMMETRIC_DIFFERENCE (0 .. 3)
__host__ __device__ inline uint32_t set_keep_mask(int op)
{
	return op == 0 ? kSetKeepMatchedA : op == 1 ? (kSetKeepMatchedA | kSetKeepUnmatchedA | kSetKeepUnmatchedB) : op == 2 ? kSetKeepUnmatchedA : (kSetKeepUnmatchedA | kSetKeepUnmatchedB);
}

// Tile i of the merged sequence with the clamps of merge_tile_kernel -- a[a0, a0 + na) inside [0, n), b[b0, b0 + nb) inside
// [0, m), na + nb <= TILE -- and its halo as codes: has_* says whether the element exists (all uniform).
template <typename K> struct SetTile {
	uint64_t a0, b0;
	uint32_t na, nb;
	bool has_a_before, has_b_before, has_b_behind;
	K a_before, b_before, b_behind;
};
template <typename K>
__device__ __forceinline__ SetTile<K> set_tile(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd, const uint64_t *__restrict__ splits)
{
	constexpr uint32_t TILE = MergeCfg<K>::TILE;
	SetTile<K> t;
	const uint64_t i = blockIdx.x, total = n + m;
	const uint64_t d0 = i * TILE < total ? i * TILE : total, d1 = (i + 1) * TILE < total ? (i + 1) * TILE : total;
	const uint64_t a1 = splits[i + 1], b1 = d1 - a1;
	t.a0 = splits[i];
	t.b0 = d0 - t.a0;
	t.na = a1 > t.a0 ? (uint32_t)(a1 - t.a0 < TILE ? a1 - t.a0 : TILE) : 0u;
	t.nb = b1 > t.b0 ? (uint32_t)(b1 - t.b0 < TILE - t.na ? b1 - t.b0 : TILE - t.na) : 0u;
	// (0 <= a0 <= n and 0 <= b0 <= m: merge_split_kernel; b0 + nb <= b1 <= m)
	t.has_a_before = t.a0 > 0 && t.a0 <= n;
	t.has_b_before = t.b0 > 0 && t.b0 <= m;
	t.has_b_behind = t.b0 + t.nb < m;
	t.a_before = t.has_a_before ? cd.enc(a[t.a0 - 1]) : (K)0;
	t.b_before = t.has_b_before ? cd.enc(b[t.b0 - 1]) : (K)0;
	t.b_behind = t.has_b_behind ? cd.enc(b[t.b0 + t.nb]) : (K)0;
	return t;
}

// The `count` codes at codes[self0 ..] are decided against the `len` codes at codes[other0 ..] (both ascending) with
// merge_rank's search: element e counts the others that are < it (BSIDE: <= it); it is a candidate iff its predecessor --
// `before`, where has_before, for e == 0 -- differs, and matched iff the other at that count (BSIDE: in front of that count)
// -- `edge`, where has_edge, if that lies outside the tile -- equals it.  A candidate is kept if keep_matched /
// keep_unmatched says so.  Returns this lane's number of kept elements.  WRITE: the element's rank e + count, clamped to
// `last`, gets its local index self0 + e in src, or kSetNone, and a kept element's decoded key goes to outk there.
// (Every thread of the workgroup calls it.)
template <typename K, bool BSIDE, bool WRITE>
__device__ __forceinline__ uint32_t set_decide(const K *__restrict__ codes, uint32_t self0, uint32_t count, uint32_t other0, uint32_t len, bool has_before, K before,
	bool has_edge, K edge, bool keep_matched, bool keep_unmatched, uint32_t last, KeyCodec<K> cd, K *__restrict__ outk, uint16_t *__restrict__ src)
{
	const K *const other = codes + other0;
	uint32_t kept = 0;
	for (uint32_t e0 = threadIdx.x; e0 < count; e0 += kMergeTh * kMergePer) {
		K x[kMergePer];
		uint32_t base[kMergePer];
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) {
			const uint32_t e = e0 + (uint32_t)v * kMergeTh;
			x[v] = codes[self0 + (e < count ? e : count - 1)]; // (a lane beyond the end decides the last element again and keeps nothing)
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
				for (int v = 0; v < kMergePer; ++v) base[v] += search_counts(k[v], x[v], BSIDE) ? half : 0u;
				l -= half;
			}
#pragma unroll
			for (int v = 0; v < kMergePer; ++v) base[v] += search_counts(other[base[v]], x[v], BSIDE) ? 1u : 0u; // (base < len)
		}
#pragma unroll
		for (int v = 0; v < kMergePer; ++v) {
			const uint32_t e = e0 + (uint32_t)v * kMergeTh;
			if (e < count) {
				const K prev = codes[self0 + (e ? e - 1 : 0u)];
				const bool head = e ? prev != x[v] : !(has_before && before == x[v]);
				const bool in_tile = BSIDE ? base[v] > 0 : base[v] < len;
				const K y = codes[in_tile ? other0 + (BSIDE ? base[v] - 1 : base[v]) : 0u]; // (count > 0: codes[0] is staged)
				const bool matched = in_tile ? y == x[v] : (has_edge && edge == x[v]);
				const bool keep = head && (matched ? keep_matched : keep_unmatched);
				kept += keep ? 1u : 0u;
				if constexpr (WRITE) {
					const uint32_t r = e + base[v] < last ? e + base[v] : last;
					src[r] = keep ? (uint16_t)(self0 + e) : kSetNone; // (< TILE <= 4096)
					if (keep) outk[r] = cd.dec(x[v]);
				}
			}
		}
	}
	return kept;
}

// both sides of a staged tile: this lane's number of kept elements
template <typename K, bool WRITE>
__device__ __forceinline__ uint32_t set_decide_tile(const K *__restrict__ codes, const SetTile<K> &t, uint32_t keep, KeyCodec<K> cd, K *__restrict__ outk,
	uint16_t *__restrict__ src)
{
	const uint32_t last = t.na + t.nb - 1;
	// a: the b that are smaller; the first b that is not smaller is codes[na + count], or b[b0 + nb]
	uint32_t kept = set_decide<K, false, WRITE>(codes, 0, t.na, t.na, t.nb, t.has_a_before, t.a_before, t.has_b_behind, t.b_behind, (keep & kSetKeepMatchedA) != 0,
		(keep & kSetKeepUnmatchedA) != 0, last, cd, outk, src);
	// b: the a that are not larger; the last of them is codes[count - 1], or a[a0 - 1]
	kept += set_decide<K, true, WRITE>(codes, t.na, t.nb, 0, t.na, t.has_b_before, t.b_before, t.has_a_before, t.a_before, false, (keep & kSetKeepUnmatchedB) != 0, last,
		cd, outk, src);
	return kept;
}

// ---- step 2
template <typename K>
__global__ __launch_bounds__(kMergeTh) void set_count_kernel(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd, uint32_t keep,
	const uint64_t *__restrict__ splits, uint64_t *__restrict__ tile_counts)
{
	constexpr uint32_t TILE = MergeCfg<K>::TILE;
	__shared__ K codes[TILE]; // the tile's a as codes, the tile's b as codes behind them
	__shared__ uint32_t tmp[8];
	const SetTile<K> t = set_tile<K>(a, n, b, m, cd, splits);
	if (t.na + t.nb == 0) { // (uniform: the barriers below are never reached by a part of the workgroup)
		if (threadIdx.x == 0) tile_counts[blockIdx.x] = 0;
		return;
	}
	search_stage<K>(a + t.a0, t.na, cd, codes);
	search_stage<K>(b + t.b0, t.nb, cd, codes + t.na);
	__syncthreads();
	const uint32_t kept = set_decide_tile<K, false>(codes, t, keep, cd, nullptr, nullptr);
	uint32_t total;
	block_excl_scan256(kept, tmp, total);
	if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// n + m == 0: the empty set
__global__ __launch_bounds__(64) void set_empty_kernel(uint64_t *__restrict__ num_out)
{
	if (threadIdx.x == 0) *num_out = 0;
}

// ---- step 4
// The tile's results go to [base, lim) with base = tile_base[i] + piece_base[i / kRunsScanTile] (the scanned counts),
// lim = min(the next tile's base -- *num_out for the last tile --, cap): at most the number step 2 counted and at most
// na + nb <= TILE, whatever this kernel decides.  A tile with nothing to store leaves before it loads anything.
// The compaction: wave w owns the ranks [w * TILE / 4, (w + 1) * TILE / 4), 64 at a time; the ranks that hold a kept element
// are one ballot, the kept ones in front of a rank are popcounts -- of the ballots of the ranks in front of the wave's, which
// the wave forms itself (no word of LDS beyond the three arrays: 40 KiB for 4-byte keys, four workgroups per CU), of the
// wave's own earlier ballots, and of the lower lanes' bits.  The keys go from outk to `codes`, which is dead behind the
// decision; the local indices are compacted in place, all of them read before the barrier and written behind it.
template <typename K>
__global__ __launch_bounds__(kMergeTh) void set_write_kernel(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd, uint32_t keep,
	const uint64_t *__restrict__ splits, const uint64_t *__restrict__ tile_base, const uint64_t *__restrict__ piece_base, const uint64_t *__restrict__ num_out,
	uint64_t cap, K *__restrict__ out, uint64_t *__restrict__ out_origin)
{
	constexpr uint32_t TILE = MergeCfg<K>::TILE;
	constexpr uint32_t PER = TILE / 64u / (kMergeTh / 64u); // ballots of one wave: 16 (4-byte), 8 (8-byte)
	__shared__ K codes[TILE];      // the tile's a as codes, the tile's b as codes behind them; then the kept keys, compacted
	__shared__ K outk[TILE];       // the kept keys, decoded, at their merged ranks
	__shared__ uint16_t src[TILE]; // per rank the local index of its element (< na from a, else from b) or kSetNone; then compacted
	const uint64_t i = blockIdx.x;
	const uint64_t base = tile_base[i] + piece_base[i / kRunsScanTile];
	const uint64_t next = i + 1 < gridDim.x ? tile_base[i + 1] + piece_base[(i + 1) / kRunsScanTile] : *num_out;
	const uint64_t lim = next < cap ? next : cap;
	if (base >= lim) return; // (uniform: the barriers below are never reached by a part of the workgroup)
	const SetTile<K> t = set_tile<K>(a, n, b, m, cd, splits);
	const uint32_t ranks = t.na + t.nb;
	if (ranks == 0) return; // (uniform)
	const uint32_t cnt = lim - base < ranks ? (uint32_t)(lim - base) : ranks;
	const uint32_t last = ranks - 1;
	search_stage<K>(a + t.a0, t.na, cd, codes);
	search_stage<K>(b + t.b0, t.nb, cd, codes + t.na);
	__syncthreads();
	set_decide_tile<K, true>(codes, t, keep, cd, outk, src);
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63u, first = (threadIdx.x >> 6) * PER; // the wave's first ballot
	uint32_t before = 0; // kept elements in front of the ballot at hand (uniform)
	for (uint32_t c = 0; c < first; ++c) {
		const uint32_t r = c * 64u + lane;
		before += (uint32_t)__popcll(__ballot(r < ranks && src[r] != kSetNone));
	}
	uint16_t s[PER];
	uint64_t bits[PER];
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k) {
		const uint32_t r = (first + k) * 64u + lane;
		s[k] = r < ranks ? src[r] : kSetNone;
		bits[k] = __ballot(s[k] != kSetNone);
	}
	__syncthreads(); // (src is read, codes is dead)
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k) {
		const uint32_t r = (first + k) * 64u + lane, to = before + popc_below_lane(bits[k]);
		if (s[k] != kSetNone && to < cnt) {
			codes[to] = outk[r];
			src[to] = s[k];
		}
		before += (uint32_t)__popcll(bits[k]);
	}
	__syncthreads();
	if (out) merge_store<K>(codes, cnt, out + base);
	if (out_origin) {
		for (uint32_t p = threadIdx.x; p < cnt; p += kMergeTh) {
			const uint32_t e = src[p] < last ? src[p] : last;
			const bool from_a = e < t.na;
			const uint64_t at = from_a ? t.a0 + e : t.b0 + (e - t.na); // (< n, < m)
			out_origin[base + p] = from_a ? at : n + at;
		}
	}
}

} // namespace msd

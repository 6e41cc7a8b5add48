// msd_setops.hpp -- set operations on two sorted arrays: msd_set_sorted.
//
// a (n keys) and b (m keys) are ascending by CODE (msd_keycodec.hpp); the result is a SET: the distinct codes that are in
// both (intersection), in either (union), in a and not in b (difference) or in exactly one (symmetric difference), ascending.
// Think of the merged sequence of msd_merge2.hpp -- among equal codes all of a's before all of b's -- in which every value
// is represented by the HEAD of its run: the first a that holds it or, where no a does, the first b.  Four stream-ordered
// steps, no atomics, and no workgroup ever waits for another one:
//   1. search_split_kernel (msd_search.hpp) with the RIGHT rule: the merge path's cut of the merged sequence into tiles.
//   2. set_count_kernel: one workgroup per tile loads a[a_i, a_{i+1}) and b[b_i, b_{i+1}) as codes into the LDS, DECIDES for
//      every element whether it is kept, and writes the number of kept ones to tile_counts[i].
//   3. runs_scan_pieces_kernel, runs_scan_top_kernel (msd_runs.hpp): the tile counts become the tiles' bases and
//      *d_num_out.
//   4. set_write_kernel: stages and decides again, places every kept element's DECODED key and local index at its merged
//      rank in the LDS, compacts the ranks that hold a kept element (ballot_compact of msd_merge2.hpp) and stores the tile's slice
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
// The two counts are those of merge_rank (merge_for_counts).  Kept are: the matched a candidates (intersection), the unmatched a candidates
// (difference), all a candidates and the unmatched b candidates (union), the unmatched candidates of both sides (symmetric
// difference): `keep` is a three-bit run-time mask, one kernel text for the four operations.  A matched b is never kept: the
// a it matches stands for the value, which is why origins name A wherever both sides hold a value.
//
// Every extent is CLAMPED (merge_tile_extent): inputs that are not ascending give unspecified values and counts, but
// every load stays inside its input array and every store inside [base_i, min(base_{i+1}, cap)) of its output, where
// base_{tiles} = *d_num_out.
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"
#include "msd_merge2.hpp" // MergeCfg, merge_for_counts, merge_store, tile_out_window, ballot_compact, kSetNone
#include "msd_search.hpp" // merge_tile_extent, search_stage

namespace msd {

constexpr uint32_t kSetKeepMatchedA = 1u, kSetKeepUnmatchedA = 2u, kSetKeepUnmatchedB = 4u; // the bits of `keep`

// `keep` of MSD_SET_INTERSECTION, _UNION, _DIFFERENCE, _SYMMETRIC_DIFFERENCE (0 .. 3)
__host__ __device__ inline uint32_t set_keep_mask(int op)
{
	return op == 0 ? kSetKeepMatchedA : op == 1 ? (kSetKeepMatchedA | kSetKeepUnmatchedA | kSetKeepUnmatchedB) : op == 2 ? kSetKeepUnmatchedA : (kSetKeepUnmatchedA | kSetKeepUnmatchedB);
}

// Tile i of the merged sequence (merge_tile_extent: a[a0, a0 + na) inside [0, n), b[b0, b0 + nb) inside [0, m),
// na + nb <= TILE) and its halo as codes: has_* says whether the element exists (all uniform).
template <typename K> struct SetTile {
	uint64_t a0, b0;
	uint32_t na, nb;
	bool has_a_before, has_b_before, has_b_behind;
	K a_before, b_before, b_behind;
};
template <typename K>
__device__ __forceinline__ SetTile<K> set_tile(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd, const uint64_t *__restrict__ splits)
{
	const MergeTileExtent x = merge_tile_extent<MergeCfg<K>::TILE>(blockIdx.x, n, m, splits);
	SetTile<K> t;
	t.a0 = x.a0;
	t.b0 = x.b0;
	t.na = x.na;
	t.nb = x.nb;
	// (0 <= a0 <= n and 0 <= b0 <= m: the split kernel; b0 + nb <= b1 <= m)
	t.has_a_before = t.a0 > 0 && t.a0 <= n;
	t.has_b_before = t.b0 > 0 && t.b0 <= m;
	t.has_b_behind = t.b0 + t.nb < m;
	t.a_before = t.has_a_before ? cd.enc(a[t.a0 - 1]) : (K)0;
	t.b_before = t.has_b_before ? cd.enc(b[t.b0 - 1]) : (K)0;
	t.b_behind = t.has_b_behind ? cd.enc(b[t.b0 + t.nb]) : (K)0;
	return t;
}

// The `count` codes at codes[self0 ..] are decided against the `len` codes at codes[other0 ..] (both ascending) with
// merge_for_counts: element e counts the others that are < it (BSIDE: <= it); it is a candidate iff its predecessor --
// `before`, where has_before, for e == 0 -- differs, and matched iff the other at that count (BSIDE: in front of that count)
// -- `edge`, where has_edge, if that lies outside the tile -- equals it.  A candidate is kept if keep_matched /
// keep_unmatched says so.  Returns this lane's number of kept elements; store(e, x, count, keep) for every element is what
// the caller does with the decision.  (Every thread of the workgroup calls it.)
template <typename K, bool BSIDE, typename F>
__device__ __forceinline__ uint32_t set_decide(const K *__restrict__ codes, uint32_t self0, uint32_t count, uint32_t other0, uint32_t len, bool has_before, K before,
	bool has_edge, K edge, bool keep_matched, bool keep_unmatched, F &&store)
{
	uint32_t kept = 0;
	merge_for_counts<K, BSIDE>(codes, self0, count, other0, len, [&](uint32_t e, K x, uint32_t base) {
		const K prev = codes[self0 + (e ? e - 1 : 0u)];
		const bool head = e ? prev != x : !(has_before && before == x);
		const bool in_tile = BSIDE ? base > 0 : base < len;
		const K y = codes[in_tile ? other0 + (BSIDE ? base - 1 : base) : 0u]; // (count > 0: codes[0] is staged)
		const bool matched = in_tile ? y == x : (has_edge && edge == x);
		const bool keep = head && (matched ? keep_matched : keep_unmatched);
		kept += keep ? 1u : 0u;
		store(e, x, base, keep);
	});
	return kept;
}
// the A side of a staged tile: the b that are smaller; the first b that is not smaller is codes[na + count], or b[b0 + nb]
template <typename K, typename F>
__device__ __forceinline__ uint32_t set_decide_a(const K *__restrict__ codes, const SetTile<K> &t, bool keep_matched, bool keep_unmatched, F &&store)
{
	return set_decide<K, false>(codes, 0, t.na, t.na, t.nb, t.has_a_before, t.a_before, t.has_b_behind, t.b_behind, keep_matched, keep_unmatched, store);
}

// Both sides of a staged tile: this lane's number of kept elements.  WRITE: the element's rank e + count, clamped to the
// tile's last, gets its local index in src, or kSetNone, and a kept element's decoded key goes to outk there.
template <typename K, bool WRITE>
__device__ __forceinline__ uint32_t set_decide_tile(const K *__restrict__ codes, const SetTile<K> &t, uint32_t keep, KeyCodec<K> cd, K *__restrict__ outk,
	uint16_t *__restrict__ src)
{
	const uint32_t last = t.na + t.nb - 1;
	uint32_t self0 = 0;
	const auto store = [&](uint32_t e, K x, uint32_t base, bool kept) {
		if constexpr (WRITE) {
			const uint32_t r = e + base < last ? e + base : last;
			src[r] = kept ? (uint16_t)(self0 + e) : kSetNone; // (< TILE <= 4096)
			if (kept) outk[r] = cd.dec(x);
		}
	};
	uint32_t kept = set_decide_a<K>(codes, t, (keep & kSetKeepMatchedA) != 0, (keep & kSetKeepUnmatchedA) != 0, store);
	// b: the a that are not larger; the last of them is codes[count - 1], or a[a0 - 1]
	self0 = t.na;
	kept += set_decide<K, true>(codes, t.na, t.nb, 0, t.na, t.has_b_before, t.b_before, t.has_a_before, t.a_before, false, (keep & kSetKeepUnmatchedB) != 0, store);
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

// ---- step 4
// The tile's results go to its window [base, lim) of the scanned counts (tile_out_window of msd_merge2.hpp): at most the
// number step 2 counted and at most na + nb <= TILE, whatever this kernel decides.  A tile with nothing to store leaves
// before it loads anything.  The ranks that hold a kept element are compacted by ballot_compact (no word of LDS beyond the
// three arrays: 40 KiB for 4-byte keys, four workgroups per CU): the keys go from outk to `codes`, which is dead behind the
// decision; the local indices are compacted in place.
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
	const TileOutWindow win = tile_out_window(tile_base, piece_base, num_out, cap);
	const uint64_t base = win.base, lim = win.lim;
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
	ballot_compact<PER, true>(src, ranks, cnt, [&](uint32_t r, uint32_t to, uint16_t e) { // (behind its barrier src is read and codes is dead)
		codes[to] = outk[r];
		src[to] = e;
	});
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

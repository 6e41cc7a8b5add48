// msd_join.hpp -- sort-merge join of two sorted arrays: msd_join_groups, msd_join_pairs.
//
// a (n keys) and b (m keys) are ascending by CODE (msd_keycodec.hpp).  The join is every pair (i, j) with code(a[i]) ==
// code(b[j]); it comes in two calls with the MATCHED GROUPS between them: for every value that both sides hold, ascending,
// the key, the first index and the length of its run in a, and the same for b.  The groups are the join in CSR form.
//
// ---- msd_join_groups: the steps of msd_setops.hpp, no atomics, and no workgroup ever waits for another one:
//   1. search_split_kernel (msd_search.hpp) with the RIGHT rule: the merge path's cut of the merged sequence into tiles.
//   2. set_count_kernel (msd_setops.hpp) with the mask of the intersection: the kept elements of a tile are the
//      matched heads of a -- one per group, at the tile that holds the first a of the group.
//   3. runs_scan_pieces_kernel, runs_scan_top_kernel (msd_runs.hpp): the tiles' bases and *d_num_groups.
//   4. join_write_kernel: stages the tile, decides again (set_decide_a: head and matched), compacts the kept heads in the
//      order of their local index (ballot_compact of msd_merge2.hpp) and works out, for the kept heads only, the four
//      numbers of the group.
//
// For a kept head with code v at local index e:  a_first = a_i + e, and b_first = b_i + |{ b in tile : b < v }|, which is
// exact by the argument of msd_setops.hpp: every b in front of the tile is strictly smaller than v.
//
// THE RUN ENDS.  With ua = |{ a in tile : a <= v }| and ub = |{ b in tile : b <= v }| (two LDS searches per kept head):
//   if ua < na the tile holds a larger a and the run of v in a ends at a_i + ua; likewise ub < nb for b.  Otherwise the tile
//   holds no larger element of that side, and the run ends at the tile's end unless the element behind the tile -- the halo
//   a[a_{i+1}] or b[b_{i+1}] -- equals v too: the run STRADDLES, and one lane finds its end by an upper-bound binary search
//   in a[a_{i+1}, n) or b[b_{i+1}, m).
// At most ONE value per tile and side can straddle.  On the A side it is the tile's largest a (ua == na holds for no other
// value).  On the B side: if two matched values v1 < v2 have their heads in the tile, then b[lb(v2)], the first b that is not
// below v2, equals v2 and lies in the tile or is the halo b[b_{i+1}]; either way a b larger than v1 sits at or in front of
// b_{i+1}, so v1's run ends inside the tile (ub(v1) < nb) or exactly at its end with the halo differing from v1.  Only the
// largest matched value of the tile can have ub == nb with the halo equal to it.  So a tile does at most two global
// searches, and only where a matched run really leaves it; the halo is the three elements of msd_setops.hpp plus a[a_{i+1}].
//
// Every extent is CLAMPED as in set_write_kernel: inputs that are not ascending give unspecified values and counts, but every
// load stays inside its input array and every store inside [base_i, min(base_{i+1}, cap)), where base_{tiles} = *d_num_groups.
//
// ---- msd_join_pairs: the groups' sizes p x q become the pairs, in three steps:
//   1. join_offsets_kernel: the products p * q of the G = min(*d_num_groups, groups_cap) groups, scanned piece by piece as
//      runs_scan_pieces_kernel scans tile counts -- the product is formed where that kernel loads a word, so no array of
//      products is written and read again -- into exclusive offsets, 8 bytes per group, and one sum per piece.  A piece
//      behind the last group writes its sum of 0 and nothing else: groups_cap may be far above G at no cost in traffic.
//   2. runs_scan_top_kernel (msd_runs.hpp): the pieces' bases and *d_num_pairs.  off[g] = the group's word plus
//      its piece's base, for g < G; behind the last group off is the total.
//   3. join_expand_kernel, OUTPUT-partitioned: workgroup j owns the ranks [j * PAIR_TILE, min((j + 1) * PAIR_TILE, total,
//      cap)) and leaves before it loads anything else if that is empty.  Every group holds at least one pair, so the range
//      overlaps at most PAIR_TILE groups: one search over off finds the first one, the starts of the next ones go to
//      the LDS relative to the range and clipped to it, and every lane takes kJoinPairPer CONSECUTIVE ranks: one LDS search
//      and one division t / q for its first rank, increments for the rest (a 32-bit division where t and q allow it).  The
//      index pairs go through the LDS and are stored coalesced, through pos_a / pos_b where given -- then one lane's
//      neighbours load neighbouring words of pos_b.
// One group of 2^30 x 2^30 pairs and a million groups of one pair are the same work per workgroup: no atomics, no worklist.
// The clamps: a rank is stored at [0, min(total, cap)) only; every group index stays below G <= groups_cap; ia < n and ib < m
// before a position is loaded; a q of 0 (groups this library did not make) divides as 1.
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"
#include "msd_merge2.hpp" // MergeCfg, tile_out_window, ballot_compact, kSetNone
#include "msd_runs.hpp"   // runs_scan_piece, tile_out_base: the scan of the products
#include "msd_search.hpp" // search_stage, lds_count
#include "msd_setops.hpp" // set_tile, set_decide_a, set_count_kernel

namespace msd {

// Fewer than 2^32 elements per side: every product a_count * b_count and the number of pairs (at most n * m) fit 64 bits, and
// an index into a or b fits the 32-bit words the expansion stages.  Fewer than 2^40 pairs are stored by one call (its grid).
constexpr uint64_t kJoinMaxElems = (uint64_t)1 << 32, kJoinMaxStored = (uint64_t)1 << 40;

// |{ k in keys[lo, hi) : code(k) <= v }| + lo: where the run of v ends behind lo (lo <= hi <= the array's length; one lane)
template <typename K> __host__ __device__ __forceinline__ uint64_t join_global_upper(const K *__restrict__ keys, uint64_t lo, uint64_t hi, K v, KeyCodec<K> cd)
{
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if (cd.enc(keys[mid]) <= v) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// ---- msd_join_groups, step 4
// The groups go to the tile's window [base, lim) (tile_out_window).  LDS: the codes (16 KiB), per local a its b count or kSetNone, and the
// compacted local indices and b counts (3 x TILE x 2 bytes): 40 KiB for 4-byte keys, 28 KiB for 8-byte keys.
template <typename K>
__global__ __launch_bounds__(kMergeTh) void join_write_kernel(const K *__restrict__ a, uint64_t n, const K *__restrict__ b, uint64_t m, KeyCodec<K> cd,
	const uint64_t *__restrict__ splits, const uint64_t *__restrict__ tile_base, const uint64_t *__restrict__ piece_base, const uint64_t *__restrict__ num_groups,
	uint64_t cap, K *__restrict__ out_keys, uint64_t *__restrict__ a_first, uint64_t *__restrict__ a_count, uint64_t *__restrict__ b_first, uint64_t *__restrict__ b_count)
{
	constexpr uint32_t TILE = MergeCfg<K>::TILE;
	constexpr uint32_t PER = TILE / 64u / (kMergeTh / 64u); // ballots of one wave: 16 (4-byte), 8 (8-byte)
	__shared__ K codes[TILE];         // the tile's a as codes, the tile's b as codes behind them
	__shared__ uint16_t below[TILE];  // per local a: |{ b in tile : b < a }| if it is a matched head, else kSetNone
	__shared__ uint16_t kept_e[TILE]; // the kept heads' local indices, compacted
	__shared__ uint16_t kept_lb[TILE]; // ... and their b counts
	const TileOutWindow win = tile_out_window(tile_base, piece_base, num_groups, cap);
	const uint64_t base = win.base, lim = win.lim;
	if (base >= lim) return; // (uniform: the barriers below are never reached by a part of the workgroup)
	const SetTile<K> t = set_tile<K>(a, n, b, m, cd, splits);
	if (t.na == 0) return; // (uniform) no a, no head
	const uint32_t cnt = lim - base < t.na ? (uint32_t)(lim - base) : t.na;
	const bool has_a_behind = t.a0 + t.na < n; // the fourth halo element
	const K a_behind = has_a_behind ? cd.enc(a[t.a0 + t.na]) : (K)0;
	search_stage<K>(a + t.a0, t.na, cd, codes);
	search_stage<K>(b + t.b0, t.nb, cd, codes + t.na);
	__syncthreads();
	// the A side's decision with the intersection's mask: a matched head keeps its b count
	set_decide_a<K>(codes, t, true, false, [&](uint32_t e, K, uint32_t lb, bool kept) { below[e] = kept ? (uint16_t)lb : kSetNone; }); // (lb <= nb < TILE <= 4096)
	__syncthreads();
	ballot_compact<PER, false>(below, t.na, cnt, [&](uint32_t e, uint32_t to, uint16_t lb) {
		kept_e[to] = (uint16_t)e;
		kept_lb[to] = lb;
	});
	__syncthreads();
	for (uint32_t p = threadIdx.x; p < cnt; p += kMergeTh) {
		const uint32_t e = kept_e[p] < t.na - 1 ? kept_e[p] : t.na - 1; // (the clamps: positions nothing was compacted to)
		const uint32_t lb = kept_lb[p] < t.nb ? kept_lb[p] : t.nb;
		const K v = codes[e];
		const uint64_t af = t.a0 + e, bf = t.b0 + lb;
		const uint32_t ua = lds_count<K>(codes, t.na, v, true);
		const uint32_t ub = lds_count<K>(codes + t.na, t.nb, v, true);
		uint64_t a_end = t.a0 + (ua > e ? ua : e + 1), b_end = t.b0 + (ub > lb ? ub : lb);
		if (ua >= t.na && has_a_behind && a_behind == v) a_end = join_global_upper<K>(a, t.a0 + t.na, n, v, cd);
		if (ub >= t.nb && t.has_b_behind && t.b_behind == v) b_end = join_global_upper<K>(b, t.b0 + t.nb, m, v, cd);
		if (out_keys) out_keys[base + p] = cd.dec(v);
		if (a_first) a_first[base + p] = af;
		if (a_count) a_count[base + p] = a_end - af;
		if (b_first) b_first[base + p] = bf;
		if (b_count) b_count[base + p] = b_end - bf;
	}
}

// ---- msd_join_pairs
constexpr int kJoinPairTh = 256, kJoinPairPer = 8;
constexpr uint32_t kJoinPairTile = kJoinPairTh * kJoinPairPer; // ranks of one workgroup of the expansion

// step 1: runs_scan_pieces_kernel over the products of the first G groups: runs_scan_piece with the product for its load
__global__ __launch_bounds__(kRunsScanTh) void join_offsets_kernel(uint64_t groups_cap, const uint64_t *__restrict__ num_groups, const uint64_t *__restrict__ a_count,
	const uint64_t *__restrict__ b_count, uint64_t *__restrict__ off_word, uint64_t *__restrict__ piece_sums)
{
	__shared__ uint64_t tmp[4];
	const uint64_t G = *num_groups < groups_cap ? *num_groups : groups_cap;
	const uint64_t first = (uint64_t)blockIdx.x * kRunsScanTile;
	if (first >= G) { // (uniform) a piece behind the last group
		if (threadIdx.x == 0) piece_sums[blockIdx.x] = 0;
		return;
	}
	const uint32_t count = G - first < kRunsScanTile ? (uint32_t)(G - first) : kRunsScanTile;
	const uint64_t total = runs_scan_piece(off_word + first, count, 0, tmp, [&](uint32_t idx) { return a_count[first + idx] * b_count[first + idx]; });
	if (threadIdx.x == 0) piece_sums[blockIdx.x] = total;
}

// step 3
template <bool POSA, bool POSB>
__global__ __launch_bounds__(kJoinPairTh) void join_expand_kernel(uint64_t groups_cap, const uint64_t *__restrict__ num_groups, const uint64_t *__restrict__ off_word,
	const uint64_t *__restrict__ off_piece, const uint64_t *__restrict__ num_pairs, const uint64_t *__restrict__ a_first, const uint64_t *__restrict__ b_first, const uint64_t *__restrict__ b_count, uint64_t n,
	uint64_t m, const uint64_t *__restrict__ pos_a, const uint64_t *__restrict__ pos_b, uint64_t cap, uint64_t *__restrict__ out_a, uint64_t *__restrict__ out_b)
{
	constexpr uint32_t PT = kJoinPairTile;
	__shared__ uint32_t rel[PT];  // rel[k], k >= 1: where group g0 + k starts, relative to the range and clipped to it
	__shared__ uint32_t sa[PT];   // the ranks' indices into a and b (< 2^32)
	__shared__ uint32_t sb[PT];
	const uint64_t total = *num_pairs;
	const uint64_t stop = total < cap ? total : cap;
	const uint64_t r0 = (uint64_t)blockIdx.x * PT;
	if (r0 >= stop) return; // (uniform: nothing else is loaded, and the barriers below are never reached by a part of the workgroup)
	const uint32_t cnt = stop - r0 < PT ? (uint32_t)(stop - r0) : PT;
	const uint64_t G = *num_groups < groups_cap ? *num_groups : groups_cap;
	if (G == 0) return; // (uniform; never with total > 0)
	auto off = [&](uint64_t g) { return tile_out_base(off_word, off_piece, g); }; // (g < G)
	// The first group: the last g < G with off[g] <= r0 (off[0] = 0).  A 64-ary search,
	// every wave for itself: the lanes probe 64 points of [lo, hi) at once and a ballot counts those that are not beyond r0,
	// five steps for 2^28 groups where a binary search has 28 dependent loads.  [lo, hi) only ever shrinks, whatever off holds.
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t lo = 0, hi = G; // invariant: off[g] <= r0 for g < lo, off[g] > r0 for g >= hi
	while (lo < hi) {
		const uint64_t step = (hi - lo + 63) >> 6;
		const uint64_t at = lo + (lane + 1) * step - 1;
		const uint32_t c = (uint32_t)__popcll(__ballot(at < hi && off(at) <= r0));
		const uint64_t stop_at = lo + (c + 1) * step - 1; // the first probe beyond r0, if there is one
		lo += c * step;
		hi = stop_at < hi ? stop_at : hi;
	}
	const uint64_t g0 = lo ? lo - 1 : 0;
	// (a lane whose last group starts behind the range loads no more: the starts are ascending)
	uint64_t o = 0;
	for (uint32_t k = threadIdx.x; k < PT; k += kJoinPairTh) {
		const uint64_t g = g0 + k;
		if (o < r0 + cnt) o = g < G ? off(g) : total;
		rel[k] = o > r0 ? (o - r0 < cnt ? (uint32_t)(o - r0) : cnt) : 0u;
	}
	__syncthreads();
	const uint32_t x0 = threadIdx.x * kJoinPairPer;
	if (x0 < cnt) {
		// this lane's first group: the number of k in [1, PT) with rel[k] <= x0
		uint32_t k = lds_count<uint32_t>(rel + 1, PT - 1, x0, true);
		uint64_t g = g0 + k < G ? g0 + k : G - 1;
		uint64_t q = b_count[g] ? b_count[g] : 1;
		const uint64_t t0 = r0 + x0 - off(g);
		uint64_t row, col;
		if (((t0 | q) >> 32) == 0) {
			row = (uint32_t)t0 / (uint32_t)q;
			col = (uint32_t)t0 % (uint32_t)q;
		} else {
			row = t0 / q;
			col = t0 % q;
		}
		uint64_t ia = a_first[g] + row, ib0 = b_first[g];
		uint32_t nxt = k + 1 < PT ? rel[k + 1] : cnt; // where the next group starts
#pragma unroll
		for (uint32_t j = 0; j < (uint32_t)kJoinPairPer; ++j) {
			const uint32_t x = x0 + j;
			if (x < cnt) {
				if (x >= nxt && k + 1 < PT) { // the next group starts here (every group holds a pair)
					++k;
					nxt = k + 1 < PT ? rel[k + 1] : cnt;
					g = g0 + k < G ? g0 + k : G - 1;
					q = b_count[g] ? b_count[g] : 1;
					ia = a_first[g];
					ib0 = b_first[g];
					col = 0;
				}
				sa[x] = (uint32_t)ia;
				sb[x] = (uint32_t)(ib0 + col);
				if (++col >= q) {
					col = 0;
					++ia;
				}
			}
		}
	}
	__syncthreads();
	for (uint32_t p = threadIdx.x; p < cnt; p += kJoinPairTh) {
		uint64_t ia = sa[p], ib = sb[p];
		if (out_a) {
			if constexpr (POSA) ia = pos_a[ia < n ? ia : n - 1];
			out_a[r0 + p] = ia;
		}
		if (out_b) {
			if constexpr (POSB) ib = pos_b[ib < m ? ib : m - 1];
			out_b[r0 + p] = ib;
		}
	}
}

} // namespace msd

// msd_reduce.hpp -- reduce-by-key over runs: msd_reduce_runs.
//
// The runs are those of msd_runs.hpp (same tiles, same head ballots, same count and scan kernels); this file adds one
// number per run: the sum, the minimum or the maximum of a value column.  No workgroup waits for another one and there
// are no atomics: stream order is the only barrier between the steps, and the order every result is evaluated in is
// fixed by the tile geometry alone.
//   1. runs_count_kernel, runs_scan_pieces_kernel, runs_scan_top_kernel: the tiles' bases and the number of runs.
//   2. reduce_tile_kernel: reads the tile's keys again and its values once (directly or through the positions), and
//      reduces them by a SEGMENTED SUFFIX scan over the head ballots: s(i) = the reduction of elements i .. the element in
//      front of the next head (or the tile's end).  At a head that is the run's part inside the tile; it is compacted in
//      the LDS at its run number within the tile and stored to d_out in run order.  The tile's RECORD is its number of
//      heads and its LEAD: the reduction of the elements in front of its first head -- of the whole tile if it has none.
//   3. The last run that starts in tile t still lacks S(t) = the leads of tiles t+1, t+2, ... up to and including the
//      first one that has a head: an exclusive segmented suffix scan over the records, in the two-level shape of step 1
//      (seg_carry_pieces_kernel<R, false>: one workgroup per kRunsScanTile records, in place; seg_carry_top_kernel<R,
//      false>: one workgroup over the piece summaries; msd_scan.hpp runs the same two with FWD true).
//      reduce_apply_kernel, one thread per tile, combines S(t) into d_out[base(t) + heads(t) - 1].  A tile adds its lead
//      to the run that is open on its LEFT, so the carry flows from right to left.
//
// A segment pair is (f, v): v = the reduction of the elements in front of the first head of a stretch (of all of them if
// it has none), f = whether it has a head.  combine(L, R) = (L.f | R.f, L.f ? L.v : op(L.v, R.v)) is associative; every
// level below is a suffix scan under it: the e of a lane, the lanes of a k, the k of a wave, the waves of a workgroup.
#pragma once

#include "msd_runs.hpp"
#include "msd_keycodec.hpp"

namespace msd {

// ---- what is reduced: A the accumulator, O the element of d_out, W the unsigned word of O's width (the codec's type)
struct RedAddU64 {
	typedef uint64_t A;
	typedef uint64_t O;
	static __device__ __forceinline__ A id(KeyCodec<O>) { return 0; }
	static __device__ __forceinline__ A op(A a, A b) { return a + b; }
	static __device__ __forceinline__ uint64_t bits(A a) { return a; }
	static __device__ __forceinline__ A from_bits(uint64_t b) { return b; }
	static __device__ __forceinline__ O out(A a, KeyCodec<O>) { return a; }
	static __device__ __forceinline__ A in(O o, KeyCodec<O>) { return o; }
};
struct RedAddF64 {
	typedef double A;
	typedef uint64_t O;
	static __device__ __forceinline__ A id(KeyCodec<O>) { return 0.0; }
	static __device__ __forceinline__ A op(A a, A b) { return a + b; }
	static __device__ __forceinline__ uint64_t bits(A a) { return (uint64_t)__double_as_longlong(a); }
	static __device__ __forceinline__ A from_bits(uint64_t b) { return __longlong_as_double((long long)b); }
	static __device__ __forceinline__ O out(A a, KeyCodec<O>) { return bits(a); }
	static __device__ __forceinline__ A in(O o, KeyCodec<O>) { return from_bits(o); }
};
// Minimum of the codes under the codec the kernel is handed; a maximum is the minimum under the codec flipped by all
// ones (code' = ~code), so there is one instance per width.  The identity is the largest code.
template <typename W> struct RedMinCode {
	typedef W A;
	typedef W O;
	static __device__ __forceinline__ A id(KeyCodec<W>) { return (W)~(W)0; }
	static __device__ __forceinline__ A op(A a, A b) { return a < b ? a : b; }
	static __device__ __forceinline__ uint64_t bits(A a) { return (uint64_t)a; }
	static __device__ __forceinline__ A from_bits(uint64_t b) { return (W)b; }
	static __device__ __forceinline__ O out(A a, KeyCodec<W> cd) { return cd.dec(a); }
	static __device__ __forceinline__ A in(O o, KeyCodec<W> cd) { return cd.enc(o); }
};

// ---- how a value becomes an accumulator: R the reduction, V the unsigned word that carries the value
struct SumU32 { typedef RedAddU64 R; typedef uint32_t V; static __device__ __forceinline__ uint64_t conv(V v, KeyCodec<uint64_t>) { return v; } };
struct SumI32 { typedef RedAddU64 R; typedef uint32_t V; static __device__ __forceinline__ uint64_t conv(V v, KeyCodec<uint64_t>) { return (uint64_t)(int64_t)(int32_t)v; } };
struct SumX64 { typedef RedAddU64 R; typedef uint64_t V; static __device__ __forceinline__ uint64_t conv(V v, KeyCodec<uint64_t>) { return v; } };
struct SumF32 { typedef RedAddF64 R; typedef uint32_t V; static __device__ __forceinline__ double conv(V v, KeyCodec<uint64_t>) { return (double)__uint_as_float(v); } };
struct SumF64 { typedef RedAddF64 R; typedef uint64_t V; static __device__ __forceinline__ double conv(V v, KeyCodec<uint64_t>) { return __longlong_as_double((long long)v); } };
template <typename W> struct MinOf { typedef RedMinCode<W> R; typedef W V; static __device__ __forceinline__ W conv(V v, KeyCodec<W> cd) { return cd.enc(v); } };
// COUNT (msd_scan.hpp): every element is worth 1, whatever d_vals holds (it is not read: V only names a pointer type)
struct CountOne { typedef RedAddU64 R; typedef uint32_t V; static __device__ __forceinline__ uint64_t conv(V, KeyCodec<uint64_t>) { return 1; } };
template <> struct ReadsValue<CountOne> : std::false_type {};

// ---- segment pairs, in both directions.  FWD false: the pair of this file (v in front of the FIRST head, a suffix scan,
// the carry flows from right to left); FWD true: the pair of msd_scan.hpp (v from the LAST head on, a prefix scan, the
// carry flows from left to right).  Either way the operands of R::op stand in the order of the elements.
template <typename R> struct SegPair {
	typename R::A v;
	bool f;
};
template <typename R, bool FWD> __device__ __forceinline__ SegPair<R> seg_combine(const SegPair<R> &l, const SegPair<R> &r)
{
	return SegPair<R>{ (FWD ? r.f : l.f) ? (FWD ? r.v : l.v) : R::op(l.v, r.v), l.f || r.f };
}
// `acc` and the pair x that comes next in the direction of the scan: behind it (FWD), in front of it (else)
template <typename R, bool FWD> __device__ __forceinline__ SegPair<R> seg_push(const SegPair<R> &acc, const SegPair<R> &x)
{
	if constexpr (FWD)
		return seg_combine<R, true>(acc, x);
	else
		return seg_combine<R, false>(x, acc);
}

// Inclusive segmented suffix scan over the 64 lanes: lane l gets the combination of the pairs (bit l of f, v) of lanes
// l .. 63.  The flags are a ballot, so whether lane l still takes from lane l + d -- no flag in [l, l + d) -- is a
// shift and a mask, and only the values are shuffled.
template <typename R> __device__ __forceinline__ typename R::A wave_seg_suffix(typename R::A v, uint64_t f)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t from_me = f >> lane;
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const typename R::A t = __shfl_down(v, d);
		if (lane + d < 64u && (from_me & (((uint64_t)1 << d) - 1u)) == 0) v = R::op(v, t);
	}
	return v;
}

// Inclusive segmented prefix scan over the 64 lanes: lane l gets the combination of the pairs (bit l of f, v) of lanes
// 0 .. l.  The flags are a ballot, so whether lane l still takes from lane l - d -- no flag in (l - d, l] -- is a shift
// and a compare, and only the values are shuffled.
template <typename R> __device__ __forceinline__ typename R::A wave_seg_prefix(typename R::A v, uint64_t f)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t up_to_me = f << (63u - lane); // (bit l at bit 63, bit l - j at bit 63 - j)
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const typename R::A t = __shfl_up(v, d);
		if (lane >= d && (up_to_me >> (64u - d)) == 0) v = R::op(t, v);
	}
	return v;
}

// One per tile, and one per piece of kRunsScanTile tiles: the workspace of the tile kernels and the carry.
//   val:  the bits of the tile's lead (reduce) or tail (scan); the carry overwrites it with what flows into the tile
//         from the tiles behind it (reduce: S) or in front of it (scan: P), within the piece.
//   flag: the tile's heads (reduce) or whether it has one (scan); the carry sets kSegClosed if a head closed what flows
//         in within the piece, so that the piece's own carry does not reach the tile.
struct SegRecord {
	uint64_t *val;
	uint32_t *flag;
};
constexpr uint32_t kSegClosed = 1u << 31;

// ---- step 2
template <typename E, typename P, bool POS>
__global__ __launch_bounds__(kRunsTh) void reduce_tile_kernel(const E *__restrict__ keys, uint64_t n, const typename P::V *__restrict__ vals,
	const uint64_t *__restrict__ positions, uint64_t cap, const uint64_t *__restrict__ tile_base, const uint64_t *__restrict__ piece_base,
	KeyCodec<typename P::R::O> cd, typename P::R::O *__restrict__ out, SegRecord rec)
{
	typedef RunsCfg<E> C;
	typedef typename P::R R;
	typedef typename R::A A;
	typedef SegPair<R> Pair;
	constexpr uint32_t V = C::V, WAVES = kRunsTh / 64;
	__shared__ uint32_t wsum[WAVES];
	__shared__ uint32_t wflag[WAVES];
	__shared__ A wlead[WAVES];
	__shared__ A res[C::TILE]; // the parts of the runs that start in the tile, at their run number within the tile
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, m = runs_misalign(keys);
	const uint64_t tile = blockIdx.x;
	const A ident = R::id(cd);
	E x[kRunsVecs][V];
	uint64_t hb[kRunsVecs][V];
	runs_load_heads<E>(keys, n, m, tile, x, hb);
	A a[kRunsVecs][V]; // (what lies outside the array is the identity, and no head)
	runs_load_values<E, P, POS>(n, m, tile, vals, positions, cd, a);
	// the lane's pairs: per k the reduction in front of its first head; the heads in front of k (uniform: runs_rank's
	// before_k, counted in this loop -- apart from it the popcounts cost SGPR spills)
	RunsRank rk;
	uint32_t c = 0;
	uint64_t gb[kRunsVecs];
	A vi[kRunsVecs];
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		rk.before_k[k] = c;
		A lead = ident;
		bool open = true;
		gb[k] = 0;
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			c += (uint32_t)__popcll(hb[k][e]);
			gb[k] |= hb[k][e];
			open = open && !lane_bit(hb[k][e]);
			if (open) lead = R::op(lead, a[k][e]);
		}
		vi[k] = wave_seg_suffix<R>(lead, gb[k]);
	}
	// the k of the wave, from the right: rc[k] = what flows into k from the wave's higher k
	Pair rc[kRunsVecs], acc = Pair{ ident, false };
#pragma unroll
	for (int k = kRunsVecs - 1; k >= 0; --k) {
		rc[k] = acc;
		acc = seg_combine<R, false>(Pair{ __shfl(vi[k], 0), gb[k] != 0 }, acc);
	}
	if (lane == 0) {
		wflag[w] = acc.f ? 1u : 0u;
		wlead[w] = acc.v;
	}
	runs_rank_waves(rk, c, w, lane, wsum); // (its barrier stands behind wflag and wlead too)
	Pair wc = Pair{ ident, false }, all = Pair{ ident, false }; // from the higher waves; the whole tile
#pragma unroll
	for (int ww = (int)WAVES - 1; ww >= 0; --ww) {
		const Pair p = Pair{ wlead[ww], wflag[ww] != 0 };
		if ((uint32_t)ww > w) wc = seg_combine<R, false>(p, wc);
		all = seg_combine<R, false>(p, all);
	}
	const uint32_t heads = rk.total;
	if (threadIdx.x == 0) {
		rec.val[tile] = R::bits(all.v);
		rec.flag[tile] = heads;
	}
	// every head: its part from itself to the element in front of the next head, from the right
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const Pair into_k = seg_combine<R, false>(rc[k], wc);
		const A down = __shfl_down(vi[k], 1); // (every lane takes part)
		const bool closed = ((gb[k] >> lane) >> 1) != 0; // a head in the lanes above, same k
		A r = lane == 63u ? into_k.v : (closed ? down : R::op(down, into_k.v));
		uint32_t incl = rk.wpre + rk.before_k[k];
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) incl += popc_below_lane(hb[k][e]) + (lane_bit(hb[k][e]) ? 1u : 0u);
		// (incl: the heads of the tile up to and including the lane's last element)
#pragma unroll
		for (int e = (int)V - 1; e >= 0; --e) {
			r = R::op(a[k][e], r);
			if (lane_bit(hb[k][e])) {
				res[incl - 1] = r; // (a head is inside the array; incl - 1 < the tile's heads <= TILE)
				--incl;
				r = ident;
			}
		}
	}
	__syncthreads();
	const uint64_t base = tile_out_base(tile_base, piece_base, tile); // heads in front of the tile
	for (uint32_t j = threadIdx.x; j < heads; j += kRunsTh) {
		const uint64_t run = base + j;
		if (run >= cap) break;
		out[run] = R::out(res[j], cd);
	}
}

// ---- step 3: the carry over the records, for this file (FWD false) and for msd_scan.hpp (FWD true)
// Exclusive segmented scan over the workgroup's 256 pairs in the direction FWD: excl = the combination of the pairs of the
// threads this one follows in that direction (below it: FWD; above it: else), total = of all of them.
// (Every thread calls it: barriers.  tmpv, tmpf: 4 words of LDS each.)
template <typename R, bool FWD>
__device__ __forceinline__ void seg_scan_block256(const SegPair<R> mine, typename R::A ident, SegPair<R> &excl, SegPair<R> &total, typename R::A *tmpv,
	uint32_t *tmpf)
{
	typedef SegPair<R> Pair;
	constexpr int WAVES = kRunsScanTh / 64;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint64_t fb = __ballot(mine.f);
	typename R::A vi, next; // the inclusive scan over the wave; that of the lane this one follows
	uint64_t closed;        // the flags of the lanes this one follows
	if constexpr (FWD) {
		vi = wave_seg_prefix<R>(mine.v, fb);
		next = __shfl_up(vi, 1);
		closed = fb & (((uint64_t)1 << lane) - 1u);
	} else {
		vi = wave_seg_suffix<R>(mine.v, fb);
		next = __shfl_down(vi, 1);
		closed = (fb >> lane) >> 1;
	}
	const Pair in_wave = Pair{ lane == (FWD ? 0u : 63u) ? ident : next, closed != 0 };
	__syncthreads(); // (the last call's readers are through with tmp)
	if (lane == (FWD ? 63u : 0u)) { // the lane that holds the whole wave
		tmpv[w] = vi;
		tmpf[w] = fb != 0 ? 1u : 0u;
	}
	__syncthreads();
	Pair wc = Pair{ ident, false };
	total = Pair{ ident, false };
#pragma unroll
	for (int i = 0; i < WAVES; ++i) {
		const int ww = FWD ? i : WAVES - 1 - i;
		const Pair p = Pair{ tmpv[ww], tmpf[ww] != 0 };
		if (FWD ? (uint32_t)ww < w : (uint32_t)ww > w) wc = seg_push<R, FWD>(wc, p);
		total = seg_push<R, FWD>(total, p);
	}
	excl = seg_push<R, FWD>(wc, in_wave);
}

// The `count` <= kRunsScanTile records at (val, flag): every val becomes the combination of the records it follows in
// the direction FWD, on top of `carry` (what lies beyond the piece on that side), and its flag word gets kSegClosed if a
// head closed that combination -- with MARK; the top level needs values only.  Returns the combination of the whole piece
// and the carry.
template <typename R, bool FWD, bool MARK>
__device__ __forceinline__ SegPair<R> seg_carry_piece(uint64_t *__restrict__ val, uint32_t *__restrict__ flag, uint32_t count, SegPair<R> carry,
	typename R::A ident, typename R::A *tmpv, uint32_t *tmpf)
{
	typedef SegPair<R> Pair;
	Pair r[kRunsScanPer], mine = Pair{ ident, false };
#pragma unroll
	for (int i = 0; i < kRunsScanPer; ++i) {
		const int j = FWD ? i : kRunsScanPer - 1 - i;
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		r[j] = idx < count ? Pair{ R::from_bits(val[idx]), (flag[idx] & ~kSegClosed) != 0 } : Pair{ ident, false };
		mine = seg_push<R, FWD>(mine, r[j]);
	}
	Pair excl, total;
	seg_scan_block256<R, FWD>(mine, ident, excl, total, tmpv, tmpf);
	Pair acc = seg_push<R, FWD>(carry, excl);
#pragma unroll
	for (int i = 0; i < kRunsScanPer; ++i) {
		const int j = FWD ? i : kRunsScanPer - 1 - i;
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		if (idx < count) {
			val[idx] = R::bits(acc.v);
			if (MARK && acc.f) flag[idx] |= kSegClosed;
		}
		acc = seg_push<R, FWD>(acc, r[j]);
	}
	return seg_push<R, FWD>(carry, total);
}

// one workgroup per piece of kRunsScanTile records, in place; the piece's summary to `piece`
template <typename R, bool FWD>
__global__ __launch_bounds__(kRunsScanTh) void seg_carry_pieces_kernel(SegRecord rec, uint64_t tiles, KeyCodec<typename R::O> cd, SegRecord piece)
{
	__shared__ typename R::A tmpv[kRunsScanTh / 64];
	__shared__ uint32_t tmpf[kRunsScanTh / 64];
	const typename R::A ident = R::id(cd);
	const uint64_t first = (uint64_t)blockIdx.x * kRunsScanTile;
	const uint32_t count = tiles - first < kRunsScanTile ? (uint32_t)(tiles - first) : kRunsScanTile;
	const SegPair<R> total = seg_carry_piece<R, FWD, true>(rec.val + first, rec.flag + first, count, SegPair<R>{ ident, false }, ident, tmpv, tmpf);
	if (threadIdx.x == 0) {
		piece.val[blockIdx.x] = R::bits(total.v);
		piece.flag[blockIdx.x] = total.f ? 1u : 0u;
	}
}

// ONE workgroup: the piece summaries in the direction FWD, kRunsScanTile at a time (chunks on the grid of kRunsScanTile)
// with a carry
template <typename R, bool FWD>
__global__ __launch_bounds__(kRunsScanTh) void seg_carry_top_kernel(SegRecord piece, uint64_t pieces, KeyCodec<typename R::O> cd)
{
	__shared__ typename R::A tmpv[kRunsScanTh / 64];
	__shared__ uint32_t tmpf[kRunsScanTh / 64];
	const typename R::A ident = R::id(cd);
	const uint64_t chunks = (pieces + kRunsScanTile - 1) / kRunsScanTile;
	SegPair<R> carry = SegPair<R>{ ident, false };
	for (uint64_t i = 0; i < chunks; ++i) {
		const uint64_t first = (FWD ? i : chunks - 1 - i) * kRunsScanTile;
		const uint32_t count = pieces - first < kRunsScanTile ? (uint32_t)(pieces - first) : kRunsScanTile;
		carry = seg_carry_piece<R, FWD, false>(piece.val + first, piece.flag + first, count, carry, ident, tmpv, tmpf);
	}
}

// One thread per tile: the last run that starts in the tile gets what the tiles behind it hold of it.  The tile's own
// part first, then the leads in ascending tile order (through the scan's tree).
template <typename R>
__global__ __launch_bounds__(256) void reduce_apply_kernel(SegRecord rec, SegRecord piece, uint64_t tiles, uint64_t cap, const uint64_t *__restrict__ tile_base,
	const uint64_t *__restrict__ piece_base, KeyCodec<typename R::O> cd, typename R::O *__restrict__ out)
{
	const uint64_t tile = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (tile >= tiles) return;
	const uint32_t word = rec.flag[tile], heads = word & ~kSegClosed;
	if (heads == 0) return;
	const uint64_t run = tile_out_base(tile_base, piece_base, tile) + heads - 1;
	if (run >= cap) return;
	typename R::A s = R::from_bits(rec.val[tile]);
	if (!(word & kSegClosed)) s = R::op(s, R::from_bits(piece.val[tile / kRunsScanTile]));
	out[run] = R::out(R::op(R::in(out[run], cd), s), cd);
}

} // namespace msd

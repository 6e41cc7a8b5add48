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
//      (reduce_carry_pieces_kernel: one workgroup per kRunsScanTile records, in place; reduce_carry_top_kernel: one
//      workgroup over the piece summaries).  reduce_apply_kernel, one thread per tile, combines S(t) into
//      d_out[base(t) + heads(t) - 1].  A tile adds its lead to the run that is open on its LEFT, so the carry flows from
//      right to left.
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

template <typename R> struct SegPair {
	typename R::A v;
	bool f;
};
template <typename R> __device__ __forceinline__ SegPair<R> seg_combine(const SegPair<R> &l, const SegPair<R> &r)
{
	return SegPair<R>{ l.f ? l.v : R::op(l.v, r.v), l.f || r.f };
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

struct ReduceRecord { // one per tile: the workspace of steps 2 and 3
	uint64_t *lead;   // step 2: the bits of the tile's lead; step 3 overwrites it with S (within the piece)
	uint32_t *heads;  // step 2: the tile's heads; step 3 sets kReduceClosed if S is complete within the piece
};
constexpr uint32_t kReduceClosed = 1u << 31;

// ---- step 2
template <typename E, typename P, bool POS>
__global__ __launch_bounds__(kRunsTh) void reduce_tile_kernel(const E *__restrict__ keys, uint64_t n, const typename P::V *__restrict__ vals,
	const uint64_t *__restrict__ positions, uint64_t cap, const uint64_t *__restrict__ tile_base, const uint64_t *__restrict__ piece_base,
	KeyCodec<typename P::R::O> cd, typename P::R::O *__restrict__ out, ReduceRecord rec)
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
	const uint64_t tile = blockIdx.x, lo = m, hi = (uint64_t)m + n;
	const A ident = R::id(cd);
	E x[kRunsVecs][V];
	uint64_t hb[kRunsVecs][V];
	runs_load_heads<E>(keys, n, m, tile, x, hb);
	// the values, once: what lies outside the array counts as the identity (and is no head)
	A a[kRunsVecs][V];
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint64_t v0 = tile * C::TILE + w * C::WAVE + (uint64_t)((k * 64 + lane) * V);
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			const uint64_t v = v0 + e;
			a[k][e] = ident;
			if (v >= lo && v < hi) {
				const uint64_t i = v - lo;
				a[k][e] = P::conv(vals[POS ? positions[i] : i], cd);
			}
		}
	}
	// the lane's pairs: per k the reduction in front of its first head; the heads in front of k (uniform)
	uint32_t before_k[kRunsVecs], c = 0;
	uint64_t gb[kRunsVecs];
	A vi[kRunsVecs];
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		before_k[k] = c;
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
		acc = seg_combine<R>(Pair{ __shfl(vi[k], 0), gb[k] != 0 }, acc);
	}
	if (lane == 0) {
		wsum[w] = c;
		wflag[w] = acc.f ? 1u : 0u;
		wlead[w] = acc.v;
	}
	__syncthreads();
	uint32_t wpre = 0;
	Pair wc = Pair{ ident, false }, all = Pair{ ident, false }; // from the higher waves; the whole tile
#pragma unroll
	for (int ww = (int)WAVES - 1; ww >= 0; --ww) {
		const Pair p = Pair{ wlead[ww], wflag[ww] != 0 };
		if ((uint32_t)ww > w) wc = seg_combine<R>(p, wc);
		if ((uint32_t)ww < w) wpre += wsum[ww];
		all = seg_combine<R>(p, all);
	}
	const uint32_t heads = wsum[0] + wsum[1] + wsum[2] + wsum[3];
	if (threadIdx.x == 0) {
		rec.lead[tile] = R::bits(all.v);
		rec.heads[tile] = heads;
	}
	// every head: its part from itself to the element in front of the next head, from the right
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const Pair into_k = seg_combine<R>(rc[k], wc);
		const A down = __shfl_down(vi[k], 1); // (every lane takes part)
		const bool closed = ((gb[k] >> lane) >> 1) != 0; // a head in the lanes above, same k
		A r = lane == 63u ? into_k.v : (closed ? down : R::op(down, into_k.v));
		uint32_t incl = wpre + before_k[k];
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
	const uint64_t base = tile_base[tile] + piece_base[tile / kRunsScanTile]; // heads in front of the tile
	for (uint32_t j = threadIdx.x; j < heads; j += kRunsTh) {
		const uint64_t run = base + j;
		if (run >= cap) break;
		out[run] = R::out(res[j], cd);
	}
}

// ---- step 3
// Exclusive segmented suffix scan over the workgroup's 256 pairs: (xf, xv) = the combination of the pairs of the threads
// above this one, (tf, tv) = of all of them.  (Every thread calls it: barriers.  tmpv, tmpf: 4 words of LDS each.)
template <typename R>
__device__ __forceinline__ void seg_suffix_block256(const SegPair<R> mine, typename R::A ident, SegPair<R> &excl, SegPair<R> &total, typename R::A *tmpv,
	uint32_t *tmpf)
{
	typedef SegPair<R> Pair;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint64_t fb = __ballot(mine.f);
	const typename R::A vi = wave_seg_suffix<R>(mine.v, fb);
	const typename R::A down = __shfl_down(vi, 1);
	const Pair in_wave = Pair{ lane == 63u ? ident : down, ((fb >> lane) >> 1) != 0 };
	__syncthreads(); // (the last call's readers are through with tmp)
	if (lane == 0) {
		tmpv[w] = vi;
		tmpf[w] = fb != 0 ? 1u : 0u;
	}
	__syncthreads();
	Pair wc = Pair{ ident, false };
	total = Pair{ ident, false };
#pragma unroll
	for (int ww = kRunsScanTh / 64 - 1; ww >= 0; --ww) {
		const Pair p = Pair{ tmpv[ww], tmpf[ww] != 0 };
		if ((uint32_t)ww > w) wc = seg_combine<R>(p, wc);
		total = seg_combine<R>(p, total);
	}
	excl = seg_combine<R>(in_wave, wc);
}

// The `count` <= kRunsScanTile records at (lead, heads): every lead becomes the combination of the records behind it, on
// top of `carry` (what lies behind the piece), and its heads word gets kReduceClosed if a head closed that combination
// -- with MARK; the top level needs values only.  Returns the combination of the whole piece and the carry.
template <typename R, bool MARK>
__device__ __forceinline__ SegPair<R> reduce_carry_piece(uint64_t *__restrict__ lead, uint32_t *__restrict__ heads, uint32_t count, SegPair<R> carry,
	typename R::A ident, typename R::A *tmpv, uint32_t *tmpf)
{
	typedef SegPair<R> Pair;
	Pair r[kRunsScanPer], mine = Pair{ ident, false };
#pragma unroll
	for (int j = kRunsScanPer - 1; j >= 0; --j) {
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		r[j] = idx < count ? Pair{ R::from_bits(lead[idx]), (heads[idx] & ~kReduceClosed) != 0 } : Pair{ ident, false };
		mine = seg_combine<R>(r[j], mine);
	}
	Pair excl, total;
	seg_suffix_block256<R>(mine, ident, excl, total, tmpv, tmpf);
	Pair acc = seg_combine<R>(excl, carry);
#pragma unroll
	for (int j = kRunsScanPer - 1; j >= 0; --j) {
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		if (idx < count) {
			lead[idx] = R::bits(acc.v);
			if (MARK && acc.f) heads[idx] |= kReduceClosed;
		}
		acc = seg_combine<R>(r[j], acc);
	}
	return seg_combine<R>(total, carry);
}

template <typename R>
__global__ __launch_bounds__(kRunsScanTh) void reduce_carry_pieces_kernel(ReduceRecord rec, uint64_t tiles, KeyCodec<typename R::O> cd, ReduceRecord piece)
{
	__shared__ typename R::A tmpv[kRunsScanTh / 64];
	__shared__ uint32_t tmpf[kRunsScanTh / 64];
	const typename R::A ident = R::id(cd);
	const uint64_t first = (uint64_t)blockIdx.x * kRunsScanTile;
	const uint32_t count = tiles - first < kRunsScanTile ? (uint32_t)(tiles - first) : kRunsScanTile;
	const SegPair<R> total = reduce_carry_piece<R, true>(rec.lead + first, rec.heads + first, count, SegPair<R>{ ident, false }, ident, tmpv, tmpf);
	if (threadIdx.x == 0) {
		piece.lead[blockIdx.x] = R::bits(total.v);
		piece.heads[blockIdx.x] = total.f ? 1u : 0u;
	}
}

// ONE workgroup: the piece summaries from the right, kRunsScanTile at a time with a carry
template <typename R>
__global__ __launch_bounds__(kRunsScanTh) void reduce_carry_top_kernel(ReduceRecord piece, uint64_t pieces, KeyCodec<typename R::O> cd)
{
	__shared__ typename R::A tmpv[kRunsScanTh / 64];
	__shared__ uint32_t tmpf[kRunsScanTh / 64];
	const typename R::A ident = R::id(cd);
	SegPair<R> carry = SegPair<R>{ ident, false };
	for (uint64_t left = pieces; left > 0;) {
		const uint32_t count = left % kRunsScanTile ? (uint32_t)(left % kRunsScanTile) : kRunsScanTile; // (the chunks lie on the grid of kRunsScanTile)
		left -= count;
		carry = reduce_carry_piece<R, false>(piece.lead + left, piece.heads + left, count, carry, ident, tmpv, tmpf);
	}
}

// One thread per tile: the last run that starts in the tile gets what the tiles behind it hold of it.  The tile's own
// part first, then the leads in ascending tile order (through the scan's tree).
template <typename R>
__global__ __launch_bounds__(256) void reduce_apply_kernel(ReduceRecord rec, ReduceRecord piece, uint64_t tiles, uint64_t cap, const uint64_t *__restrict__ tile_base,
	const uint64_t *__restrict__ piece_base, KeyCodec<typename R::O> cd, typename R::O *__restrict__ out)
{
	const uint64_t tile = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (tile >= tiles) return;
	const uint32_t word = rec.heads[tile], heads = word & ~kReduceClosed;
	if (heads == 0) return;
	const uint64_t run = tile_base[tile] + piece_base[tile / kRunsScanTile] + heads - 1;
	if (run >= cap) return;
	typename R::A s = R::from_bits(rec.lead[tile]);
	if (!(word & kReduceClosed)) s = R::op(s, R::from_bits(piece.lead[tile / kRunsScanTile]));
	out[run] = R::out(R::op(R::in(out[run], cd), s), cd);
}

} // namespace msd

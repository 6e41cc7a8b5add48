// msd_scan.hpp -- scan-by-key over runs: msd_scan_runs.
//
// The runs are those of msd_runs.hpp (same tiles, same head ballots) and the values, accumulators and policies those of
// msd_reduce.hpp; this file writes one number per ELEMENT: the sum, the minimum, the maximum or the count of the elements
// of its run up to it (inclusive) or in front of it (exclusive).  Nothing depends on the run numbers, so the count and
// scan kernels of msd_runs.hpp are not launched.  No workgroup waits for another one and there are no atomics: stream
// order is the only barrier between the steps, and the order every result is evaluated in is fixed by the tile geometry
// alone.
//   1. scan_tail_kernel: reads the tile's keys and values and writes the tile's
//      RECORD: whether it has a head, and its TAIL -- the reduction from its last head to its end, of the whole tile if
//      it has none.
//   2. The run that is open at the start of tile t holds P(t) from the tiles in front of it: the exclusive segmented
//      PREFIX scan over the records, two levels deep (scan_carry_pieces_kernel: one workgroup per kRunsScanTile records,
//      in place; scan_carry_top_kernel: one workgroup over the piece summaries).  A tile hands its tail to the run that is
//      open on its RIGHT, so the carry flows from left to right -- the mirror of msd_reduce.hpp, whose tiles hand their
//      leads to the left.
//   3. scan_tile_kernel: reads keys and values again, scans them by a segmented prefix scan on top of P(t) and stores the
//      n results in the order of the elements.
// Values through positions and results scattered through them are not built: msd_scan_runs refuses d_positions.
//
// A segment pair is (f, v) as in msd_reduce.hpp, seen from the other end: v = the reduction of the elements from the LAST
// head of a stretch to its end (of all of them if it has none), f = whether it has a head.
// combine(L, R) = (L.f | R.f, R.f ? R.v : op(L.v, R.v)) is associative; every level below is a prefix scan under it: the e
// of a lane, the lanes of a k, the k of a wave, the waves of a workgroup, the tiles of a piece, the pieces.
#pragma once

#include "msd_reduce.hpp"

#include <type_traits>

namespace msd {

// COUNT: every element is worth 1, whatever d_vals holds (it is not read: V only names a pointer type)
struct CountOne { typedef RedAddU64 R; typedef uint32_t V; static __device__ __forceinline__ uint64_t conv(V, KeyCodec<uint64_t>) { return 1; } };

template <typename R> __device__ __forceinline__ SegPair<R> seg_combine_fwd(const SegPair<R> &l, const SegPair<R> &r)
{
	return SegPair<R>{ r.f ? r.v : R::op(l.v, r.v), l.f || r.f };
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

struct ScanRecord { // one per tile: the workspace of steps 1 and 2
	uint64_t *tail;  // step 1: the bits of the tile's tail; step 2 overwrites it with P (within the piece)
	uint32_t *flag;  // step 1: 1 if the tile has a head; step 2 sets kScanClosed if P is complete within the piece
};
constexpr uint32_t kScanClosed = 1u << 31;
constexpr int kScanExclusive = 1; // MSD_SCAN_EXCLUSIVE

// The values of this lane's elements of tile `tile`, once: what lies outside the array counts as the identity
template <typename E, typename P>
__device__ __forceinline__ void scan_load_values(uint64_t n, uint32_t m, uint64_t tile, const typename P::V *__restrict__ vals,
	KeyCodec<typename P::R::O> cd, typename P::R::A (&a)[kRunsVecs][RunsCfg<E>::V])
{
	typedef RunsCfg<E> C;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint64_t lo = m, hi = (uint64_t)m + n;
	const typename P::R::A ident = P::R::id(cd);
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const uint64_t v0 = tile * C::TILE + w * C::WAVE + (uint64_t)((k * 64 + lane) * C::V);
#pragma unroll
		for (uint32_t e = 0; e < C::V; ++e) {
			const uint64_t v = v0 + e;
			a[k][e] = ident;
			if (v >= lo && v < hi) {
				const uint64_t i = v - lo;
				if constexpr (std::is_same<P, CountOne>::value)
					a[k][e] = 1;
				else
					a[k][e] = P::conv(vals[i], cd);
			}
		}
	}
}

// What the scan needs of the sixteen head ballots of runs_load_heads: hm[k] = bit e set where the lane's element (k, e) is a
// head (a lane's own word), gb[k] = the lanes that hold a head (uniform).  The empty asm makes hm a value of its own: the
// four words are computed here, once, in front of the loads of the values, and not read back out of the ballots later.
template <uint32_t V>
__device__ __forceinline__ void scan_head_masks(const uint64_t (&hb)[kRunsVecs][V], uint32_t (&hm)[kRunsVecs], uint64_t (&gb)[kRunsVecs])
{
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		hm[k] = 0;
		gb[k] = 0;
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			gb[k] |= hb[k][e];
			hm[k] |= lane_bit(hb[k][e]) ? 1u << e : 0u;
		}
		asm volatile("" : "+v"(hm[k]));
	}
}

// The wave's part of a tile, from the left.  Per k: vi[k] = the inclusive scan over the lanes of every lane's own pair
// (its V elements from the left), lc[k] = what flows into k from the wave's lower k.  Returns the wave's pair (uniform).
template <typename R, uint32_t V>
__device__ __forceinline__ SegPair<R> scan_wave_pairs(const typename R::A (&a)[kRunsVecs][V], const uint32_t (&hm)[kRunsVecs], const uint64_t (&gb)[kRunsVecs],
	typename R::A ident, typename R::A (&vi)[kRunsVecs], SegPair<R> (&lc)[kRunsVecs])
{
	typedef SegPair<R> Pair;
	Pair acc = Pair{ ident, false };
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		typename R::A tail = ident;
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) tail = (hm[k] >> e & 1u) ? a[k][e] : R::op(tail, a[k][e]);
		vi[k] = wave_seg_prefix<R>(tail, gb[k]);
		lc[k] = acc;
		acc = seg_combine_fwd<R>(acc, Pair{ __shfl(vi[k], 63), gb[k] != 0 });
	}
	return acc;
}

// ---- step 1
// (The record is the last pair of the scan that step 3 makes: scan_wave_pairs is called as it is, and the prefixes vi and lc
// it also yields are dropped here.  A bare reduction would halve the shuffle steps of a kernel that waits for its loads; in
// return the record and the scan it feeds cannot differ in how they group the elements.)
template <typename E, typename P>
__global__ __launch_bounds__(kRunsTh) void scan_tail_kernel(const E *__restrict__ keys, uint64_t n, const typename P::V *__restrict__ vals,
	KeyCodec<typename P::R::O> cd, ScanRecord rec)
{
	typedef RunsCfg<E> C;
	typedef typename P::R R;
	typedef typename R::A A;
	typedef SegPair<R> Pair;
	constexpr uint32_t V = C::V, WAVES = kRunsTh / 64;
	__shared__ uint32_t wflag[WAVES];
	__shared__ A wtail[WAVES];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, m = runs_misalign(keys);
	const uint64_t tile = blockIdx.x;
	const A ident = R::id(cd);
	E x[kRunsVecs][V];
	uint64_t hb[kRunsVecs][V];
	runs_load_heads<E>(keys, n, m, tile, x, hb);
	uint32_t hm[kRunsVecs];
	uint64_t gb[kRunsVecs];
	scan_head_masks<V>(hb, hm, gb);
	A a[kRunsVecs][V];
	scan_load_values<E, P>(n, m, tile, vals, cd, a);
	A vi[kRunsVecs];
	Pair lc[kRunsVecs];
	const Pair mine = scan_wave_pairs<R, V>(a, hm, gb, ident, vi, lc);
	if (lane == 0) {
		wflag[w] = mine.f ? 1u : 0u;
		wtail[w] = mine.v;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		Pair all = Pair{ ident, false };
#pragma unroll
		for (uint32_t ww = 0; ww < WAVES; ++ww) all = seg_combine_fwd<R>(all, Pair{ wtail[ww], wflag[ww] != 0 });
		rec.tail[tile] = R::bits(all.v);
		rec.flag[tile] = all.f ? 1u : 0u;
	}
}

// ---- step 2
// Exclusive segmented prefix scan over the workgroup's 256 pairs: excl = the combination of the pairs of the threads below
// this one, total = of all of them.  (Every thread calls it: barriers.  tmpv, tmpf: 4 words of LDS each.)
template <typename R>
__device__ __forceinline__ void seg_prefix_block256(const SegPair<R> mine, typename R::A ident, SegPair<R> &excl, SegPair<R> &total, typename R::A *tmpv,
	uint32_t *tmpf)
{
	typedef SegPair<R> Pair;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint64_t fb = __ballot(mine.f);
	const typename R::A vi = wave_seg_prefix<R>(mine.v, fb);
	const typename R::A up = __shfl_up(vi, 1);
	const Pair in_wave = Pair{ lane == 0 ? ident : up, (fb & (((uint64_t)1 << lane) - 1u)) != 0 };
	__syncthreads(); // (the last call's readers are through with tmp)
	if (lane == 63u) {
		tmpv[w] = vi;
		tmpf[w] = fb != 0 ? 1u : 0u;
	}
	__syncthreads();
	Pair wc = Pair{ ident, false };
	total = Pair{ ident, false };
#pragma unroll
	for (uint32_t ww = 0; ww < kRunsScanTh / 64; ++ww) {
		const Pair p = Pair{ tmpv[ww], tmpf[ww] != 0 };
		if (ww < w) wc = seg_combine_fwd<R>(wc, p);
		total = seg_combine_fwd<R>(total, p);
	}
	excl = seg_combine_fwd<R>(wc, in_wave);
}

// The `count` <= kRunsScanTile records at (tail, flag): every tail becomes the combination of the records in front of it,
// on top of `carry` (what lies in front of the piece), and its flag word gets kScanClosed if a head closed that
// combination -- with MARK; the top level needs values only.  Returns the combination of the carry and the whole piece.
template <typename R, bool MARK>
__device__ __forceinline__ SegPair<R> scan_carry_piece(uint64_t *__restrict__ tail, uint32_t *__restrict__ flag, uint32_t count, SegPair<R> carry,
	typename R::A ident, typename R::A *tmpv, uint32_t *tmpf)
{
	typedef SegPair<R> Pair;
	Pair r[kRunsScanPer], mine = Pair{ ident, false };
#pragma unroll
	for (int j = 0; j < kRunsScanPer; ++j) {
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		r[j] = idx < count ? Pair{ R::from_bits(tail[idx]), (flag[idx] & ~kScanClosed) != 0 } : Pair{ ident, false };
		mine = seg_combine_fwd<R>(mine, r[j]);
	}
	Pair excl, total;
	seg_prefix_block256<R>(mine, ident, excl, total, tmpv, tmpf);
	Pair acc = seg_combine_fwd<R>(carry, excl);
#pragma unroll
	for (int j = 0; j < kRunsScanPer; ++j) {
		const uint32_t idx = threadIdx.x * kRunsScanPer + j;
		if (idx < count) {
			tail[idx] = R::bits(acc.v);
			if (MARK && acc.f) flag[idx] |= kScanClosed;
		}
		acc = seg_combine_fwd<R>(acc, r[j]);
	}
	return seg_combine_fwd<R>(carry, total);
}

template <typename R>
__global__ __launch_bounds__(kRunsScanTh) void scan_carry_pieces_kernel(ScanRecord rec, uint64_t tiles, KeyCodec<typename R::O> cd, ScanRecord piece)
{
	__shared__ typename R::A tmpv[kRunsScanTh / 64];
	__shared__ uint32_t tmpf[kRunsScanTh / 64];
	const typename R::A ident = R::id(cd);
	const uint64_t first = (uint64_t)blockIdx.x * kRunsScanTile;
	const uint32_t count = tiles - first < kRunsScanTile ? (uint32_t)(tiles - first) : kRunsScanTile;
	const SegPair<R> total = scan_carry_piece<R, true>(rec.tail + first, rec.flag + first, count, SegPair<R>{ ident, false }, ident, tmpv, tmpf);
	if (threadIdx.x == 0) {
		piece.tail[blockIdx.x] = R::bits(total.v);
		piece.flag[blockIdx.x] = total.f ? 1u : 0u;
	}
}

// ONE workgroup: the piece summaries from the left, kRunsScanTile at a time with a carry
template <typename R>
__global__ __launch_bounds__(kRunsScanTh) void scan_carry_top_kernel(ScanRecord piece, uint64_t pieces, KeyCodec<typename R::O> cd)
{
	__shared__ typename R::A tmpv[kRunsScanTh / 64];
	__shared__ uint32_t tmpf[kRunsScanTh / 64];
	const typename R::A ident = R::id(cd);
	SegPair<R> carry = SegPair<R>{ ident, false };
	for (uint64_t first = 0; first < pieces; first += kRunsScanTile) {
		const uint32_t count = pieces - first < kRunsScanTile ? (uint32_t)(pieces - first) : kRunsScanTile;
		carry = scan_carry_piece<R, false>(piece.tail + first, piece.flag + first, count, carry, ident, tmpv, tmpf);
	}
}

// ---- step 3
// Every element: the reduction from its run's head up to it (exclusive: up to the element in front of it, the identity
// at a head), stored at its index.  The flag is uniform.
template <typename E, typename P>
__global__ __launch_bounds__(kRunsTh) void scan_tile_kernel(const E *__restrict__ keys, uint64_t n, const typename P::V *__restrict__ vals,
	KeyCodec<typename P::R::O> cd, ScanRecord rec, ScanRecord piece, int flags, typename P::R::O *__restrict__ out)
{
	typedef RunsCfg<E> C;
	typedef typename P::R R;
	typedef typename R::A A;
	typedef SegPair<R> Pair;
	constexpr uint32_t V = C::V, WAVES = kRunsTh / 64;
	__shared__ uint32_t wflag[WAVES];
	__shared__ A wtail[WAVES];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, m = runs_misalign(keys);
	const uint64_t tile = blockIdx.x, lo = m, hi = (uint64_t)m + n;
	const A ident = R::id(cd);
	const bool exclusive = (flags & kScanExclusive) != 0;
	E x[kRunsVecs][V];
	uint64_t hb[kRunsVecs][V];
	runs_load_heads<E>(keys, n, m, tile, x, hb);
	uint32_t hm[kRunsVecs];
	uint64_t gb[kRunsVecs];
	scan_head_masks<V>(hb, hm, gb);
	A a[kRunsVecs][V];
	scan_load_values<E, P>(n, m, tile, vals, cd, a);
	A vi[kRunsVecs];
	Pair lc[kRunsVecs];
	const Pair mine = scan_wave_pairs<R, V>(a, hm, gb, ident, vi, lc);
	if (lane == 0) {
		wflag[w] = mine.f ? 1u : 0u;
		wtail[w] = mine.v;
	}
	__syncthreads();
	// what flows into the wave: P(t) -- on top of the piece's carry where no head closed it -- and the waves below
	A p = R::from_bits(rec.tail[tile]);
	if (!(rec.flag[tile] & kScanClosed)) p = R::op(R::from_bits(piece.tail[tile / kRunsScanTile]), p);
	Pair wc = Pair{ p, false };
#pragma unroll
	for (uint32_t ww = 0; ww < WAVES - 1; ++ww)
		if (ww < w) wc = seg_combine_fwd<R>(wc, Pair{ wtail[ww], wflag[ww] != 0 });
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const Pair into_k = seg_combine_fwd<R>(wc, lc[k]);
		const A up = __shfl_up(vi[k], 1); // (every lane takes part)
		const bool closed = (gb[k] & (((uint64_t)1 << lane) - 1u)) != 0; // a head in the lanes below, same k
		A r = lane == 0 ? into_k.v : (closed ? up : R::op(into_k.v, up));
		const uint64_t v0 = tile * C::TILE + w * C::WAVE + (uint64_t)((k * 64 + lane) * V);
#pragma unroll
		for (uint32_t e = 0; e < V; ++e) {
			const uint64_t v = v0 + e;
			const bool head = (hm[k] >> e & 1u) != 0;
			const A before = head ? ident : r;
			r = head ? a[k][e] : R::op(r, a[k][e]);
			if (v >= lo && v < hi) {
				const uint64_t i = v - lo;
				out[i] = R::out(exclusive ? before : r, cd);
			}
		}
	}
}

} // namespace msd

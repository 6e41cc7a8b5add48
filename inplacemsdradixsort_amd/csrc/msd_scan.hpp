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
//      PREFIX scan over the records, two levels deep: the carry kernels of msd_reduce.hpp with FWD true
//      (seg_carry_pieces_kernel: one workgroup per kRunsScanTile records, in place; seg_carry_top_kernel: one workgroup
//      over the piece summaries).  A tile hands its tail to the run that is open on its RIGHT, so the carry flows from left
//      to right -- the mirror of msd_reduce.hpp, whose tiles hand their leads to the left.
//   3. scan_tile_kernel: reads keys and values again, scans them by a segmented prefix scan on top of P(t) and stores the
//      n results in the order of the elements.
// Values through positions and results scattered through them are not built: msd_scan_runs refuses d_positions.
//
// A segment pair is (f, v) as in msd_reduce.hpp, seen from the other end (seg_combine<R, true>): v = the reduction of the
// elements from the LAST head of a stretch to its end (of all of them if it has none), f = whether it has a head.
// combine(L, R) = (L.f | R.f, R.f ? R.v : op(L.v, R.v)) is associative; every level below is a prefix scan under it: the e
// of a lane, the lanes of a k, the k of a wave, the waves of a workgroup, the tiles of a piece, the pieces.
#pragma once

#include "msd_reduce.hpp"

namespace msd {

constexpr int kScanExclusive = 1; // MSD_SCAN_EXCLUSIVE

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
		acc = seg_combine<R, true>(acc, Pair{ __shfl(vi[k], 63), gb[k] != 0 });
	}
	return acc;
}

// ---- step 1
// (The record is the last pair of the scan that step 3 makes: scan_wave_pairs is called as it is, and the prefixes vi and lc
// it also yields are dropped here.  A bare reduction would halve the shuffle steps of a kernel that waits for its loads; in
// return the record and the scan it feeds cannot differ in how they group the elements.)
template <typename E, typename P>
__global__ __launch_bounds__(kRunsTh) void scan_tail_kernel(const E *__restrict__ keys, uint64_t n, const typename P::V *__restrict__ vals,
	KeyCodec<typename P::R::O> cd, SegRecord rec)
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
	runs_load_values<E, P, false>(n, m, tile, vals, nullptr, cd, a);
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
		for (uint32_t ww = 0; ww < WAVES; ++ww) all = seg_combine<R, true>(all, Pair{ wtail[ww], wflag[ww] != 0 });
		rec.val[tile] = R::bits(all.v);
		rec.flag[tile] = all.f ? 1u : 0u;
	}
}

// ---- step 2: seg_carry_pieces_kernel<R, true>, seg_carry_top_kernel<R, true> (msd_reduce.hpp)

// ---- step 3
// Every element: the reduction from its run's head up to it (exclusive: up to the element in front of it, the identity
// at a head), stored at its index.  The flag is uniform.
template <typename E, typename P>
__global__ __launch_bounds__(kRunsTh) void scan_tile_kernel(const E *__restrict__ keys, uint64_t n, const typename P::V *__restrict__ vals,
	KeyCodec<typename P::R::O> cd, SegRecord rec, SegRecord piece, int flags, typename P::R::O *__restrict__ out)
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
	runs_load_values<E, P, false>(n, m, tile, vals, nullptr, cd, a);
	A vi[kRunsVecs];
	Pair lc[kRunsVecs];
	const Pair mine = scan_wave_pairs<R, V>(a, hm, gb, ident, vi, lc);
	if (lane == 0) {
		wflag[w] = mine.f ? 1u : 0u;
		wtail[w] = mine.v;
	}
	__syncthreads();
	// what flows into the wave: P(t) -- on top of the piece's carry where no head closed it -- and the waves below
	A p = R::from_bits(rec.val[tile]);
	if (!(rec.flag[tile] & kSegClosed)) p = R::op(R::from_bits(piece.val[tile / kRunsScanTile]), p);
	Pair wc = Pair{ p, false };
#pragma unroll
	for (uint32_t ww = 0; ww < WAVES - 1; ++ww)
		if (ww < w) wc = seg_combine<R, true>(wc, Pair{ wtail[ww], wflag[ww] != 0 });
#pragma unroll
	for (int k = 0; k < kRunsVecs; ++k) {
		const Pair into_k = seg_combine<R, true>(wc, lc[k]);
		const A up = __shfl_up(vi[k], 1); // (every lane takes part)
		const bool closed = (gb[k] & (((uint64_t)1 << lane) - 1u)) != 0; // a head in the lanes below, same k
		A r = lane == 0 ? into_k.v : (closed ? up : R::op(into_k.v, up));
		const uint64_t v0 = runs_vindex<E>(tile, w, lane, k);
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

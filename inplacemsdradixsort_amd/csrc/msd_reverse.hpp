// msd_reverse.hpp -- typed and descending order behind the unsigned sort.
//
// The sort orders unsigned bit patterns.  Afterwards the array is [keys without the sign bit, ascending][keys with it,
// ascending by pattern]; with P = the first block's length and N = n - P, every typed order is that array with at most
// three ranges reversed in place (R[a,b) = elements a .. b-1 reversed):
//
//   key kind   ascending                                              descending
//   unsigned   nothing                                                R[0,n)
//   signed     nothing if N == 0 or P == 0; else R[0,n), then         R[0,P) and R[P,n)
//              R[0,N) and R[N,n)
//   float      nothing if N == 0; R[0,n) if P == 0; else R[0,n),      R[0,P)
//              then R[N,n)
//
// sign_split_kernel finds P and writes the ranges into the PLAN, a few device words; reverse_ranges_kernel, launched once
// per stage, reads its stage's ranges from there: the host never learns P, the call adds no host wait.  No key bit is
// transformed anywhere: NaN payloads and -0 come back bit-exact.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msd_keycodec.hpp"

namespace msd {

// ---- the plan: uint64 words
enum {
	kFixStage1 = 0,   // a0, b0, a1, b1: up to two disjoint ranges, reversed by the first launch (an empty range: a == b)
	kFixStage2 = 4,   // the same for the second launch (stream order is the barrier between the two)
	kFixSplit = 8,    // P (unsigned key types have no sign bit: n)
	kFixReversed = 9, // sum of the lengths of the ranges above that have at least 2 elements
	kFixWords = 16
};

// ---- geometry of reverse_ranges_kernel
constexpr int kRevTh = 256;
constexpr int kRevVecs = 4;                       // 16-byte loads in flight per lane and side (8 per lane in all)
constexpr uint32_t kRevSlots = kRevTh * kRevVecs; // 16-byte slots of one side's LDS buffer (16 KiB)
template <typename E> struct RevCfg {
	static constexpr uint32_t V = 16 / sizeof(E);          // elements per 16 bytes
	typedef E Vec __attribute__((ext_vector_type(16 / sizeof(E))));
	// A tile lies in its LDS buffer at the offset its first element has in its 16-byte line of global memory (0 .. V-1
	// elements), so that every aligned 16 bytes of global memory are one aligned slot: one slot less than the buffer holds.
	static constexpr uint32_t TILE = (kRevSlots - 1) * V;  // elements: 4092 (4-byte), 2046 (8-byte)
};

// workgroups a range of `len` elements needs: one per pair of whole tiles (front + mirror), one for a remainder of 2 or more
template <typename E> __host__ __device__ inline uint64_t rev_workgroups(uint64_t len)
{
	const uint64_t pairs = len / (2 * RevCfg<E>::TILE);
	return pairs + (len - pairs * 2 * RevCfg<E>::TILE >= 2 ? 1 : 0);
}
// what the host launches for ranges that are disjoint parts of n elements, at most two of them
template <typename E> inline uint64_t rev_grid_for(uint64_t n) { return n / (2 * RevCfg<E>::TILE) + 2; }

// ---- P and the plan.  One wave: 64 probes per step cut the interval to a 64th, 6 dependent steps for 2^36 keys.
// kind: 0 unsigned, 1 signed, 2 float (key_type % 3); descending: 0 / 1.
template <typename K>
__global__ __launch_bounds__(64) void sign_split_kernel(const K *__restrict__ keys, uint64_t n, int kind, int descending, uint64_t *__restrict__ plan)
{
	constexpr K SIGN = (K)1 << (sizeof(K) * 8 - 1);
	const uint32_t lane = threadIdx.x;
	uint64_t lo = 0, hi = kind == 0 ? 0 : n; // the answer lies in [lo, hi]; keys[hi] counts as set
	while (lo < hi) {
		const uint64_t step = (hi - lo + 63) / 64;
		const uint64_t p = lo + lane * step;
		const bool set = p >= hi || (keys[p] & SIGN) != 0;
		const unsigned long long m = __ballot(set);
		if (m & 1) break;                                   // keys[lo] is set: P = lo
		const uint32_t f = m ? (uint32_t)__ffsll(m) - 1 : 64; // first probe that is set: the one in front of it is not
		const uint64_t nlo = lo + (f - 1) * step + 1, nhi = lo + f * step;
		lo = nlo;
		hi = nhi < hi ? nhi : hi;
	}
	if (lane != 0) return;
	const uint64_t P = kind == 0 ? n : lo, N = n - P;
	uint64_t r[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	const auto put = [&](int at, uint64_t a, uint64_t b) { r[at] = a; r[at + 1] = b; };
	if (descending) {
		if (kind == 0) put(0, 0, n);
		else {
			put(0, 0, P);
			if (kind == 1) put(2, P, n);
		}
	} else if (kind != 0 && N != 0) {
		if (P != 0 || kind == 2) put(0, 0, n);
		if (P != 0) {
			put(6, N, n);
			if (kind == 1) put(4, 0, N);
		}
	}
	uint64_t sum = 0;
#pragma unroll
	for (int i = 0; i < 8; i += 2) {
		plan[i] = r[i];
		plan[i + 1] = r[i + 1];
		if (r[i + 1] - r[i] >= 2) sum += r[i + 1] - r[i];
	}
	plan[kFixSplit] = P;
	plan[kFixReversed] = sum;
}

// ---- the reversal
// One side of a workgroup's job: the L elements from data[s] on, element j at index m + j of its LDS buffer, m = the
// offset of data + s in its 16-byte line.  Slot i of the buffer (V elements from index V * i on) is then one aligned
// 16 bytes of global memory; a slot that lies only partly inside [m, m + L) -- the first and the last one, at most --
// is moved element by element, and nothing outside the L elements is read or written.
template <typename E> __device__ __forceinline__ void rev_load_side(typename RevCfg<E>::Vec (&v)[kRevVecs], const E *base, uint32_t L, uint32_t m)
{
	constexpr uint32_t V = RevCfg<E>::V;
	typedef typename RevCfg<E>::Vec Vec;
#pragma unroll
	for (int k = 0; k < kRevVecs; ++k) {
		const uint32_t lo = (threadIdx.x + k * kRevTh) * V;
		if (lo >= m && lo + V <= m + L) {
			v[k] = *reinterpret_cast<const Vec *>(base + ((ptrdiff_t)lo - (ptrdiff_t)m));
		} else {
#pragma unroll
			for (uint32_t e = 0; e < V; ++e) {
				const uint32_t idx = lo + e;
				v[k][e] = (idx >= m && idx < m + L) ? base[(ptrdiff_t)idx - (ptrdiff_t)m] : (E)0;
			}
		}
	}
}
// element j of this side <- element L-1-j of the other side, which lies at index ms + L-1-j of `src`
template <typename E> __device__ __forceinline__ void rev_store_side(E *base, uint32_t L, uint32_t m, const E *src, uint32_t ms)
{
	constexpr uint32_t V = RevCfg<E>::V;
	typedef typename RevCfg<E>::Vec Vec;
	const uint32_t top = ms + L - 1 + m; // buffer index idx here <- src[top - idx]
#pragma unroll
	for (int k = 0; k < kRevVecs; ++k) {
		const uint32_t lo = (threadIdx.x + k * kRevTh) * V;
		if (lo >= m && lo + V <= m + L) {
			Vec x;
#pragma unroll
			for (uint32_t e = 0; e < V; ++e) x[e] = src[top - (lo + e)];
			*reinterpret_cast<Vec *>(base + ((ptrdiff_t)lo - (ptrdiff_t)m)) = x;
		} else {
#pragma unroll
			for (uint32_t e = 0; e < V; ++e) {
				const uint32_t idx = lo + e;
				if (idx >= m && idx < m + L) base[(ptrdiff_t)idx - (ptrdiff_t)m] = src[top - idx];
			}
		}
	}
}

// Reverses up to two disjoint ranges of `data` in place: plan[0..4) = a0, b0, a1, b1, or, without a plan, [a0, b0) alone.
// Workgroup t of a range [a, b) takes tile t from the front and its mirror tile from the back, loads both completely
// (all loads issued before anything is stored: the barrier between the LDS writes and reads stands between them), and
// stores each reversed into the other's place.  The remainder in the middle, fewer than two tiles, is ONE workgroup's:
// its front half and its back half, which share the middle element of an odd range -- both write it the value it has.
// The grid comes from n alone (rev_grid_for): workgroups beyond the ranges' tiles leave at once.
template <typename E>
__global__ __launch_bounds__(kRevTh) void reverse_ranges_kernel(E *data, const uint64_t *__restrict__ plan, uint64_t a0, uint64_t b0)
{
	constexpr uint32_t V = RevCfg<E>::V, T = RevCfg<E>::TILE;
	typedef typename RevCfg<E>::Vec Vec;
	__shared__ Vec lds[2][kRevSlots];
	uint64_t a = a0, b = b0, a1 = 0, b1 = 0;
	if (plan) {
		a = plan[0];
		b = plan[1];
		a1 = plan[2];
		b1 = plan[3];
	}
	uint64_t t = blockIdx.x;
	const uint64_t w0 = rev_workgroups<E>(b - a);
	if (t >= w0) {
		t -= w0;
		a = a1;
		b = b1;
		if (t >= rev_workgroups<E>(b - a)) return;
	}
	const uint64_t len = b - a, pairs = len / (2 * T);
	const uint32_t L = t < pairs ? T : (uint32_t)((len - pairs * 2 * T + 1) / 2);
	E *front = data + a + t * T;          // [front, front + L)
	E *back = data + b - t * T - L;       // [back, back + L)
	const uint32_t mf = (uint32_t)((uintptr_t)front / sizeof(E)) % V, mb = (uint32_t)((uintptr_t)back / sizeof(E)) % V;
	Vec vf[kRevVecs], vb[kRevVecs];
	rev_load_side<E>(vf, front, L, mf);
	rev_load_side<E>(vb, back, L, mb);
#pragma unroll
	for (int k = 0; k < kRevVecs; ++k) {
		lds[0][threadIdx.x + k * kRevTh] = vf[k];
		lds[1][threadIdx.x + k * kRevTh] = vb[k];
	}
	__syncthreads();
	rev_store_side<E>(front, L, mf, reinterpret_cast<const E *>(lds[1]), mb);
	rev_store_side<E>(back, L, mb, reinterpret_cast<const E *>(lds[0]), mf);
}

} // namespace msd

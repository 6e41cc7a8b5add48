// msd_regtile.hpp -- what the register-resident leaves share (included by msd_device.hpp): the tile of a workgroup's
// registers on the array's 16-byte grid and the steps of the 2^16 byte counters, both for the u32 leaves:
// count_place16_kernel uses them; merge_place16_kernel, for which load's `at` and the HALVES of the counter steps are
// made, stands on its own text until its conversion has been timed.  Device code only; every function is inlined into its kernel, and an
// opaque copy of the thread index (asm volatile("" : "+v"(..)), explained where it is made) is handed in, never made here.
// What is NOT here, and why ("Register-resident leaves"): a helper is optimised on its own before it is
// inlined, and the kernels that must keep their machine code did not all keep it.  The 8-byte leaves (regpart_kernel,
// leaf17_kernel) share nothing of this file: their element index, loads and LDS -> array stores are written out in them.
// count_place16_kernel's store (which also clears the area) is written out, and so are its fetch-add loop and its LDS
// output loop.
#pragma once

namespace msd {

// ------------------------------------------------------------------------------------------------------------------
// A segment of u32 on the 16-byte grid of its array, in the registers of TH threads: NV 16-byte vectors (VE = 4
// elements each) and NT single tail elements per thread.  The segment starts at any element: `base` is
// the 16-byte boundary at or below it, `off` < VE the elements between the two, and the segment is the grid elements
// [off, tot).  Vector v of thread t = grid elements (v * TH + t) * VE .. + VE - 1, tail element s of thread t = grid
// element NV * TH * VE + s * TH + t.
template <int TH, int NV, int NT> struct RegTile {
	using T = uint32_t;
	static constexpr int VE = Vec16<T>::N, NK = NV * VE + NT;
	static constexpr uint32_t CAP = (uint32_t)TH * NK; // grid elements the tile holds

	// the grid element of register u of thread t
	static __device__ __forceinline__ uint32_t elem(int u, uint32_t t)
	{
		return u < NV * VE ? (uint32_t)((u / VE) * TH * VE) + t * VE + (u % VE) : (uint32_t)(NV * TH * VE + (u - NV * VE) * TH) + t;
	}

	// Grid elements [0, tot), tot >= 1, into rk[at .. at + NK): branch-free and unconditional (a register set written on
	// only some paths becomes a loop-carried value and spills) -- lanes beyond the segment read its last vector / element
	// again.  NTL: nontemporal loads.
	template <bool NTL, int N> static __device__ __forceinline__ void load(T (&rk)[N], const T *base, uint32_t tot, uint32_t t, int at = 0)
	{
		static_assert(NK <= N, "the registers of the tile");
		const uint32_t lastv = (tot - 1u) / VE;
#pragma unroll
		for (int v = 0; v < NV; ++v) {
			T x[VE];
			vec16_unpack<T>(ld16<NTL>(base + min((uint32_t)(v * TH) + t, lastv) * (uint32_t)VE), x);
#pragma unroll
			for (int i = 0; i < VE; ++i) rk[at + v * VE + i] = x[i];
		}
#pragma unroll
		for (int s = 0; s < NT; ++s) {
			const T *e = base + min((uint32_t)(NV * TH * VE + s * TH) + t, tot - 1u);
			if constexpr (NTL) rk[at + NV * VE + s] = __builtin_nontemporal_load(e);
			else rk[at + NV * VE + s] = *e;
		}
	}
};

// ------------------------------------------------------------------------------------------------------------------
// The 2^16 byte counters of the u32 leaves: 2^14 words of four counters in the c16_at layout, in an LDS area of AREA
// words (kC16Cap, msd_count16.hpp) that is the output buffer afterwards.  A key's register carries value | rank << 16 |
// "not an element" << 31, then value | place << 16 | the same bit.  TH threads, NK registers per thread, CH LDS
// operations in flight.

// the whole counter / output area to zero, 16-byte stores (zero, t: the caller's opaque copies)
template <int TH, uint32_t AREA> __device__ __forceinline__ void bc_clear(uint32_t *cw, uint32_t zero, uint32_t t)
{
#pragma unroll
	for (uint32_t j = 0; j < (AREA / 4 + TH - 1) / TH; ++j) {
		const uint32_t q = j * TH + t;
		if (q < AREA / 4) reinterpret_cast<u32x4 *>(cw)[q] = u32x4{ zero, zero, zero, zero };
	}
}

// A thread's WPT counter words at cq, read as 16-byte vectors in HALVES parts of WPT / HALVES words (all WPT beside
// many key registers spill: merge_place16_kernel's way is two halves, twice).
// the sum of their bytes on top of totk; cr is left holding the last part
template <int WPT, int HALVES> __device__ __forceinline__ uint32_t bc_sums(const u32x4 *cq, uint32_t (&cr)[WPT / HALVES], uint32_t totk)
{
	constexpr int HW = WPT / HALVES;
#pragma unroll
	for (int h = 0; h < HALVES; ++h) {
#pragma unroll
		for (int j = 0; j < HW / 4; ++j) {
			const u32x4 q = cq[h * (HW / 4) + j];
			cr[4 * j + 0] = q.x; cr[4 * j + 1] = q.y; cr[4 * j + 2] = q.z; cr[4 * j + 3] = q.w;
		}
#pragma unroll
		for (int j = 0; j < HW; ++j) totk = __builtin_amdgcn_sad_u8(cr[j], 0u, totk);
	}
	return totk;
}
// the words become byte prefixes inside the thread's run (byte_prefix), in place.  HALVES == 1: cr holds the words
// (bc_sums left them there); otherwise every part is read again
template <int WPT, int HALVES> __device__ __forceinline__ void bc_prefixes(u32x4 *cq, uint32_t (&cr)[WPT / HALVES])
{
	constexpr int HW = WPT / HALVES;
	uint32_t run = 0;
#pragma unroll
	for (int h = 0; h < HALVES; ++h) {
		if constexpr (HALVES > 1) {
#pragma unroll
			for (int j = 0; j < HW / 4; ++j) {
				const u32x4 q = cq[h * (HW / 4) + j];
				cr[4 * j + 0] = q.x; cr[4 * j + 1] = q.y; cr[4 * j + 2] = q.z; cr[4 * j + 3] = q.w;
			}
		}
#pragma unroll
		for (int j = 0; j < HW / 4; ++j) {
#pragma unroll
			for (int e = 0; e < 4; ++e) byte_prefix(cr[4 * j + e], run);
			cq[h * (HW / 4) + j] = u32x4{ cr[4 * j + 0], cr[4 * j + 1], cr[4 * j + 2], cr[4 * j + 3] };
		}
		if constexpr (HALVES > 1) __builtin_amdgcn_sched_barrier(0);
	}
}

// place of every key: tbase[owner of its value] + prefix[value] + rank (the place, < 2^15, replaces the rank in bits
// 16..30), CH look-ups in flight
template <int NK, int CH, int WPT> __device__ __forceinline__ void bc_places(uint32_t (&rk)[NK], const uint32_t *tbase, const uint32_t *cw)
{
#pragma unroll
	for (int u0 = 0; u0 < NK; u0 += CH) {
		uint32_t tb[CH], cv[CH];
#pragma unroll
		for (int i = 0; i < CH; ++i) {
			if (u0 + i < NK) {
				const uint32_t wi = (rk[u0 + i] & 0xFFFFu) >> 2;
				tb[i] = tbase[wi / (uint32_t)WPT];
				cv[i] = cw[c16_at(wi)];
			}
		}
#pragma unroll
		for (int i = 0; i < CH; ++i) {
			if (u0 + i < NK) {
				const uint32_t r = rk[u0 + i];
				const uint32_t pl = tb[i] + ((cv[i] >> ((r & 3u) * 8u)) & 0xFFu) + ((r >> 16) & 0xFFu);
				rk[u0 + i] = (r & 0x8000FFFFu) | (pl << 16);
			}
		}
		__builtin_amdgcn_sched_barrier(0);
	}
}

// Work tickets of the u32 leaves (thread 0 only), `take` at a time from ctr->count_ticket3 -- fewer fetch-adds on the one
// ticket word; those in hand live in LDS: wtot[12] the next one, wtot[13] how many.
// (first: the fetch-add's answer + the grid's size -- every workgroup starts with the ticket of its own number)
__device__ __forceinline__ void bc_tickets_in(uint32_t *wtot, uint32_t first, uint32_t take)
{
	wtot[12] = first;
	wtot[13] = take;
}
__device__ __forceinline__ void bc_ticket_next(uint32_t *wtot, uint32_t *nexti)
{
	*nexti = wtot[12];
	wtot[12] += 1;
	wtot[13] -= 1;
}

} // namespace msd

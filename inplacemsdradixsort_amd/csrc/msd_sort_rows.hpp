// msd_sort_rows.hpp -- per-row (batched) sort with positions: msd_sort_rows.
//
// ONE launch sorts all rows.  A GROUP of `LANES` threads owns a row, as in msd_select_rows.hpp: a 1024-thread workgroup, a
// 256-thread workgroup, or one wave of a 256-thread workgroup (four rows per workgroup at a time, each wave with its own
// slice of the LDS and no workgroup barrier).  Groups walk the rows `group, group + groups, ...`.
//
// Per row:
//   1. load: the row is read from memory ONCE, element by element (coalesced over a wave, no alignment needed), into
//      registers in wave-striped order -- wave w, item i, lane l holds element w * nitems * 64 + i * 64 + l -- as
//      fk = code(key) ^ flip (flip = all ones: descending).  Elements past row_len carry the all-ones code: they are
//      the last of the register order, the passes are stable, so they rank last and are never stored.  The position of
//      an element is its load index and costs nothing to make.  A wave requests its next row before it works on this one.
//   2. sort: stable LSD passes of 8 bits, the pass of lds_sort_kernel (msd_device.hpp): the rank of a key among the
//      equal digits of its wave is a match-any from 8 ballots and a popcount of the lower lanes, on top of a per-wave
//      digit counter in LDS; a scan (digit-major, wave-minor) gives every key its place in the exchange buffer.  Digits
//      that are constant over the row (OR / AND of its codes) have no pass.  Keys go through the buffer first; positions
//      follow, as 32-bit words, through the SAME buffer once the keys have been taken out of it: positions take no LDS of
//      their own.  (What bounds a row with positions is the registers of the 1024-lane shape, not the LDS.)
//   3. store: out of the buffer behind the last pass (out of the registers where no digit varies), coalesced, the key
//      decoded in front of the store, the position widened to 64 bits.  The whole row is in registers before its first
//      store: a row may be sorted in place.
// Every global load is predicated on `element < row_len` and every store on `j < row_len`.
#pragma once

#include "msd_select_rows.hpp"

namespace msd {

// keys per lane of the three group shapes: 512 keys for a wave, 4096 for 256 lanes; for 1024 lanes what fits 128 VGPRs
// per lane without scratch -- without positions what lds_sort_kernel takes (Cfg<K, NoVal>::SORT_KPT: 24576 32-bit
// keys, 17408 64-bit keys), with positions (one more register per key) 16384 and 12288
template <typename K, bool IDX, int LANES> struct SortRowsCfg;
template <typename K, bool IDX> struct SortRowsCfg<K, IDX, 64> { static constexpr int BLOCK = 256, KPT = 8; };
template <typename K, bool IDX> struct SortRowsCfg<K, IDX, 256> { static constexpr int BLOCK = 256, KPT = 16; };
template <> struct SortRowsCfg<uint32_t, false, 1024> { static constexpr int BLOCK = 1024, KPT = 24; };
template <> struct SortRowsCfg<uint64_t, false, 1024> { static constexpr int BLOCK = 1024, KPT = 17; };
template <> struct SortRowsCfg<uint32_t, true, 1024> { static constexpr int BLOCK = 1024, KPT = 16; };
template <> struct SortRowsCfg<uint64_t, true, 1024> { static constexpr int BLOCK = 1024, KPT = 12; };

template <typename K, bool IDX, int LANES> constexpr uint64_t sort_rows_cap() { return (uint64_t)LANES * SortRowsCfg<K, IDX, LANES>::KPT; }

// LDS of one group: exchange buffer | per-wave digit counters | digit bases | wave totals of the scan (16) | OR, AND
template <typename K, bool IDX, int LANES> struct SortRowsLds {
	typedef SortRowsCfg<K, IDX, LANES> C;
	static constexpr size_t exch = (size_t)LANES * C::KPT * sizeof(K), wcnt = (size_t)(LANES / 64) * kP * 4, dbase = (size_t)kP * 4, tmp = 16 * 4, orand = 16;
	static constexpr size_t group = exch + wcnt + dbase + tmp + orand; // (every part a multiple of 16 bytes)
	static constexpr size_t bytes = group * (C::BLOCK / LANES);
};

template <typename K, bool IDX, int LANES>
__global__ __launch_bounds__((SortRowsCfg<K, IDX, LANES>::BLOCK)) void sort_rows_kernel(const K *keys, uint64_t rows, uint32_t n, uint64_t stride, K flip,
	KeyCodec<K> codec, K *out_keys, uint64_t *__restrict__ out_idx) // (out_keys may be keys: no __restrict__ on either)
{
	typedef SortRowsCfg<K, IDX, LANES> C;
	typedef SortRowsLds<K, IDX, LANES> L;
	constexpr int KPT = C::KPT, NW = LANES / 64, GROUPS = C::BLOCK / LANES;
	constexpr uint32_t KB = sizeof(K) * 8;
	static_assert((uint64_t)LANES * KPT <= 65536, "a place in the exchange buffer travels in 16 bits");
	extern __shared__ __attribute__((aligned(16))) unsigned char sort_rows_smem[];
	const uint32_t group = GROUPS == 1 ? 0 : threadIdx.x / LANES, t = threadIdx.x % LANES, lane = t & 63u, w = t >> 6;
	unsigned char *const base = sort_rows_smem + (size_t)group * L::group;
	K *const xk = reinterpret_cast<K *>(base);
	uint32_t *const xp = reinterpret_cast<uint32_t *>(base); // (the positions' turn in the exchange buffer)
	uint32_t *const wcnt = reinterpret_cast<uint32_t *>(base + L::exch);
	uint32_t *const dbase = wcnt + NW * kP;
	uint32_t *const tmp = dbase + kP;
	K *const s_or = reinterpret_cast<K *>(tmp + 16);
	uint32_t *const mycnt = wcnt + w * kP;
	const KeyCodec<K> fcodec = codec.flipped(flip);
	const int nitems = (int)((n + LANES - 1) / LANES); // items per lane in use (all rows have the same length)
	const uint32_t wbase = w * (uint32_t)nitems * 64u;
	// item i of this lane is element first + i * 64 of the row, and inside the row iff i < nitems and i * 64 < rem.
	// (Both words pass through an empty asm in every row: the compiler then makes an item's offset and predicate where
	// they are used, from an immediate, instead of keeping KPT loop-invariant offsets and masks alive -- and spilling them.)
	uint32_t first = wbase + lane;
	int32_t rem = (int32_t)n - (int32_t)first;

	auto load_row = [&](uint64_t rr, K(&dst)[KPT]) {
		const K *const src = keys + rr * stride + first;
		const int32_t left = rr < rows ? rem : 0;
#pragma unroll
		for (int i = 0; i < KPT; ++i) {
			dst[i] = (K)~(K)0;
			if (i < nitems && i * 64 < left) dst[i] = fcodec.enc(src[i * 64]);
		}
	};
	const uint64_t r0 = (uint64_t)blockIdx.x * GROUPS + group, rstep = (uint64_t)gridDim.x * GROUPS;
	K kr[KPT], nxt[LANES == 64 ? KPT : 1];
	if constexpr (LANES == 64) load_row(r0, nxt);
	for (uint64_t r = r0; r < rows; r += rstep) {
		asm volatile("" : "+v"(first), "+v"(rem));
		if constexpr (LANES == 64) {
#pragma unroll
			for (int i = 0; i < KPT; ++i) kr[i] = nxt[i];
			load_row(r + rstep, nxt);
		} else
			load_row(r, kr);
		uint32_t pr[IDX ? KPT : 1];
		K k_or = 0, k_and = (K)~(K)0;
#pragma unroll
		for (int i = 0; i < KPT; ++i) {
			if constexpr (IDX) pr[i] = first + (uint32_t)i * 64u;
			if (i < nitems && i * 64 < rem) {
				k_or |= kr[i];
				k_and &= kr[i];
			}
		}
		// ---- which digits vary over the row
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			k_or |= __shfl_xor(k_or, o);
			k_and &= __shfl_xor(k_and, o);
		}
		rows_sync<LANES>(); // (the previous row is done with the LDS)
		if constexpr (NW > 1) {
			if (t == 0) {
				s_or[0] = 0;
				s_or[1] = (K)~(K)0;
			}
			__syncthreads();
			if (lane == 0) {
				if constexpr (sizeof(K) == 4) {
					atomicOr(reinterpret_cast<unsigned int *>(&s_or[0]), (unsigned int)k_or);
					atomicAnd(reinterpret_cast<unsigned int *>(&s_or[1]), (unsigned int)k_and);
				} else {
					atomicOr(reinterpret_cast<unsigned long long *>(&s_or[0]), (unsigned long long)k_or);
					atomicAnd(reinterpret_cast<unsigned long long *>(&s_or[1]), (unsigned long long)k_and);
				}
			}
			__syncthreads();
			k_or = s_or[0];
			k_and = s_or[1];
		}
		const K vary = n ? (K)(k_or ^ k_and) : (K)0;
		K *const ok = out_keys + r * n;
		uint64_t *const ox = IDX ? out_idx + r * n : nullptr;
		if (vary == 0) { // no digit varies (one key, or all keys equal): the row as it was loaded
#pragma unroll
			for (int i = 0; i < KPT; ++i) {
				if (i < nitems && i * 64 < rem) {
					ok[first + (uint32_t)i * 64u] = fcodec.dec(kr[i]);
					if constexpr (IDX) ox[first + (uint32_t)i * 64u] = first + (uint32_t)i * 64u;
				}
			}
			continue;
		}
		// ---- the passes: one per digit that varies, lowest first
		K todo = vary;
		uint32_t rk[(KPT + 1) / 2]; // two 16-bit words per register: the rank in the wave, then the place in the buffer
		do {
			const uint32_t shift = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)__builtin_ctzll((unsigned long long)todo) & ~7u)); // (uniform)
			todo &= (K)~((K)0xFFu << shift);
#pragma unroll 1
			for (uint32_t j = t; j < NW * kP; j += LANES) wcnt[j] = 0;
			rows_sync<LANES>();
#pragma unroll
			for (int i = 0; i < KPT; ++i) {
				if (i < nitems) {
					const uint32_t d = digit_of(kr[i], shift, 0xFFu);
					uint32_t plo = ~0u, phi = ~0u; // match-any: lanes of this wave with the same digit
#pragma unroll
					for (int b = 0; b < 8; ++b) {
						const uint32_t bit = (d >> b) & 1u;
						const uint64_t m = __ballot(bit != 0);
						const uint32_t ext = bit - 1u; // 0 when the bit is set, ~0 otherwise
						plo &= (uint32_t)m ^ ext;
						phi &= (uint32_t)(m >> 32) ^ ext;
					}
					const uint32_t below = popc_below_lane((uint64_t)plo | ((uint64_t)phi << 32));
					const uint32_t old = mycnt[d];                              // same value for all peers
					if (below == 0) mycnt[d] = old + __popc(plo) + __popc(phi); // lowest peer bumps the counter
					const uint32_t rank = old + below;                          // < nitems * 64 <= 1536
					if (i & 1) rk[i / 2] |= rank << 16; else rk[i / 2] = rank;
				}
				__builtin_amdgcn_sched_barrier(0); // keep one item's ballots live at a time
			}
			rows_sync<LANES>();
			// exclusive offsets: digit-major, wave-minor
			if constexpr (NW == 1) {
				uint32_t c4[4], sum = 0;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					c4[j] = wcnt[lane * 4 + j];
					sum += c4[j];
				}
				uint32_t run = wave_incl_scan(sum) - sum;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					dbase[lane * 4 + j] = run;
					run += c4[j];
				}
				rows_sync<LANES>();
			} else {
				uint32_t tot_d = 0;
				if (t < kP) {
#pragma unroll
					for (int ww = 0; ww < NW; ++ww) {
						const uint32_t c = wcnt[ww * kP + t];
						wcnt[ww * kP + t] = tot_d;
						tot_d += c;
					}
				}
				uint32_t gt;
				const uint32_t ex = block_excl_scan256(tot_d, tmp, gt);
				if (t < kP) dbase[t] = ex;
				__syncthreads();
			}
			uint32_t shift2 = shift; // (an item's digit is extracted again -- one instruction -- rather than kept from the ranking loop)
			asm volatile("" : "+s"(shift2));
#pragma unroll
			for (int i = 0; i < KPT; ++i) {
				if (i < nitems) {
					const uint32_t d = digit_of(kr[i], shift2, 0xFFu);
					const uint32_t rank = (i & 1) ? rk[i / 2] >> 16 : rk[i / 2] & 0xFFFFu;
					const uint32_t p = dbase[d] + (NW == 1 ? 0u : mycnt[d]) + rank; // < nitems * LANES
					xk[p] = kr[i];
					if constexpr (IDX) rk[i / 2] = (i & 1) ? (rk[i / 2] & 0xFFFFu) | (p << 16) : (rk[i / 2] & 0xFFFF0000u) | p;
				}
				if constexpr (KPT > 8) __builtin_amdgcn_sched_barrier(0); // (the counters of a few items at a time, not of all)
			}
			rows_sync<LANES>();
			if (todo != 0) { // another pass: the keys back to the registers, in the new order
#pragma unroll
				for (int i = 0; i < KPT; ++i)
					if (i < nitems) kr[i] = xk[first + (uint32_t)i * 64u];
				if constexpr (IDX) { // the positions' turn: every key has left the buffer
					rows_sync<LANES>();
#pragma unroll
					for (int i = 0; i < KPT; ++i)
						if (i < nitems) xp[(i & 1) ? rk[i / 2] >> 16 : rk[i / 2] & 0xFFFFu] = pr[i];
					rows_sync<LANES>();
#pragma unroll
					for (int i = 0; i < KPT; ++i)
						if (i < nitems) pr[i] = xp[first + (uint32_t)i * 64u];
				}
				// (the next pass writes to the buffer behind its own barriers)
			}
		} while (todo != 0);
		// ---- store, out of the buffer
#pragma clang loop unroll(disable) vectorize(disable)
		for (uint32_t j = t; j < n; j += LANES) ok[j] = fcodec.dec(xk[j]);
		if constexpr (IDX) {
			rows_sync<LANES>();
#pragma unroll
			for (int i = 0; i < KPT; ++i)
				if (i < nitems) xp[(i & 1) ? rk[i / 2] >> 16 : rk[i / 2] & 0xFFFFu] = pr[i];
			rows_sync<LANES>();
#pragma clang loop unroll(disable) vectorize(disable)
			for (uint32_t j = t; j < n; j += LANES) ox[j] = xp[j];
		}
	}
}

// ---- rows beyond the kernel's envelope: elementwise kernels around the segment sort (msd_radix.hip, sort_rows_segments)

// contiguous codes of the strided rows: out[r * n + j] = code(keys[r * stride + j]) ^ flip; POS: and idx[r * n + j] = j.
// `out` may be `keys` where stride == n: an element is written where it was read.
template <typename K, bool POS>
__global__ __launch_bounds__(256) void rows_encode_kernel(const K *keys, uint64_t rows, uint64_t n, uint64_t stride, KeyCodec<K> fcodec, K *out,
	uint64_t *__restrict__ idx)
{
	const uint64_t total = rows * n, step = (uint64_t)gridDim.x * 256;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
		const uint64_t r = i / n, j = i - r * n;
		out[i] = fcodec.enc(keys[r * stride + j]);
		if constexpr (POS) idx[i] = j;
	}
}

// 32-bit keys with positions: packed[r * n + j] = (code ^ flip) << 32 | j, sorted as 64-bit keys in the index array itself
__global__ __launch_bounds__(256) void rows_pack_kernel(const uint32_t *__restrict__ keys, uint64_t rows, uint64_t n, uint64_t stride, KeyCodec<uint32_t> fcodec,
	uint64_t *__restrict__ packed)
{
	const uint64_t total = rows * n, step = (uint64_t)gridDim.x * 256;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
		const uint64_t r = i / n, j = i - r * n;
		packed[i] = ((uint64_t)fcodec.enc(keys[r * stride + j]) << 32) | j;
	}
}

template <typename K> __global__ __launch_bounds__(256) void rows_decode_kernel(K *__restrict__ data, uint64_t total, KeyCodec<K> fcodec)
{
	const uint64_t step = (uint64_t)gridDim.x * 256;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) data[i] = fcodec.dec(data[i]);
}

// out_keys = the key of the high half, packed = the low half (an element is rewritten by the thread that read it)
__global__ __launch_bounds__(256) void rows_unpack_kernel(uint64_t *__restrict__ packed, uint64_t total, KeyCodec<uint32_t> fcodec, uint32_t *__restrict__ out_keys)
{
	const uint64_t step = (uint64_t)gridDim.x * 256;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
		const uint64_t e = packed[i];
		out_keys[i] = fcodec.dec((uint32_t)(e >> 32));
		packed[i] = e & 0xFFFFFFFFull;
	}
}

} // namespace msd

// msd_select_rows.hpp -- per-row (batched) top-k: msd_topk_rows.
//
// ONE launch answers all rows.  A GROUP of `LANES` threads owns a row: a whole 1024-thread workgroup (long rows), a
// 256-thread workgroup (medium rows) or one wave of a 256-thread workgroup (short rows: four rows per workgroup at a
// time, each wave with its own slice of the LDS and no workgroup barrier anywhere).  The state of the search that
// SelectState (msd_select.hpp) keeps in global memory lives in registers and LDS here: nothing is read back, and there is
// no workspace.
//
// Per row, on fk = code(key) ^ flip (flip = all ones: largest), exactly the search of msd_select.hpp:
//   1. counting read: the next DIGIT bits of the keys that match the pivot prefix, in LDS bins (sel_count); scan; the
//      bin that holds rank k - 1 becomes the pivot bucket.  Repeated while `below + bucket` does not fit the LDS buffer
//      of BUF elements and key bits are left.
//   2. filter read: keys below the pivot prefix and the keys that match it go to the LDS buffer as (fk, position in the
//      row).  When the bits ran out (more equal keys than the buffer holds) the first `needed` of them are taken.
//   3. bitonic sort of the buffer on (fk, position) -- equal keys therefore come out with ascending positions --
//      padded to a power of two, and k coalesced writes: the key decoded, ascending in the key type's order for both
//      directions.
// Rows start anywhere (alignment of the element type only): a row's head up to the first 16-byte boundary and its tail
// are read element by element, the body in 16-byte loads; a wave's row is loaded element-wise into registers, once.  All loops have trip counts that are uniform in a wave
// (sel_count and the reservations below use wave-wide ballots).
#pragma once

#include "msd_select.hpp"

namespace msd {

constexpr uint64_t kRowsMaxLen = 1ull << 20; // envelope: longest row one workgroup takes
constexpr uint32_t kRowsMaxK = 2048;         // ... and the largest k: the medium variant's whole LDS buffer

// the three group shapes; LANES == 64: a wave per row
template <int LANES> struct RowsCfg;
template <> struct RowsCfg<64> { static constexpr int BLOCK = 256, DIGIT = 8, BUF = 512, U = 2; };
template <> struct RowsCfg<256> { static constexpr int BLOCK = 256, DIGIT = 11, BUF = 2048, U = 4; };
template <> struct RowsCfg<1024> { static constexpr int BLOCK = 1024, DIGIT = 12, BUF = 4096, U = 4; };
constexpr uint64_t kRowsWaveMaxLen = RowsCfg<64>::BUF; // a wave's rows fit its LDS buffer whole
constexpr uint64_t kRowsMidMaxLen = 8192;

// LDS of one group: bins | wave totals (16) + shared words (8) | fk of the buffer | positions
template <typename K, bool IDX, int LANES> struct RowsLds {
	typedef RowsCfg<LANES> C;
	static constexpr size_t bins = (size_t)(1u << C::DIGIT) * 4, words = 24 * 4, codes = (size_t)C::BUF * sizeof(K), pos = IDX ? (size_t)C::BUF * 4 : 0;
	static constexpr size_t group = bins + words + codes + pos; // (every part a multiple of 16 bytes)
	static constexpr size_t bytes = group * (C::BLOCK / LANES);
};

template <int LANES> __device__ __forceinline__ void rows_sync()
{
	if constexpr (LANES == 64) { // a wave's LDS operations complete in order: only the compiler must not move them (and
		// nothing here waits for the loads of the next row, which are in flight)
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	} else
		__syncthreads();
}

// f(bit pattern, position in the row, valid) for every element of the row, all lanes of a wave together
template <typename K, int LANES, int U, typename F> __device__ __forceinline__ void rows_foreach(const K *__restrict__ row, uint32_t n, uint32_t lane, F &&f)
{
	constexpr uint32_t VEC = Vec16<K>::N;
	const uint32_t head = min(n, (uint32_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) / sizeof(K)));
	if (head) { // (uniform in the group; fewer than VEC elements)
		const bool v = lane < head;
		f(v ? row[lane] : (K)0, lane, v);
	}
	const K *body = row + head;
	const uint32_t nvec = (n - head) / VEC;
	for (uint32_t v0 = 0; v0 < nvec; v0 += LANES * U) {
		u32x4 q[U];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint32_t v = v0 + u * LANES + lane;
			q[u] = v < nvec ? reinterpret_cast<const u32x4 *>(body)[v] : u32x4{ 0, 0, 0, 0 };
		}
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint32_t v = v0 + u * LANES + lane;
			const bool valid = v < nvec;
			const uint32_t p = head + v * VEC;
			if constexpr (sizeof(K) == 4) {
				f(q[u].x, p, valid);
				f(q[u].y, p + 1, valid);
				f(q[u].z, p + 2, valid);
				f(q[u].w, p + 3, valid);
			} else {
				f((K)q[u].x | ((K)q[u].y << 32), p, valid);
				f((K)q[u].z | ((K)q[u].w << 32), p + 1, valid);
			}
		}
	}
	const uint32_t done = head + nvec * VEC;
	if (done < n) { // (uniform; fewer than VEC elements)
		const uint32_t i = done + lane;
		const bool v = i < n;
		f(v ? row[i] : (K)0, i, v);
	}
}

// one slot per lane with `take`, reserved with one LDS atomic per wave; 0xFFFFFFFF for the others
__device__ __forceinline__ uint32_t rows_reserve(uint32_t *counter, bool take)
{
	const unsigned long long m = __ballot(take);
	if (m == 0) return 0xFFFFFFFFu;
	const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__builtin_ctzll(m);
	uint32_t base = 0;
	if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
	base = (uint32_t)__shfl((int)base, (int)leader);
	return take ? base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;
}

template <typename K, bool IDX, int LANES>
__global__ __launch_bounds__(RowsCfg<LANES>::BLOCK) void topk_rows_kernel(const K *__restrict__ keys, uint64_t rows, uint32_t n, uint64_t stride, uint32_t k,
	K flip, KeyCodec<K> codec, K *__restrict__ out_keys, uint64_t *__restrict__ out_idx)
{
	typedef RowsCfg<LANES> C;
	typedef RowsLds<K, IDX, LANES> L;
	constexpr uint32_t KB = sizeof(K) * 8, BINS = 1u << C::DIGIT, PER = BINS / LANES, GROUPS = C::BLOCK / LANES, BUF = C::BUF;
	static_assert(PER >= 1 && LANES / 64 <= 16, "bins per lane, wave totals");
	extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
	const uint32_t group = GROUPS == 1 ? 0 : threadIdx.x / LANES, lane = threadIdx.x % LANES;
	unsigned char *const base = rows_smem + (size_t)group * L::group;
	uint32_t *const h = reinterpret_cast<uint32_t *>(base);
	uint32_t *const s_wave = reinterpret_cast<uint32_t *>(base + L::bins);
	uint32_t *const s_word = s_wave + 16; // 0 digit, 1 run, 2 count, 3 cursor of the keys below, 4 cursor of the candidates
	K *const s_fk = reinterpret_cast<K *>(base + L::bins + L::words);
	uint32_t *const s_pos = reinterpret_cast<uint32_t *>(base + L::bins + L::words + L::codes);
	const KeyCodec<K> fcodec = codec.flipped(flip);

	// A wave's row (at most BUF = 64 x RPL keys) stays in registers: lane l holds keys l, l + 64, ...  Element-wise loads,
	// coalesced over the wave, need no alignment; the row is read from memory ONCE, and the next row's loads are issued
	// before this row is worked on.
	constexpr uint32_t RPL = LANES == 64 ? BUF / 64 : 1;
	K cur[RPL], nxt[RPL];
	auto load_row = [&](uint64_t rr, K(&dst)[RPL]) {
#pragma unroll
		for (uint32_t j = 0; j < RPL; ++j) {
			const uint32_t i = j * 64 + lane;
			dst[j] = rr < rows && i < n ? keys[rr * stride + i] : (K)0;
		}
	};
	const uint64_t r0 = (uint64_t)blockIdx.x * GROUPS + group, rstep = (uint64_t)gridDim.x * GROUPS;
	if constexpr (LANES == 64) load_row(r0, nxt);
	for (uint64_t r = r0; r < rows; r += rstep) {
		const K *const row = keys + r * stride;
		if constexpr (LANES == 64) {
#pragma unroll
			for (uint32_t j = 0; j < RPL; ++j) cur[j] = nxt[j];
			load_row(r + rstep, nxt);
		}
		auto each = [&](auto &&f) { // f(bit pattern, position in the row, valid), all lanes of a wave together
			if constexpr (LANES == 64) {
#pragma unroll
				for (uint32_t j = 0; j < RPL; ++j)
					if (j * 64 < n) { // (uniform)
						const uint32_t i = j * 64 + lane;
						f(cur[j], i, i < n);
					}
			} else
				rows_foreach<K, LANES, C::U>(row, n, lane, f);
		};
		uint32_t consumed = 0, below = 0, bucket = n, want = k - 1;
		K prefix = 0;
		// ---- 1. the search
		for (;;) {
			const uint32_t w = min((uint32_t)C::DIGIT, KB - consumed), shift = KB - consumed - w, mask = (1u << w) - 1u;
			rows_sync<LANES>(); // (the previous pass, or the previous row, is done with the bins and the shared words)
			for (uint32_t j = lane; j < BINS; j += LANES) h[j] = 0;
			if (lane < 8) s_word[lane] = 0;
			rows_sync<LANES>();
			each([&](K b, uint32_t, bool valid) {
				const K fk = fcodec.enc(b);
				sel_count(h, (uint32_t)(fk >> shift) & mask, valid && sel_hi(fk, consumed) == prefix);
			});
			rows_sync<LANES>();
			uint32_t c[PER], sum = 0;
#pragma unroll
			for (uint32_t i = 0; i < PER; ++i) {
				c[i] = h[lane * PER + i];
				sum += c[i];
			}
			uint32_t inc = sum; // inclusive scan over the lanes of the group
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
				if ((int)(lane & 63) >= d) inc += t;
			}
			uint32_t excl = inc - sum;
			if constexpr (LANES > 64) {
				if ((lane & 63) == 63) s_wave[lane >> 6] = inc;
				__syncthreads();
				for (uint32_t i = 0; i < (lane >> 6); ++i) excl += s_wave[i];
			}
			if (want >= excl && want < excl + sum) { // exactly one lane: the wanted rank lies in its bins
				uint32_t run = excl, digit = 0, cnt = 0;
				bool found = false;
#pragma unroll
				for (uint32_t i = 0; i < PER; ++i) {
					if (!found && want < run + c[i]) {
						digit = lane * PER + i;
						cnt = c[i];
						found = true;
					}
					if (!found) run += c[i];
				}
				s_word[0] = digit;
				s_word[1] = run; // keys of the bucket in front of the pivot digit
				s_word[2] = cnt;
			}
			rows_sync<LANES>();
			const uint32_t digit = s_word[0], run = s_word[1];
			prefix = (K)((K)(prefix << w) | (K)digit);
			consumed += w;
			below += run;
			want -= run;
			bucket = s_word[2];
			if (below + bucket <= BUF || consumed == KB) break;
		}
		// ---- 2. the filter
		const bool exhausted = below + bucket > BUF; // all candidates are equal: any `needed` of them
		const uint32_t needed = want + 1, take = exhausted ? needed : bucket, m = below + take;
		each([&](K b, uint32_t p, bool valid) {
			const K fk = fcodec.enc(b);
			const K hi = sel_hi(fk, consumed);
			const uint32_t sb = rows_reserve(&s_word[3], valid && hi < prefix);
			const uint32_t sc = rows_reserve(&s_word[4], valid && hi == prefix);
			uint32_t slot = 0xFFFFFFFFu;
			if (sb != 0xFFFFFFFFu)
				slot = sb;
			else if (sc < take)
				slot = below + sc;
			if (slot < BUF) { // (always, for a slot that was given out: below + take <= BUF)
				s_fk[slot] = fk;
				if constexpr (IDX) s_pos[slot] = p;
			}
		});
		// ---- 3. sort (fk, position) and write
		uint32_t P = 1;
		while (P < m) P <<= 1;
		for (uint32_t j = m + lane; j < P; j += LANES) {
			s_fk[j] = (K)~(K)0;
			if constexpr (IDX) s_pos[j] = 0xFFFFFFFFu;
		}
		for (uint32_t size = 2; size <= P; size <<= 1)
			for (uint32_t st = size >> 1; st > 0; st >>= 1) {
				rows_sync<LANES>();
				for (uint32_t t = lane; t < P / 2; t += LANES) {
					const uint32_t i = 2 * t - (t & (st - 1)), j = i + st;
					const bool up = (i & size) == 0;
					const K a = s_fk[i], bb = s_fk[j];
					bool gt = a > bb;
					if constexpr (IDX) {
						const uint32_t pa = s_pos[i], pb = s_pos[j];
						gt = gt || (a == bb && pa > pb);
						if (gt == up) {
							s_pos[i] = pb;
							s_pos[j] = pa;
						}
					}
					if (gt == up) {
						s_fk[i] = bb;
						s_fk[j] = a;
					}
				}
			}
		rows_sync<LANES>();
		K *const ok = out_keys + r * k;
		for (uint32_t j = lane; j < k; j += LANES) {
			const uint32_t o = flip ? k - 1 - j : j; // ascending keys in both directions
			ok[o] = fcodec.dec(s_fk[j]);
			if constexpr (IDX) out_idx[r * k + o] = s_pos[j];
		}
	}
}

} // namespace msd

// msd_select.hpp -- radix select / top-k: read-only passes over the caller's keys ("Select and top-k").
//
// Everything works on fk = key ^ flip (flip = 0: smallest, all ones: largest), so that "largest" is "smallest" with one
// XOR.  The state of the search lives on the device (SelectState) and is advanced by the kernels themselves: the host
// launches   hist(0) pivot(0) hist(1) pivot(1) ... filter   back to back and reads the state once, behind the filter.
//
//   select_hist_kernel   one read of the input: counts the next digit (kSelDigit bits) of the keys whose consumed top
//                        bits equal the pivot prefix, in LDS-private bins, one flush per workgroup.  Lanes of a wave
//                        that share the first lane's digit are counted with ONE LDS add (ballot + popcount), so that
//                        constant / Zipf / zero-upper-half inputs do not serialise on one LDS word.  Pass 0 also
//                        reduces OR(fk) and OR(~fk): the leading bits all keys share are skipped, not counted.
//   select_pivot_kernel  one workgroup: scans the bins, finds the digit whose bucket holds the wanted rank and advances
//                        the state; sets `done` once the pivot bucket fits the candidate buffer or no key bits are left
//                        (later hist/pivot launches then return at once).
//   select_filter_kernel one more read: keys below the pivot prefix go straight to the output, keys that match it to
//                        the candidate buffer.  A workgroup takes 32 KiB of keys per tile into registers, counts its
//                        matches and writes them compacted through an LDS staging buffer that costs one atomic when
//                        it is full; a tile without a match costs none.
//
// Typed keys (msd_topk_keys / msd_select_key; msd_keycodec.hpp) run the same two kernels: what is done to a key's bit pattern
// right behind the load is a policy the kernels take by value (HOW: SelPlain = b ^ flip, SelCoded = the order-preserving code
// of b), and what the filter writes -- keys and loaded rids, or codes and the keys' positions -- is EMIT.  Plain keys keep
// instances of their own (HOW is a template parameter), with the machine code they had before typed keys existed: the body
// stands in the __global__ function itself, only the key transform is called.  select_finish_kernel turns
// the k sorted output elements of a typed call back into keys.
#pragma once

#include "msd_device.hpp"
#include "msd_keycodec.hpp"

namespace msd {

#ifndef MSD_SELECT_DIGIT // (overridable for experiments: 11 or 12)
#define MSD_SELECT_DIGIT 12
#endif
constexpr uint32_t kSelDigit = MSD_SELECT_DIGIT;
constexpr uint32_t kSelBins = 1u << kSelDigit;
constexpr int kSelTh = 256;        // threads of the hist and filter workgroups
constexpr int kSelHistU = 4;       // 16-byte loads in flight per lane in the histogram pass
#ifndef MSD_SELECT_FILTER_U // (overridable for experiments)
#define MSD_SELECT_FILTER_U 8
#endif
#ifndef MSD_SELECT_STAGE_BYTES
#define MSD_SELECT_STAGE_BYTES 8192
#endif
constexpr int kSelFilterU = MSD_SELECT_FILTER_U; // ... in the filter pass: a tile is 256 x 8 x 16 B = 32 KiB of keys
constexpr uint32_t kSelPivotTh = 256;
// (a pass 0 that only skips shared bits skips at least one digit: never more passes than digits in the key)
template <typename K> constexpr uint32_t sel_max_passes() { return (uint32_t)(sizeof(K) * 8 + kSelDigit - 1) / kSelDigit; }

struct SelectState {
	unsigned long long or_all;   // OR of all fk (pass 0)
	unsigned long long nand_all; // OR of all ~fk: AND = ~nand_all
	unsigned long long prefix;   // the pivot's consumed top bits: fk >> (KB - consumed)
	unsigned long long rank;     // wanted rank inside the pivot bucket (0-based)
	unsigned long long below;    // keys strictly below the pivot bucket
	unsigned long long bucket;   // keys in the pivot bucket
	unsigned long long cap;      // candidate capacity (elements)
	unsigned long long out_cursor;  // filter: keys written below the pivot bucket
	unsigned long long cand_cursor; // filter: candidates seen (reserved)
	uint32_t consumed;           // key bits decided so far, from the top (skipped ones included)
	uint32_t skipped;            // leading bits all keys share
	uint32_t passes;             // histogram passes over the input that ran (a pass 0 that only found shared bits included)
	uint32_t done;               // 1: pivot bucket fits the candidate buffer or the bits are used up
	uint32_t exhausted;          // 1: bits used up and the bucket does NOT fit: all candidates are equal to `prefix`
	uint32_t pad[3];
};

template <typename K> __device__ __forceinline__ K sel_hi(K fk, uint32_t consumed)
{
	constexpr uint32_t KB = sizeof(K) * 8;
	return consumed == 0 ? (K)0 : (K)(fk >> (KB - consumed)); // (consumed <= KB: a shift by 0 .. KB - 1)
}

// one key into the LDS bins; `take`: the key matches the pivot prefix.  The lanes whose digit equals the first active
// lane's are counted by that lane alone.
__device__ __forceinline__ void sel_count(uint32_t *h, uint32_t digit, bool take)
{
	const uint32_t d = take ? digit : 0xFFFFFFFFu;
	const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
	const unsigned long long same = __ballot(d == lead);
	if (d == lead) {
		if (lead != 0xFFFFFFFFu && (uint32_t)__builtin_ctzll(same) == (threadIdx.x & 63u)) atomicAdd(&h[lead], (uint32_t)__popcll(same));
	} else if (take)
		atomicAdd(&h[d], 1u);
}

// What a kernel does with a key's bit pattern b, passed by value where `flip` was passed (the first field is `flip` in
// both): enc(b) = the code that is searched on and written, fk(b) = enc(b) ^ flip.
template <typename K> struct SelPlain { // plain unsigned keys: the key is its own code
	K flip;
	__device__ __forceinline__ K enc(K b) const { return b; }
	__device__ __forceinline__ K fk(K b) const { return b ^ flip; }
};
template <typename K> struct SelCoded { // typed keys (msd_topk_keys / msd_select_key): the search runs on the keys' codes
	K flip;
	KeyCodec<K> codec;
	__device__ __forceinline__ K enc(K b) const { return codec.enc(b); }
	__device__ __forceinline__ K fk(K b) const { return codec.flipped(flip).enc(b); }
};

template <typename K, bool FIRST, typename HOW>
__global__ __launch_bounds__(kSelTh) void select_hist_kernel(const K *__restrict__ keys, uint64_t n, HOW how, SelectState *__restrict__ st,
	unsigned long long *__restrict__ bins)
{
	constexpr uint32_t KB = sizeof(K) * 8;
	constexpr int VEC = Vec16<K>::N;
	__shared__ uint32_t h[kSelBins];
	__shared__ unsigned long long s_red[2][kSelTh / 64];
	uint32_t consumed = 0;
	K prefix = 0;
	if constexpr (!FIRST) {
		if (st->done) return;
		consumed = st->consumed;
		prefix = (K)st->prefix;
	}
	const uint32_t w = min(kSelDigit, KB - consumed), shift = KB - consumed - w, mask = (1u << w) - 1u;
	for (uint32_t j = threadIdx.x; j < kSelBins; j += kSelTh) h[j] = 0;
	__syncthreads();
	K acc_or = 0, acc_nand = 0;
	auto one = [&](K key, bool valid) {
		const K fk = how.fk(key);
		if constexpr (FIRST) {
			if (valid) {
				acc_or |= fk;
				acc_nand |= (K)~fk;
			}
			sel_count(h, (uint32_t)(fk >> shift) & mask, valid);
		} else
			sel_count(h, (uint32_t)(fk >> shift) & mask, valid && sel_hi(fk, consumed) == prefix);
	};
	const uint64_t nvec = n / VEC;
	const uint64_t stride = (uint64_t)gridDim.x * kSelTh;
	// (all lanes of a wave stay in the loop together: sel_count uses wave-wide ballots)
	const uint64_t rounds = (nvec + stride * kSelHistU - 1) / (stride * kSelHistU);
	for (uint64_t r = 0; r < rounds; ++r) {
		const uint64_t v0 = r * stride * kSelHistU + (uint64_t)blockIdx.x * kSelTh + threadIdx.x;
		u32x4 q[kSelHistU];
#pragma unroll
		for (int u = 0; u < kSelHistU; ++u) {
			const uint64_t v = v0 + u * stride;
			q[u] = v < nvec ? reinterpret_cast<const u32x4 *>(keys)[v] : u32x4{ 0, 0, 0, 0 };
		}
#pragma unroll
		for (int u = 0; u < kSelHistU; ++u) {
			const bool valid = v0 + u * stride < nvec;
			if constexpr (sizeof(K) == 4) {
				one(q[u].x, valid);
				one(q[u].y, valid);
				one(q[u].z, valid);
				one(q[u].w, valid);
			} else {
				one((K)q[u].x | ((K)q[u].y << 32), valid);
				one((K)q[u].z | ((K)q[u].w << 32), valid);
			}
		}
	}
	if (blockIdx.x == 0) { // the up to VEC - 1 keys behind the last whole vector
		const uint64_t i = nvec * VEC + threadIdx.x;
		if (threadIdx.x < 64) one(i < n ? keys[i] : (K)0, i < n);
	}
	if constexpr (FIRST) {
		unsigned long long o = acc_or, a = acc_nand;
		for (int d = 32; d; d >>= 1) {
			o |= __shfl_xor(o, d);
			a |= __shfl_xor(a, d);
		}
		if ((threadIdx.x & 63) == 0) {
			s_red[0][threadIdx.x >> 6] = o;
			s_red[1][threadIdx.x >> 6] = a;
		}
	}
	__syncthreads();
	for (uint32_t j = threadIdx.x; j < kSelBins; j += kSelTh)
		if (h[j]) atomicAdd(&bins[j], (unsigned long long)h[j]);
	if constexpr (FIRST) {
		if (threadIdx.x == 0) {
			unsigned long long o = 0, a = 0;
			for (int i = 0; i < kSelTh / 64; ++i) {
				o |= s_red[0][i];
				a |= s_red[1][i];
			}
			atomicOr(&st->or_all, o);
			atomicOr(&st->nand_all, a);
		}
	}
}

// Pass `pass` of the search: bins = that pass's histogram.  pass 0 sets the state up (rank: the wanted rank in the whole
// input, 0-based, < n) and skips the leading bits all keys share.
template <typename K>
__global__ __launch_bounds__(kSelPivotTh) void select_pivot_kernel(SelectState *__restrict__ st, const unsigned long long *__restrict__ bins,
	uint32_t pass, uint64_t n, uint64_t rank, uint64_t cap)
{
	constexpr uint32_t KB = sizeof(K) * 8;
	constexpr uint32_t PER = kSelBins / kSelPivotTh;
	__shared__ unsigned long long s_wave[kSelPivotTh / 64];
	__shared__ uint32_t s_stop;
	const uint32_t tid = threadIdx.x;
	if (tid == 0) {
		uint32_t stop = 0;
		if (pass == 0) {
			const K o = (K)st->or_all, a = (K)~st->nand_all, diff = o ^ a;
			const uint32_t skipped = diff ? (uint32_t)(sizeof(K) == 4 ? __clz((uint32_t)diff) : __clzll((unsigned long long)diff)) : KB;
			st->skipped = skipped;
			st->cap = cap;
			st->rank = rank;
			st->below = 0;
			st->bucket = n;
			st->passes = 1;
			st->consumed = 0;
			st->prefix = 0;
			if (skipped >= min(kSelDigit, KB)) { // the first digit is the same in all keys: that histogram says nothing
				st->consumed = skipped;
				st->prefix = sel_hi(o, skipped);
				const uint32_t done = n <= cap || skipped == KB;
				st->done = done;
				st->exhausted = skipped == KB && n > cap;
				stop = 1;
			}
		} else if (st->done)
			stop = 1;
		s_stop = stop;
	}
	__syncthreads();
	if (s_stop) return;
	const uint32_t consumed = st->consumed;
	const uint64_t want = st->rank;
	const uint32_t w = min(kSelDigit, KB - consumed), nb = 1u << w;
	unsigned long long c[PER], sum = 0;
#pragma unroll
	for (uint32_t i = 0; i < PER; ++i) {
		const uint32_t b = tid * PER + i;
		c[i] = b < nb ? bins[b] : 0;
		sum += c[i];
	}
	unsigned long long inc = sum; // inclusive scan over the threads
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long t = __shfl_up(inc, d);
		if ((int)(tid & 63) >= d) inc += t;
	}
	if ((tid & 63) == 63) s_wave[tid >> 6] = inc;
	__syncthreads();
	unsigned long long excl = inc - sum;
	for (uint32_t i = 0; i < (tid >> 6); ++i) excl += s_wave[i];
	if (want >= excl && want < excl + sum) { // exactly one thread: the wanted rank lies in its bins
		unsigned long long run = excl;
		uint32_t digit = 0;
		unsigned long long cnt = 0;
		bool found = false;
#pragma unroll
		for (uint32_t i = 0; i < PER; ++i) {
			if (!found && want < run + c[i]) {
				digit = tid * PER + i;
				cnt = c[i];
				found = true;
			}
			if (!found) run += c[i];
		}
		const uint32_t now = consumed + w;
		st->prefix = (st->prefix << w) | digit;
		st->consumed = now;
		st->rank = want - run;
		st->below += run;
		st->bucket = cnt;
		st->passes = pass + 1;
		st->done = cnt <= cap || now == KB;
		st->exhausted = now == KB && cnt > cap;
	}
}

// `OUT`: top-k (keys below the pivot bucket are written to out_keys); otherwise only the candidates are collected (select).
// Candidates go to cand_keys[0 .. bucket) -- or, when the bits are exhausted (all candidates equal, more of them than the
// buffer holds), the first rank + 1 of them straight to out_keys[below ..).
// Reservations: a tile's matches are counted (one packed scan over the workgroup) and appended, compacted, to a staging
// buffer in LDS (one per destination); a full buffer is written out as whole lines with ONE atomic (one per 16 KiB of
// output keys), the rest at the end of the pass.  Evenly spread keys at small k: one or two atomics per workgroup for
// the whole pass; a tile without a match costs no atomic and one barrier.  (Writing the matches of a dense tile from
// registers straight to their place -- runs of a few keys per store instruction -- took twice as long as the detour.)
//
// Staging bytes per element kind, chosen by the host from k / n (the share of the keys that goes to the output): a pass that
// writes little keeps the buffers small (more workgroups per CU), a pass that writes much makes the runs it reserves long --
// every reservation is one atomic on ONE word, which takes about 88 of them per microsecond.  Both fit the 64 KiB of LDS a
// kernel gets without asking.
constexpr uint32_t kSelStageSmall = MSD_SELECT_STAGE_BYTES, kSelStageLargeCand = 16384, kSelStageLargeBelow = 40960;

// What a selected key is written as (EMIT):
//   kSelRaw     the key itself, and its rid, loaded from `rids`, for tuples: msd_topk_* / msd_select_*
//   kSelCodes   the key's code (typed keys without indices); a finishing pass decodes the k output elements
//   kSelPos     (code, position): the tuple path with the rid GENERATED -- it is the index the rid would be loaded from (64-bit keys)
//   kSelPacked  ONE 64-bit element  code << 32 | position  per 32-bit key (n <= 2^32): candidates and output are u64 keys
//               for the plain sort; the finishing pass splits them
enum { kSelRaw = 0, kSelCodes = 1, kSelPos = 2, kSelPacked = 3 };
template <typename K, int EMIT> struct sel_elem { typedef K type; };
template <> struct sel_elem<uint32_t, kSelPacked> { typedef uint64_t type; };

// `rids` is read for EMIT == kSelRaw tuples only (typed keys: null, positions are generated).
template <typename K, typename V, bool OUT, int EMIT, typename HOW>
__global__ __launch_bounds__(kSelTh) void select_filter_kernel(const K *__restrict__ keys, const uint64_t *__restrict__ rids, uint64_t n, HOW how,
	SelectState *__restrict__ st, typename sel_elem<K, EMIT>::type *__restrict__ out_keys, uint64_t *__restrict__ out_rids,
	typename sel_elem<K, EMIT>::type *__restrict__ cand_keys, uint64_t *__restrict__ cand_rids, uint32_t stage_cand, uint32_t stage_below)
{
	typedef typename sel_elem<K, EMIT>::type E; // the element written for a selected key
	constexpr bool HV = has_val<V>::value;
	static_assert((EMIT == kSelRaw) == std::is_same<HOW, SelPlain<K>>::value, "plain keys have instances of their own");
	static_assert(EMIT != kSelPos || HV, "positions travel as rids");
	static_assert(EMIT != kSelPacked || (!HV && sizeof(K) == 4), "packed elements are for 32-bit keys without rids");
	constexpr uint32_t KB = sizeof(K) * 8;
	constexpr int VEC = Vec16<K>::N, U = kSelFilterU;
	constexpr int KINDS = OUT ? 2 : 1; // 0: candidates, 1: below the pivot bucket
	// staging buffers (elements: stage_cand, stage_below; dynamic LDS): keys of both kinds, then their rids
	extern __shared__ __attribute__((aligned(16))) unsigned char sel_smem[];
	const uint32_t S[2] = { stage_cand, OUT ? stage_below : 0u };
	E *const s_key[2] = { reinterpret_cast<E *>(sel_smem), reinterpret_cast<E *>(sel_smem) + S[0] };
	uint64_t *const s_rid0 = reinterpret_cast<uint64_t *>(reinterpret_cast<E *>(sel_smem) + S[0] + S[1]);
	uint64_t *const s_rid[2] = { s_rid0, s_rid0 + S[0] };
	__shared__ uint32_t s_wave[kSelTh / 64];
	__shared__ unsigned long long s_base;
	const uint32_t consumed = st->consumed;
	const uint64_t below = st->below;
	const bool exhausted = st->exhausted != 0;
	if (exhausted && !OUT) return; // select: the value is the prefix itself
	// the pivot bucket in the fk domain: [lo, lo + span]
	const K lo = consumed == 0 ? (K)0 : (K)((K)st->prefix << (KB - consumed));
	const K span = consumed == 0 ? (K)~(K)0 : (K)(((K)1 << (KB - consumed)) - 1);
	// destinations: [0] candidates, [1] below
	E *const gkey[2] = { exhausted ? out_keys + below : cand_keys, out_keys };
	uint64_t *const grid_[2] = { exhausted ? out_rids + below : cand_rids, out_rids };
	const uint64_t glimit[2] = { exhausted ? st->rank + 1 : min(st->bucket, st->cap), below }; // (nothing is ever written at or behind these)
	unsigned long long *const gcursor[2] = { &st->cand_cursor, &st->out_cursor };
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t fill[2] = { 0, 0 }; // staged elements (the same value in all threads)
	const unsigned long long lt_mask = (1ull << lane) - 1ull;

	// the first `count` staged elements of kind `kd` to their place: one atomic, whole lines
	auto flush = [&](int kd, uint32_t count) {
		__syncthreads(); // (the staged elements are all written)
		if (tid == 0) {
			unsigned long long b = glimit[kd]; // (at or behind the limit: nothing is left to write)
			// (only a pass that stops early looks before it adds: the others need every one of their places)
			if (!(exhausted && kd == 0) || __hip_atomic_load(gcursor[kd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < glimit[kd])
				b = atomicAdd(gcursor[kd], (unsigned long long)count);
			s_base = b;
		}
		__syncthreads();
		const uint64_t base = s_base;
		for (uint32_t i = tid; i < count; i += kSelTh)
			if (base + i < glimit[kd]) {
				gkey[kd][base + i] = s_key[kd][i];
				if constexpr (HV) grid_[kd][base + i] = s_rid[kd][i];
			}
		__syncthreads(); // (the buffer is free again)
	};

	// what is written for the key at `pos`
	auto emit = [&](K key, uint64_t pos) -> E {
		if constexpr (EMIT == kSelPacked)
			return (E)how.enc(key) << 32 | (E)(uint32_t)pos;
		else
			return how.enc(key);
	};
	// 0: candidate, 1: below, 2: neither
	auto kind_of_key = [&](K key) -> int {
		const K fk = how.fk(key);
		if (fk < lo) return OUT ? 1 : 2;
		return (K)(fk - lo) <= span ? 0 : 2;
	};

	const uint64_t nvec = n / VEC;
	const uint64_t tile_vecs = (uint64_t)kSelTh * U;
	const uint64_t ntiles = (nvec + tile_vecs - 1) / tile_vecs;
	for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const uint64_t v0 = t * tile_vecs + tid;
		u32x4 q[U];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint64_t v = v0 + (uint64_t)u * kSelTh;
			q[u] = v < nvec ? reinterpret_cast<const u32x4 *>(keys)[v] : u32x4{ 0, 0, 0, 0 };
		}
		auto key_at = [&](int u, int e) -> K {
			if constexpr (sizeof(K) == 4)
				return e == 0 ? q[u].x : e == 1 ? q[u].y : e == 2 ? q[u].z : q[u].w;
			else
				return e == 0 ? ((K)q[u].x | ((K)q[u].y << 32)) : ((K)q[u].z | ((K)q[u].w << 32));
		};
		auto kind_of = [&](int u, int e) -> int { return v0 + (uint64_t)u * kSelTh < nvec ? kind_of_key(key_at(u, e)) : 2; };
		uint32_t mine = 0; // counts packed as candidates | below << 16 (a tile has 2^14 keys at most: a sum fits 15 bits)
#pragma unroll
		for (int u = 0; u < U; ++u)
#pragma unroll
			for (int e = 0; e < VEC; ++e) {
				const int kd = kind_of(u, e);
				mine += kd == 0 ? 1u : kd == 1 ? 0x10000u : 0u;
			}
		if (!__syncthreads_or(mine != 0)) continue; // the common case at small k: nothing here, no atomic
		uint32_t inc = mine;
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t x = __shfl_up(inc, d);
			if ((int)lane >= d) inc += x;
		}
		if (lane == 63) s_wave[wave] = inc;
		__syncthreads();
		uint32_t excl = inc - mine, total = 0;
		for (uint32_t i = 0; i < kSelTh / 64; ++i) {
			if (i < wave) excl += s_wave[i];
			total += s_wave[i];
		}
		uint64_t rr[HV ? U : 1][HV ? VEC : 1];
		if constexpr (HV) {
#pragma unroll
			for (int u = 0; u < U; ++u)
#pragma unroll
				for (int e = 0; e < VEC; ++e) {
					if constexpr (EMIT == kSelPos) // (the rid is the index it would be loaded from)
						rr[u][e] = (v0 + (uint64_t)u * kSelTh) * VEC + e;
					else
						rr[u][e] = kind_of(u, e) < KINDS ? rids[(v0 + (uint64_t)u * kSelTh) * VEC + e] : 0;
				}
		}
		// The tile's elements of a kind continue the staging buffer at `fill`: they take the places [fill, fill + tot) of
		// which [0, S) exist.  Write what falls inside; a full buffer is written out and the places move down by S, until
		// the tile is through.
#pragma unroll
		for (int kd = 0; kd < KINDS; ++kd) {
			const int32_t tot = (int32_t)(kd ? total >> 16 : total & 0xFFFFu);
			if (tot == 0) continue;
			// (lane 0's exclusive sum is where the wave's elements start; inside the wave they are placed slot by slot)
			const int32_t wex = __builtin_amdgcn_readfirstlane((int)(kd ? excl >> 16 : excl & 0xFFFFu));
			int32_t first = (int32_t)fill[kd];
			for (;;) {
				int32_t at = first + wex;
#pragma unroll
				for (int u = 0; u < U; ++u)
#pragma unroll
					for (int e = 0; e < VEC; ++e) {
						// the lanes with an element of this kind in this register slot write one dense run
						const bool is = kind_of(u, e) == kd;
						const unsigned long long m = __ballot(is);
						if (m == 0) continue;
						const uint32_t p = (uint32_t)(at + (int32_t)__popcll(m & lt_mask));
						if (is && p < S[kd]) { // (places below 0 have been written out already)
							if constexpr (EMIT == kSelRaw)
								s_key[kd][p] = key_at(u, e);
							else
								s_key[kd][p] = emit(key_at(u, e), (v0 + (uint64_t)u * kSelTh) * VEC + e);
							if constexpr (HV) s_rid[kd][p] = rr[u][e];
						}
						at += (int32_t)__popcll(m);
					}
				if (first + tot < (int32_t)S[kd]) break;
				flush(kd, S[kd]);
				first -= (int32_t)S[kd];
				if (first + tot == 0) break;
			}
			fill[kd] = (uint32_t)(first + tot);
		}
		__syncthreads(); // (s_wave is rewritten by the next tile)
	}
#pragma unroll
	for (int kd = 0; kd < KINDS; ++kd)
		if (fill[kd]) flush(kd, fill[kd]);
	// the up to VEC - 1 keys behind the last whole vector: one lane each, one atomic each
	if (blockIdx.x == 0 && tid < (uint32_t)VEC) {
		const uint64_t i = nvec * VEC + tid;
		if (i < n) {
			const K key = keys[i];
			const int kd = kind_of_key(key);
			if (kd < KINDS) {
				const uint64_t p = atomicAdd(gcursor[kd], 1ull);
				if (p < glimit[kd]) {
					gkey[kd][p] = emit(key, i);
					if constexpr (HV && EMIT == kSelPos)
						grid_[kd][p] = i;
					else if constexpr (HV)
						grid_[kd][p] = rids[i];
				}
			}
		}
	}
}

// The finishing pass of typed top-k over the k output elements, element-wise and in place: codes back to keys.
//   PACKED: elems = the caller's index array holding  code << 32 | position : out_keys[i] = dec(high half), and the
//   element itself becomes the position (each lane reads its element before it overwrites it).
//   otherwise: elems = out_keys = the codes (positions, if any, are in their place already).
constexpr int kSelFinishTh = 256;
template <typename K, bool PACKED>
__global__ __launch_bounds__(kSelFinishTh) void select_finish_kernel(uint64_t *__restrict__ packed, K *__restrict__ out_keys, uint64_t k, KeyCodec<K> codec)
{
	for (uint64_t i = (uint64_t)blockIdx.x * kSelFinishTh + threadIdx.x; i < k; i += (uint64_t)gridDim.x * kSelFinishTh) {
		if constexpr (PACKED) {
			const uint64_t p = packed[i];
			out_keys[i] = codec.dec((K)(p >> 32));
			packed[i] = p & 0xFFFFFFFFull;
		} else
			out_keys[i] = codec.dec(out_keys[i]);
	}
}

} // namespace msd

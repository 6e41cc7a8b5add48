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
// Typed keys (msd_topk_keys / msd_select_key; msd_keycodec.hpp): select_hist_codes_kernel and select_filter_codes_kernel are
// the same two kernels with the key turned into its order-preserving code right behind the load -- the bodies are shared
// text (msd_select_hist_body.hpp, msd_select_filter_body.hpp) -- and with the filter writing codes, and the keys' positions,
// instead of keys and loaded rids; select_finish_kernel turns the k sorted output elements back into keys.
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

template <typename K, bool FIRST>
__global__ __launch_bounds__(kSelTh) void select_hist_kernel(const K *__restrict__ keys, uint64_t n, K flip, SelectState *__restrict__ st,
	unsigned long long *__restrict__ bins)
{
#define SEL_FK(b) ((b) ^ flip)
#include "msd_select_hist_body.hpp"
#undef SEL_FK
}

// typed keys (msd_topk_keys / msd_select_key): the search runs on the keys' codes
template <typename K, bool FIRST>
__global__ __launch_bounds__(kSelTh) void select_hist_codes_kernel(const K *__restrict__ keys, uint64_t n, K flip, KeyCodec<K> codec,
	SelectState *__restrict__ st, unsigned long long *__restrict__ bins)
{
	const KeyCodec<K> fcodec = codec.flipped(flip);
#define SEL_FK(b) fcodec.enc(b)
#include "msd_select_hist_body.hpp"
#undef SEL_FK
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

template <typename K, typename V, bool OUT>
__global__ __launch_bounds__(kSelTh) void select_filter_kernel(const K *__restrict__ keys, const uint64_t *__restrict__ rids, uint64_t n, K flip,
	SelectState *__restrict__ st, K *__restrict__ out_keys, uint64_t *__restrict__ out_rids, K *__restrict__ cand_keys,
	uint64_t *__restrict__ cand_rids, uint32_t stage_cand, uint32_t stage_below)
{
	constexpr int EMIT = kSelRaw;
#define SEL_ENC(b) (b)
#define SEL_FK(b) ((b) ^ flip)
#include "msd_select_filter_body.hpp"
#undef SEL_FK
#undef SEL_ENC
}

// typed keys: codes (and positions) are written instead of keys (and rids); no rid array is read
template <typename K, typename V, bool OUT, int EMIT>
__global__ __launch_bounds__(kSelTh) void select_filter_codes_kernel(const K *__restrict__ keys, uint64_t n, K flip, KeyCodec<K> codec,
	SelectState *__restrict__ st, typename sel_elem<K, EMIT>::type *__restrict__ out_keys, uint64_t *__restrict__ out_rids,
	typename sel_elem<K, EMIT>::type *__restrict__ cand_keys, uint64_t *__restrict__ cand_rids, uint32_t stage_cand, uint32_t stage_below)
{
	static_assert(EMIT != kSelRaw, "plain keys: select_filter_kernel");
	const uint64_t *const rids = nullptr; // (positions are generated, nothing is loaded)
	const KeyCodec<K> fcodec = codec.flipped(flip);
#define SEL_ENC(b) codec.enc(b)
#define SEL_FK(b) fcodec.enc(b)
#include "msd_select_filter_body.hpp"
#undef SEL_FK
#undef SEL_ENC
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

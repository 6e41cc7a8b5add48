// msd_front16.hpp -- the top 16 key bits counted once, before the first round (included by msd_device.hpp).
//
// A whole-array keys sort that runs two direct 8-bit rounds (msd_direct.hpp) used to learn the key distribution in
// three instalments, each with a readback of its own: a strided sample for the leading-bit skip, a sample for round 0's
// boundaries, an exact count (direct_hist_kernel, a full read) for round 1's.  The histogram of the top 16 bits of the
// whole array does not change when the array is permuted: counted once, up front, it gives round 0's exact boundaries
// (the 256 row sums), the exact boundaries of all 256 parents of round 1 (the rows), the exact OR / AND of all keys
// and both rounds' verdicts (uneven children, keys in runs) -- one readback tells the host all of it.
//
//   front_init_kernel       clears the summary (a count without the probe: tools/microbench/front_count16.hip)
//   front_probe_kernel      clears the summary; 2^15 sampled keys: is the input hopeless (skewed top digit, runs)?  Then the kernels below return at once
//   front_count16_kernel    the read: 2^16 counters of 16 bits in LDS, flushed as per-workgroup partials
//   front_plan_kernel       partials -> the 2^16 counts, the row sums, round 1's verdicts, the children by route
//   front_top_kernel        row sums -> round 0's verdict
//   front_apply_kernel      the counts into a round's DirectPlans, where direct_sample_kernel / direct_hist_kernel put theirs
#pragma once

namespace msd {

constexpr int kF16Th = 1024;
constexpr uint32_t kF16Words = 1u << 15;                  // counter words: prefixes 2 w (low half) and 2 w + 1 (high half)
constexpr size_t kF16Lds = (size_t)kF16Words * 4 + 64 * 4; // 128 KiB of counters: one workgroup per CU
constexpr int kF16Loads = 8;                              // 16-byte loads in flight per thread

struct FrontSummary { // what the host reads back, once
	uint32_t top[kP];              // keys per top digit: round 0's children, round 1's parents
	unsigned long long v_or, v_and; // OR and AND of all keys
	uint32_t adj_seen, adj_same[2]; // 16-byte vectors looked at / whose first and last key agree in the top ([0]) and the second ([1]) digit
	uint32_t overflow;             // workgroups whose counters do not add up to the keys they read (a 16-bit counter overflowed)
	uint32_t uneven[2];            // direct_declines: round 0's parent ([0]), how many of round 1's parents ([1])
	uint32_t nroute[5];            // round 1's children by route_child's verdict (index = Route + 1)
	uint32_t hopeless;             // front_probe_kernel's verdict: the count was not made
};
static_assert(sizeof(FrontSummary) % 8 == 0, "the OR / AND words take 64-bit atomics");

// the summary cleared (every thread of ONE workgroup calls it)
__device__ __forceinline__ void front_clear(FrontSummary *__restrict__ sum)
{
	uint32_t *w = reinterpret_cast<uint32_t *>(sum);
	for (uint32_t i = threadIdx.x; i < sizeof(FrontSummary) / 4; i += blockDim.x) w[i] = 0;
	__syncthreads();
	if (threadIdx.x == 0) sum->v_and = ~0ull;
}
__global__ __launch_bounds__(256) void front_init_kernel(FrontSummary *__restrict__ sum) { front_clear(sum); }

// A look before the read: one workgroup, kFpRuns runs of 1024 consecutive keys spread evenly over the array (2^15 keys,
// ten microseconds).  An input whose top digit is skewed far beyond what direct placement accepts (some digit has more
// than four times the keys of another: on 128 sampled keys per digit evenly spread keys stay below two), or whose
// neighbours mostly agree in it (sorted, reversed, runs), would be declined after the full read anyway; for those --
// Zipf keys, small key ranges, sorted input -- the read is not made.  What the sample lets through and should not
// have is caught by the exact verdicts behind the read.  All loads are issued before the first key is used: one memory
// latency, not four.  The kernel clears the summary first (it is the first of the front pass).
constexpr int kFpRuns = 32;
template <typename K>
__global__ __launch_bounds__(1024) void front_probe_kernel(const K *__restrict__ keys, uint64_t n, uint32_t shift, FrontSummary *__restrict__ sum)
{
	__shared__ uint32_t h[kP], s_mn, s_mx, s_same;
	const uint32_t tid = threadIdx.x;
	if (tid < kP) h[tid] = 0;
	if (tid == 0) {
		s_mn = 0xFFFFFFFFu;
		s_mx = 0;
		s_same = 0;
	}
	__syncthreads();
	const uint64_t stride = n / 1024 / kFpRuns * 1024; // (n >= 1024: run r < kFpRuns ends at or before n)
	uint32_t same = 0;                                 // per wave (identical in all its lanes)
	K ks[kFpRuns];
#pragma unroll
	for (int u = 0; u < kFpRuns; ++u) ks[u] = keys[(uint64_t)u * stride + tid];
	front_clear(sum); // (under the loads' latency)
#pragma unroll
	for (int u = 0; u < kFpRuns; ++u) {
		const uint32_t d = ((uint32_t)(ks[u] >> shift) >> 8) & 0xFFu;
		atomicAdd(&h[d], 1u);
		same += __popcll(__ballot(d == (uint32_t)__shfl_down((int)d, 1) && (tid & 63) != 63));
	}
	if ((tid & 63) == 0) atomicAdd(&s_same, same);
	__syncthreads();
	if (tid < kP) {
		atomicMin(&s_mn, h[tid]);
		atomicMax(&s_mx, h[tid]);
	}
	__syncthreads();
	if (tid == 0) sum->hopeless = ((uint64_t)s_same * 8u > 63u * 16u * kFpRuns || s_mx > 4u * s_mn) ? 1u : 0u;
}

// Persistent, read-only: workgroup b takes the chunks b, b + grid, ... of kF16Loads x 1024 vectors.  One ds_add per key
// on the word of its prefix ((key >> shift) & 0xFFFF); nothing branches per key.  A counter that passes 65535 carries
// into its neighbour or out of the word: the workgroup's counters then add up to less than the keys it read, which is
// checked once at the flush (count_place_kernel's byte counters play the same trick).  `keys` is 16-byte aligned.
template <typename K>
__global__ __launch_bounds__(kF16Th, 1) void front_count16_kernel(const K *__restrict__ keys, uint64_t n, uint32_t shift,
	uint32_t *__restrict__ partials, FrontSummary *__restrict__ sum)
{
	constexpr int VEC = Vec16<K>::N, U = kF16Loads;
	if (sum->hopeless) return; // (uniform) front_probe_kernel: this input will not take the path
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint32_t *cnt = reinterpret_cast<uint32_t *>(smem);
	uint32_t *tmp = cnt + kF16Words;
	const uint32_t tid = threadIdx.x;
	for (uint32_t i = tid; i < kF16Words / 4; i += kF16Th) reinterpret_cast<u32x4 *>(cnt)[i] = u32x4{ 0, 0, 0, 0 };
	if (tid < 64) tmp[tid] = 0;
	K v_or = 0, v_and = ~(K)0;
	uint32_t nk = 0, seen = 0, same0 = 0, same1 = 0;
	auto prefix_of = [&](K k) { return (uint32_t)(k >> shift) & 0xFFFFu; };
	auto count = [&](K k) {
		v_or |= k;
		v_and &= k;
		const uint32_t p = prefix_of(k);
		atomicAdd(&cnt[p >> 1], (p & 1u) ? 0x10000u : 1u);
	};
	__syncthreads();
	const uint64_t nvec = n / VEC;
	const uint64_t chunk = (uint64_t)U * kF16Th, step = (uint64_t)gridDim.x * chunk;
	for (uint64_t v0 = (uint64_t)blockIdx.x * chunk; v0 < nvec; v0 += step) {
		const K *kp = keys + v0 * VEC;                                  // uniform base, 32-bit offsets, loads branch-free
		const uint32_t rem = nvec - v0 < chunk ? (uint32_t)(nvec - v0) : (uint32_t)chunk; // vectors of this chunk (>= 1)
		K kk[U][VEC];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint32_t vv = min(tid + (uint32_t)u * kF16Th, rem - 1u);
			// (nontemporal: a read-once stream, as in direct_hist_kernel)
			vec16_unpack<K>(__builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(kp + (size_t)vv * VEC)), kk[u]);
		}
#pragma unroll
		for (int u = 0; u < U; ++u) {
			if (tid + (uint32_t)u * kF16Th < rem) {
#pragma unroll
				for (int e = 0; e < VEC; ++e) count(kk[u][e]);
				nk += VEC;
				// first and last key of the vector: equal digits nearly always <=> locally sorted / runs
				const uint32_t x = prefix_of(kk[u][0]) ^ prefix_of(kk[u][VEC - 1]);
				seen += 1;
				same0 += (x >> 8) == 0 ? 1u : 0u;
				same1 += (x & 0xFFu) == 0 ? 1u : 0u;
			}
		}
	}
	if (blockIdx.x == gridDim.x - 1) // the keys behind the last whole vector
		for (uint64_t i = nvec * VEC + tid; i < n; i += kF16Th) {
			count(keys[i]);
			nk += 1;
		}
	__syncthreads();
	// flush: the counter words as they are (front_plan_kernel adds the workgroups up), and their sum
	uint32_t s = 0;
	u32x4 *dst = reinterpret_cast<u32x4 *>(partials + (size_t)blockIdx.x * kF16Words);
	for (uint32_t i = tid; i < kF16Words / 4; i += kF16Th) {
		const u32x4 w = reinterpret_cast<const u32x4 *>(cnt)[i];
		dst[i] = w;
		s += (w.x & 0xFFFFu) + (w.x >> 16) + (w.y & 0xFFFFu) + (w.y >> 16) + (w.z & 0xFFFFu) + (w.z >> 16) + (w.w & 0xFFFFu) + (w.w >> 16);
	}
	unsigned long long o = (unsigned long long)v_or, a = (unsigned long long)v_and | (sizeof(K) == 4 ? 0xFFFFFFFF00000000ull : 0ull);
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		s += (uint32_t)__shfl_xor((int)s, d);
		nk += (uint32_t)__shfl_xor((int)nk, d);
		seen += (uint32_t)__shfl_xor((int)seen, d);
		same0 += (uint32_t)__shfl_xor((int)same0, d);
		same1 += (uint32_t)__shfl_xor((int)same1, d);
		o |= __shfl_xor(o, d);
		a &= __shfl_xor(a, d);
	}
	if ((tid & 63) == 0) {
		atomicAdd(&tmp[0], s);
		atomicAdd(&tmp[1], nk);
		atomicAdd(&tmp[2], seen);
		atomicAdd(&tmp[3], same0);
		atomicAdd(&tmp[4], same1);
		atomicOr(&sum->v_or, o);
		atomicAnd(&sum->v_and, a);
	}
	__syncthreads();
	if (tid == 0) {
		if (tmp[0] != tmp[1]) atomicAdd(&sum->overflow, 1u);
		if (tmp[2]) {
			atomicAdd(&sum->adj_seen, tmp[2]);
			atomicAdd(&sum->adj_same[0], tmp[3]);
			atomicAdd(&sum->adj_same[1], tmp[4]);
		}
	}
}

// min, max and sum of the 256 threads' values (every thread of the workgroup calls it; s: 3 words of LDS, preset by the caller)
__device__ __forceinline__ void front_row_stats(uint32_t c, uint32_t *s)
{
	uint32_t mn = c, mx = c, sm = c;
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		mn = min(mn, (uint32_t)__shfl_xor((int)mn, d));
		mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
		sm += (uint32_t)__shfl_xor((int)sm, d);
	}
	if ((threadIdx.x & 63) == 0) {
		atomicMin(&s[0], mn);
		atomicMax(&s[1], mx);
		atomicAdd(&s[2], sm);
	}
	__syncthreads();
}

// One workgroup per top digit b, one thread per prefix: the partials of `nparts` workgroups added up -> hist[2^16], the
// row's sum (round 1's parent b), direct_plan_kernel's verdict on the row, and where each child would go (route_child
// with the arguments collect_kernel gets in round 1).
__global__ __launch_bounds__(256) void front_plan_kernel(const uint32_t *__restrict__ partials, uint32_t nparts, uint32_t *__restrict__ hist,
	FrontSummary *__restrict__ sum, uint32_t child_bits, uint32_t stop_bits, uint32_t count_bits, uint64_t small_max, uint64_t med_max)
{
	__shared__ uint32_t s_st[3], s_r[5];
	if (sum->hopeless) return; // (uniform) nothing was counted
	const uint32_t t = threadIdx.x, p = blockIdx.x * kP + t, sh = (p & 1u) * 16u;
	if (t == 0) {
		s_st[0] = 0xFFFFFFFFu;
		s_st[1] = 0;
		s_st[2] = 0;
	}
	if (t < 5) s_r[t] = 0;
	__syncthreads();
	const uint32_t *src = partials + (p >> 1);
	uint32_t c = 0;
#pragma unroll 8
	for (uint32_t w = 0; w < nparts; ++w) c += (src[(size_t)w * kF16Words] >> sh) & 0xFFFFu;
	hist[p] = c;
	atomicAdd(&s_r[(int)route_child(c, child_bits, stop_bits, count_bits, small_max, med_max, true) + 1], 1u);
	front_row_stats(c, s_st);
	if (t == 0) {
		sum->top[blockIdx.x] = s_st[2];
		if (direct_declines(s_st[0], s_st[1], sum->adj_same[1], sum->adj_seen)) atomicAdd(&sum->uneven[1], 1u);
	}
	if (t < 5 && s_r[t]) atomicAdd(&sum->nroute[t], s_r[t]);
}

// the row sums are round 0's children
__global__ __launch_bounds__(256) void front_top_kernel(FrontSummary *__restrict__ sum)
{
	__shared__ uint32_t s_st[3];
	if (sum->hopeless) return; // (uniform)
	if (threadIdx.x == 0) {
		s_st[0] = 0xFFFFFFFFu;
		s_st[1] = 0;
		s_st[2] = 0;
	}
	__syncthreads();
	front_row_stats(sum->top[threadIdx.x], s_st);
	if (threadIdx.x == 0 && direct_declines(s_st[0], s_st[1], sum->adj_same[0], sum->adj_seen)) sum->uneven[0] = 1;
}

// One workgroup per parent of a direct round: the exact counts into its plan, in front of direct_plan_kernel.  Round 0
// (rows == 0): the row sums; round 1: parent b's row (all 256 parents are there, in the order of their digit).  The
// adjacent-equal statistic is the whole array's, for the round's digit.
__global__ __launch_bounds__(256) void front_apply_kernel(DirectPlan *__restrict__ plans, const uint32_t *__restrict__ hist,
	const FrontSummary *__restrict__ sum, uint32_t rows)
{
	DirectPlan *plan = plans + blockIdx.x;
	plan->est_cnt[threadIdx.x] = rows ? hist[blockIdx.x * kP + threadIdx.x] : sum->top[threadIdx.x];
	if (threadIdx.x == 0) {
		plan->adj_seen = sum->adj_seen;
		plan->adj_same = sum->adj_same[rows ? 1 : 0];
	}
}

} // namespace msd

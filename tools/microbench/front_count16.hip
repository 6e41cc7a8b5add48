// front_count16_kernel against direct_hist_kernel: the same full read of 2^logn u32 keys, 2^16 counters against 256.
//
//   hipcc --offload-arch=gfx950 -O3 front_count16.hip -o front_count16 && ./front_count16 [logn=30]
//
// Uniform keys (a multiplicative hash of the index).  direct_hist_kernel runs as round 1 launches it: 256 parents, stripes
// of 2^20 keys.  The front pass is timed as the count alone and with front_plan_kernel + front_top_kernel behind it (what
// replaces the histogram read), and checked against the 256-counter histogram.
#include "../../inplacemsdradixsort_amd/csrc/msd_device.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
using namespace msd;

__global__ void fill_kernel(uint32_t *k, size_t n)
{
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull;
		x ^= x >> 29;
		x *= 0xBF58476D1CE4E5B9ull;
		k[i] = (uint32_t)(x >> 32);
	}
}

template <typename F> static void timed(const char *label, size_t bytes, F &&f)
{
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0));
	CK(hipEventCreate(&e1));
	float best = 1e9f, sum = 0;
	const int reps = 8;
	for (int rep = 0; rep < reps + 1; ++rep) {
		CK(hipEventRecord(e0));
		f();
		CK(hipEventRecord(e1));
		CK(hipEventSynchronize(e1));
		CK(hipGetLastError());
		float ms;
		CK(hipEventElapsedTime(&ms, e0, e1));
		if (rep) {
			best = std::min(best, ms);
			sum += ms;
		}
	}
	printf("{\"what\": \"%s\", \"best_ms\": %.4f, \"avg_ms\": %.4f, \"best_TBps\": %.3f}\n", label, best, sum / reps, bytes / best / 1e9);
	fflush(stdout);
}

int main(int argc, char **argv)
{
	const int logn = argc > 1 ? atoi(argv[1]) : 30;
	const size_t n = (size_t)1 << logn;
	hipDeviceProp_t prop;
	CK(hipGetDeviceProperties(&prop, 0));
	const int cus = prop.multiProcessorCount;
	printf("{\"device\": \"%s\", \"cus\": %d, \"logn\": %d}\n", prop.name, cus, logn);
	uint32_t *keys, *partials, *hist;
	FrontSummary *sum;
	CK(hipMalloc(&keys, n * 4));
	CK(hipMalloc(&partials, (size_t)cus * kF16Words * 4));
	CK(hipMalloc(&hist, 65536 * 4));
	CK(hipMalloc(&sum, sizeof(FrontSummary)));
	fill_kernel<<<4096, 256>>>(keys, n);
	CK(hipDeviceSynchronize());

	// direct_hist_kernel as round 1 runs it
	const size_t slen = (size_t)1 << 20, per = n / 256;
	std::vector<Parent> ps;
	std::vector<Stripe> ss;
	for (uint32_t p = 0; p < 256; ++p) {
		Parent pa = { p * per, per, 16, 8, p * 256, (uint32_t)ss.size(), 0, 0 };
		for (size_t b = pa.start; b < pa.start + per; b += slen) ss.push_back({ b, std::min(b + slen, pa.start + per), 0, p, 0, 0, 0 });
		pa.stripe_hi = (uint32_t)ss.size();
		ps.push_back(pa);
	}
	Parent *d_ps;
	Stripe *d_ss;
	DirectPlan *d_plans;
	unsigned long long *vres;
	CK(hipMalloc(&d_ps, ps.size() * sizeof(Parent)));
	CK(hipMalloc(&d_ss, ss.size() * sizeof(Stripe)));
	CK(hipMalloc(&d_plans, 256 * sizeof(DirectPlan)));
	CK(hipMalloc(&vres, 16));
	CK(hipMemcpy(d_ps, ps.data(), ps.size() * sizeof(Parent), hipMemcpyHostToDevice));
	CK(hipMemcpy(d_ss, ss.data(), ss.size() * sizeof(Stripe), hipMemcpyHostToDevice));
	CK(hipMemset(d_plans, 0, 256 * sizeof(DirectPlan)));
	CK(hipMemset(vres, 0, 16));
	timed("direct_hist_kernel", n * 4, [&] { direct_hist_kernel<uint32_t><<<(unsigned)ss.size(), 1024>>>(keys, d_ss, d_ps, d_plans, vres); });

	CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&front_count16_kernel<uint32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16Lds));
	const unsigned grid = (unsigned)std::min<size_t>(cus, std::max<size_t>(1, n >> 18));
	const uint64_t small_max = 24576, med_max = kCountMedMax;
	auto front = [&](bool plan) {
		front_init_kernel<<<1, 256>>>(sum);
		front_count16_kernel<uint32_t><<<grid, kF16Th, kF16Lds>>>(keys, n, 16, partials, sum);
		if (plan) {
			front_plan_kernel<<<256, 256>>>(partials, grid, hist, sum, 16, 0, 16, small_max, med_max);
			front_top_kernel<<<1, 256>>>(sum);
		}
	};
	timed("front_init + front_count16_kernel", n * 4, [&] { front(false); });
	timed("front_init + front_count16_kernel + front_plan_kernel + front_top_kernel", n * 4, [&] { front(true); });

	// the check: row sums against a host count of the top byte
	std::vector<uint32_t> hk(n), hh(65536);
	FrontSummary hs;
	CK(hipMemcpy(hk.data(), keys, n * 4, hipMemcpyDeviceToHost));
	CK(hipMemcpy(hh.data(), hist, 65536 * 4, hipMemcpyDeviceToHost));
	CK(hipMemcpy(&hs, sum, sizeof hs, hipMemcpyDeviceToHost));
	std::vector<uint32_t> ref(65536);
	uint32_t o = 0, a = ~0u;
	for (size_t i = 0; i < n; ++i) {
		ref[hk[i] >> 16]++;
		o |= hk[i];
		a &= hk[i];
	}
	size_t bad = 0;
	for (int i = 0; i < 65536; ++i) bad += ref[i] != hh[i];
	printf("{\"check\": \"hist\", \"mismatches\": %zu, \"or_ok\": %d, \"and_ok\": %d, \"overflow\": %u, \"uneven0\": %u, \"uneven1\": %u, "
	       "\"adj_seen\": %u, \"adj_same\": [%u, %u], \"nroute\": [%u, %u, %u, %u, %u]}\n",
	       bad, (uint32_t)hs.v_or == o, (uint32_t)hs.v_and == a, hs.overflow, hs.uneven[0], hs.uneven[1], hs.adj_seen, hs.adj_same[0],
	       hs.adj_same[1], hs.nroute[0], hs.nroute[1], hs.nroute[2], hs.nroute[3], hs.nroute[4]);
	return bad != 0;
}

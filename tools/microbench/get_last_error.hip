// get_last_error.hip -- what one hipGetLastError() costs the host (the runtime initialised, a kernel launched before), beside
// what the enqueue of an empty kernel costs it: the price of checking every launch.
//   hipcc --offload-arch=gfx950 -O2 get_last_error.hip -o get_last_error && ./get_last_error
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
__global__ void k(int *p) { if (p) *p = 1; }
int main()
{
	int *d = nullptr;
	if (hipMalloc(&d, 4) != hipSuccess) return 1;
	hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, nullptr, d);
	if (hipDeviceSynchronize() != hipSuccess) return 1;
	for (int rep = 0; rep < 3; ++rep) {
		const int N = 1000000;
		unsigned bad = 0;
		auto t0 = std::chrono::steady_clock::now();
		for (int i = 0; i < N; ++i) bad += hipGetLastError() != hipSuccess;
		auto t1 = std::chrono::steady_clock::now();
		printf("hipGetLastError: %.1f ns per call (%u errors)\n", std::chrono::duration<double, std::nano>(t1 - t0).count() / N, bad);
		const int M = 20000;
		t0 = std::chrono::steady_clock::now();
		for (int i = 0; i < M; ++i) hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, nullptr, d);
		t1 = std::chrono::steady_clock::now();
		if (hipDeviceSynchronize() != hipSuccess) return 1;
		printf("launch (enqueue only): %.1f ns per call\n", std::chrono::duration<double, std::nano>(t1 - t0).count() / M);
	}
	(void)hipFree(d);
	return 0;
}

// msd_select_hist_body.hpp -- the body of select_hist_kernel and select_hist_codes_kernel (msd_select.hpp), included
// into both: the two kernels are the same text, so that the kernel for plain keys compiles to exactly the machine code
// it had before typed keys existed.  In scope: K, FIRST, keys, n, flip, st, bins; SEL_FK(b) = code of the bit pattern b ^ flip
// (plain keys: b ^ flip).
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
		const K fk = SEL_FK(key);
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

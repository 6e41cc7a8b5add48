// msd_select_filter_body.hpp -- the body of select_filter_kernel and select_filter_codes_kernel (msd_select.hpp), included
// into both (see msd_select_hist_body.hpp for why).  In scope: K, V, OUT, EMIT, keys, rids, n, flip, st, out_keys, out_rids,
// cand_keys, cand_rids, stage_cand, stage_below; SEL_ENC(b) = the code of the bit pattern b (plain keys: b itself), SEL_FK(b) = that code ^ flip.
	typedef typename sel_elem<K, EMIT>::type E; // the element written for a selected key
	constexpr bool HV = has_val<V>::value;
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
		// what is written for the key at `pos`
		auto emit = [&](K key, uint64_t pos) -> E {
			if constexpr (EMIT == kSelPacked)
				return (E)SEL_ENC(key) << 32 | (E)(uint32_t)pos;
			else
				return SEL_ENC(key);
		};
		auto key_at = [&](int u, int e) -> K {
			if constexpr (sizeof(K) == 4)
				return e == 0 ? q[u].x : e == 1 ? q[u].y : e == 2 ? q[u].z : q[u].w;
			else
				return e == 0 ? ((K)q[u].x | ((K)q[u].y << 32)) : ((K)q[u].z | ((K)q[u].w << 32));
		};
		// 0: candidate, 1: below, 2: neither
		auto kind_of = [&](int u, int e) -> int {
			if (v0 + (uint64_t)u * kSelTh >= nvec) return 2;
			const K fk = SEL_FK(key_at(u, e));
			if (fk < lo) return OUT ? 1 : 2;
			return (K)(fk - lo) <= span ? 0 : 2;
		};
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
			const K fk = SEL_FK(key);
			const int kd = fk < lo ? 1 : (K)(fk - lo) <= span ? 0 : 2;
			if (kd < KINDS) {
				const uint64_t p = atomicAdd(gcursor[kd], 1ull);
				if (p < glimit[kd]) {
					if constexpr (EMIT == kSelPacked)
						gkey[kd][p] = (E)SEL_ENC(key) << 32 | (E)(uint32_t)i;
					else
						gkey[kd][p] = SEL_ENC(key);
					if constexpr (HV && EMIT == kSelPos)
						grid_[kd][p] = i;
					else if constexpr (HV)
						grid_[kd][p] = rids[i];
				}
			}
		}
	}

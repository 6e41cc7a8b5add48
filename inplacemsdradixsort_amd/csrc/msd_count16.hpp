// msd_count16.hpp -- the one-pass counting leaf for the case the planner aims at: u32 keys, 16 open bits (or a few
// less: the values are then spread over the 2^16 counters by a shift), a segment that fits the registers of one
// 512-thread workgroup (included by msd_device.hpp).
//
// Same algorithm as count_place_kernel (2^16 byte counters in LDS, the fetch-add's return value is the key's
// rank among equal keys, place = base[owner of the value] + prefix[value] + rank, keys are re-generated as
// prefix | value), rebuilt around what profiles/r02_stamps_count_place_before.json showed: 17 four-byte
// loads and 17 four-byte stores per thread cost 12 of a segment's 37 thousand cycles (vector memory
// instructions issue at a fixed rate, whatever their width), the counters were read three times, and
// every conditional fetch-add waited for the one before it.  Here:
//   * global loads and stores are 16 bytes per lane: the segment is handled on the 16-byte grid of the array
//     (a segment starts at any element; the up to three elements in front of it are masked), the re-generated
//     keys are staged in LDS relative to that grid and leave as whole vectors;
//   * a thread's 32 counter words (128 values) are read ONCE (ds_read_b128), summed, scanned across the
//     workgroup and turned into byte prefixes in registers, then written back (layout: four words of padding
//     per 64 words, which keeps 16-byte alignment and makes the b128 accesses bank-conflict free);
//   * fetch-adds, position look-ups and output writes are branch-free and issued back to back; an element
//     outside the segment uses the lane's junk words;
//   * 512-thread workgroups, two per CU, 128 VGPRs;
//   * two sets of key registers: the next segment's keys are requested as soon as the counter registers are dead,
//     in front of the position look-ups and the LDS output phase; the store phase leaves the counters clear.
// What this kernel does not take -- other bit counts, longer segments, a thread with more than 255 keys, an
// overflowing byte -- is queued untouched for count_place_kernel / count_walk_kernel.
#pragma once

namespace msd {

#ifndef MSD_C16_TH // (overridable for experiments)
#define MSD_C16_TH 512
#endif
constexpr int kC16Th = MSD_C16_TH;
#ifndef MSD_C16_EARLY_TICKET // work tickets drawn a segment ahead
#define MSD_C16_EARLY_TICKET 1
#endif
#ifndef MSD_C16_SV // 16-byte vectors of the store phase in flight per thread
#define MSD_C16_SV 8
#endif
// cache policy (overridable for experiments, tools/nt_variants.py): bit 0 nontemporal key loads (prefetch), bit 1
// nontemporal full-vector stores (put); a segment is read once and written once per launch.  2^30 keys, per launch
// (profiles/nt_variants.jsonl): plain 1765 us, loads 1756 (inside the plain build's range of 20), stores 1726, both 1747.
#ifndef MSD_C16_NT
#define MSD_C16_NT 2
#endif
constexpr bool kC16NtLoad = (MSD_C16_NT & 1) != 0, kC16NtStore = (MSD_C16_NT & 2) != 0;
constexpr int kC16Vec = 4096 / kC16Th;                      // 16-byte vectors per thread: TH * NV * 4 = 16384 elements
constexpr int kC16Tail = 1024 / kC16Th;                      // + scalar elements per thread behind them
constexpr uint32_t kC16Cap = kC16Th * (kC16Vec * 4 + kC16Tail); // 17408 elements on the 16-byte grid
constexpr uint32_t kC16MinBits = 9;                          // fewer open bits: more than 255 copies per value are the rule (byte counters)
constexpr uint32_t kC16Words = 16384;                        // counter words (4 byte counters each)
constexpr uint32_t kC16CwWords = kC16Words + (kC16Words >> 6) * 4; // with 4 words of padding per 64
static_assert(kC16CwWords == kC16Cap, "counters and output buffer share one LDS area");
// [counters | output buffer][per-thread bases][junk words: 64 counters + 64 keys][wave totals, flags]
constexpr size_t kC16Lds = (size_t)kC16Cap * 4 + kC16Th * 4 + 128 * 4 + 128;
__device__ __forceinline__ uint32_t c16_at(uint32_t w) { return w + ((w >> 6) << 2); }

template <bool BIG> // BIG: the array exceeds the memory-side cache, MSD_C16_NT applies (kStreamMinBytes, msd_device.hpp)
__global__ __launch_bounds__(kC16Th, (kC16Th >= 1024 ? 8 : 4)) void count_place16_kernel(uint32_t *__restrict__ keys,
	const Segment *__restrict__ segs, uint32_t nsegs, Segment *__restrict__ rejected, Counters *__restrict__ ctr,
	uint64_t n_total)
{
	constexpr int TH = kC16Th, NV = kC16Vec, NT = kC16Tail, NK = NV * 4 + NT;
	constexpr int CH = TH >= 1024 ? 4 : 8; // fetch-adds / look-ups in flight per thread (register budget: 64 or 128 VGPRs)
	constexpr bool NTL = BIG && kC16NtLoad, NTS = BIG && kC16NtStore;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint32_t *cw = reinterpret_cast<uint32_t *>(smem);  // packed byte counters (padded layout) ...
	uint32_t *out = reinterpret_cast<uint32_t *>(smem); // ... later the output buffer, on the array's 16-byte grid
	uint32_t *tbase = cw + kC16Cap;                     // per-thread output base
	uint32_t *junkc = tbase + TH;                       // per-lane junk counter / junk output word
	uint32_t *junko = junkc + 64;
	uint32_t *wtot = junko + 64;                        // 8 wave totals
	uint32_t *nexti = wtot + 9, *hi_l = wtot + 10, *crowded = wtot + 11;
	const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	if (blockIdx.x >= nsegs) return;
	// tickets (only thread 0 uses them): two at a time when there are many segments -- fewer fetch-adds on the one
	// ticket word; those in hand live in LDS, wtot[12] next / wtot[13] how many.  A workgroup that ends may hold
	// tickets it does not use: they are later ones than the one that ended it, so none is below nsegs.
	constexpr bool kEarlyTicket = MSD_C16_EARLY_TICKET;
	const uint32_t ntake = nsegs > 64u * gridDim.x ? 2u : 1u;
	if (tid == 0) {
		wtot[13] = 0;
		if (kEarlyTicket) {
			wtot[12] = atomicAdd(&ctr->count_ticket3, ntake) + gridDim.x;
			wtot[13] = ntake;
		}
	}
	// segment descriptors are the same in every lane: keep them in scalar registers (loaded through vector
	// memory or LDS they would make every address a per-lane 64-bit computation)
	auto uniform = [](Segment g) -> Segment {
		Segment u;
		// (the builtin returns a signed int: without the cast to uint32_t a low word >= 2^31 sign-extends into the high
		// word -- element offsets that large exist only in arrays of more than 2^31 keys.  THIS was round 2's GPU fault
		// at 2^32 keys: `keys + start` pointed 16 GiB below the array and the segment's first 16-byte load faulted.)
		auto rfl = [](uint32_t x) -> uint64_t { return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(x); };
		u.start = rfl((uint32_t)g.start) | (rfl((uint32_t)(g.start >> 32)) << 32);
		u.count = rfl((uint32_t)g.count) | (rfl((uint32_t)(g.count >> 32)) << 32);
		u.bits = (uint32_t)rfl(g.bits);
		u.pad = 0;
		return u;
	};
	Segment sg = uniform(segs[blockIdx.x]);

	// TWO register sets of one register per key: the key (prefetched) -> value | rank << 16 -> value | place << 16 -> dead.
	// While one set carries a segment through its position look-ups and the LDS output phase, the other already
	// receives the next segment's keys (requested as soon as the 32 counter registers are dead); the loop body exists
	// twice with the sets' roles swapped, so no register is copied and no wait sits between the two segments.
	uint32_t rka[NK], rkb[NK];
	// the segment's elements on the 16-byte grid: vector v of thread t = grid elements (v * TH + t) * 4 .. + 3,
	// tail element s of thread t = grid element NV * TH * 4 + s * TH + t.  Branch-free and unconditional (a register
	// set written on only some paths becomes a loop-carried value and spills): lanes beyond the segment re-read its
	// last vector / element; of a segment this kernel will not take, and when there is no next segment (!live), only
	// the first vector is read.  Addresses come from an opaque copy of the thread index (not hoisted out of the loop).
	auto prefetch = [&](uint32_t (&rk)[NK], const Segment &g, bool live) __attribute__((always_inline)) {
		uint32_t tp = tid;
		asm volatile("" : "+v"(tp));
		const uint32_t off = (uint32_t)(g.start & 3u);
		const uint32_t *base = keys + (g.start - off);
		const uint64_t tot = g.count + off;
		// (the only other access of this kernel that can leave the array: the 16-byte vector holding the LAST elements of
		// the array's last segment may extend up to 12 bytes behind the allocation -- such a segment is not taken, n_total
		// is the array's length)
		const bool take = live && g.bits >= kC16MinBits && g.bits <= 16 && tot <= (uint64_t)kC16Cap && ((g.start - off + tot + 3) & ~3ull) <= n_total;
		const uint32_t totc = take ? (uint32_t)tot : 1u;
		const uint32_t lastv = (totc - 1u) >> 2;
#pragma unroll
		for (int v = 0; v < NV; ++v) {
			const u32x4 q = ld16<NTL>(base + min((uint32_t)(v * TH) + tp, lastv) * 4u);
			rk[v * 4 + 0] = q.x; rk[v * 4 + 1] = q.y; rk[v * 4 + 2] = q.z; rk[v * 4 + 3] = q.w;
		}
#pragma unroll
		for (int s = 0; s < NT; ++s) {
			const uint32_t *e = base + min((uint32_t)(NV * TH * 4 + s * TH) + tp, totc - 1u);
			if constexpr (NTL) rk[NV * 4 + s] = __builtin_nontemporal_load(e);
			else rk[NV * 4 + s] = *e;
		}
	};
	// the whole counter / output area to zero (16-byte stores): before the first segment and behind a rejected one;
	// behind a sorted segment the store phase leaves the area cleared
	auto clear_all = [&]() __attribute__((always_inline)) {
		uint32_t zero = 0, tc = tid;
		asm volatile("" : "+v"(zero), "+v"(tc));
#pragma unroll
		for (uint32_t j = 0; j < (kC16Cap / 4 + TH - 1) / TH; ++j) {
			const uint32_t q = j * TH + tc;
			if (q < kC16Cap / 4) reinterpret_cast<u32x4 *>(cw)[q] = u32x4{ zero, zero, zero, zero };
		}
	};
	prefetch(rka, sg, true);
	clear_all();
	__syncthreads();
	MSD_STAMP_DECL(2);
	MSD_STAMP_START();
	// one segment: its keys are in rk (requested during the segment before), the next segment's go to rn.
	// Returns false behind the workgroup's last segment.
	auto segment = [&](uint32_t (&rk)[NK], uint32_t (&rn)[NK]) __attribute__((always_inline)) -> bool {
		const uint32_t off = (uint32_t)(sg.start & 3u);
		const uint32_t tot = (uint32_t)min(sg.count + off, (uint64_t)0xFFFFFFFFu), n = tot - off;
		const bool fits = sg.bits >= kC16MinBits && sg.bits <= 16 && sg.count + off <= (uint64_t)kC16Cap && ((sg.start + sg.count + 3) & ~3ull) <= n_total;
		const uint32_t vsh = 16u - (fits ? sg.bits : 16u); // a value of b < 16 bits is counted as value << (16 - b): every thread's counters get their share
		uint32_t *segb = keys + (sg.start - off); // 16-byte aligned
		MSD_STAMP(9);
		MSD_STAMP_TICK(11);
		// (loop invariants of one use per segment -- a vector of zeros, a lane's slot in the wave totals -- are made
		// opaque: hoisted out of the loop they are spilled, and their reload waits for the stores in flight)
		uint32_t zero = 0, tq = tid;
		asm volatile("" : "+v"(zero), "+v"(tq));
		// (the counters are clear: the store phase of the segment before, or clear_all, left them so)
		if (tid == 0) {
			if (!kEarlyTicket && wtot[13] == 0) {
				wtot[12] = atomicAdd(&ctr->count_ticket3, ntake) + gridDim.x;
				wtot[13] = ntake;
			}
			*nexti = wtot[12]; // (a ticket is in hand: drawn before the loop or during the segment before)
			wtot[12] += 1;
			wtot[13] -= 1;
			*crowded = 0;
			const uint32_t k0 = off == 0 ? rk[0] : off == 1 ? rk[1] : off == 2 ? rk[2] : rk[3]; // first key
			*hi_l = k0 & ~((1u << sg.bits) - 1u); // common prefix of the whole segment
		}
		MSD_STAMP(0); // ticket, first key
		MSD_STAMP(1);
		// ---- one fetch-add per key: value (low 16 bits) | rank among equal keys << 16; elements outside the segment
		// bump the lane's junk counter
		if (fits) {
			// (eight fetch-adds in flight at a time)
#pragma unroll
			for (int u0 = 0; u0 < NK; u0 += CH) {
				uint32_t old[CH];
#pragma unroll
				for (int i = 0; i < CH; ++i) {
					const int u = u0 + i;
					if (u < NK) {
						const uint32_t el = u < NV * 4 ? (uint32_t)((u / 4) * TH * 4) + tid * 4 + (u % 4) : (uint32_t)(NV * TH * 4 + (u - NV * 4) * TH) + tid;
						const uint32_t val = (rk[u] << vsh) & 0xFFFFu; // (fewer than 16 open bits: spread over the counters, order kept)
						const bool in = el >= off && el < tot;
						const uint32_t a = in ? c16_at(val >> 2) : (uint32_t)(junkc - cw) + lane; // word index from cw
						old[i] = atomicAdd(cw + a, 1u << ((val & 3u) * 8u));
						rk[u] = val | (in ? 0u : 0x80000000u);
					}
				}
#pragma unroll
				for (int i = 0; i < CH; ++i) {
					const int u = u0 + i;
					if (u < NK) rk[u] |= ((old[i] >> ((rk[u] & 3u) * 8u)) & 0xFFu) << 16;
				}
				__builtin_amdgcn_sched_barrier(0);
			}
		}
		MSD_STAMP(2); // fetch-adds (incl. the wait for the keys)
		__syncthreads();
		MSD_STAMP(3);
		const uint32_t nxt = (uint32_t)__builtin_amdgcn_readfirstlane(*nexti), hi = (uint32_t)__builtin_amdgcn_readfirstlane(*hi_l);
		const bool more = nxt < nsegs;
		// the next segment's descriptor travels during the counter phases (loaded where its keys are prefetched,
		// its whole memory latency would sit in front of that prefetch)
		const Segment nraw = segs[more ? nxt : blockIdx.x];
		// thread 0 draws the tickets of the segments after the next one here, where nothing waits for them: the
		// fetch-add's answer is stored behind the prefetch (drawn at the segment's start, every wave stood at the
		// first barrier for the round trip to the one ticket word)
		const bool refill = kEarlyTicket && tid == 0 && wtot[13] == 0;
		uint32_t drawn = 0;
		if (refill) drawn = atomicAdd(&ctr->count_ticket3, ntake);
		// ---- the thread's 32 counter words, once: byte sums -> scan over the workgroup -> byte prefixes
		constexpr int WPT = (int)(kC16Words / TH); // counter words per thread (32 or 16: whole 16-byte vectors, inside one 64-word group)
		u32x4 *cq = reinterpret_cast<u32x4 *>(cw + c16_at(tid * (uint32_t)WPT)); // (16-byte aligned)
		uint32_t cr[WPT];
		uint32_t totk = 0;
		if (fits) {
#pragma unroll
			for (int j = 0; j < WPT / 4; ++j) {
				const u32x4 q = cq[j];
				cr[4 * j + 0] = q.x; cr[4 * j + 1] = q.y; cr[4 * j + 2] = q.z; cr[4 * j + 3] = q.w;
			}
#pragma unroll
			for (int j = 0; j < WPT; ++j) totk = __builtin_amdgcn_sad_u8(cr[j], 0u, totk);
		}
		if (totk > 255u) *crowded = 1; // (a byte prefix would not fit)
		const uint32_t inc = wave_incl_scan(totk);
		if ((tq & 63u) == 63u) wtot[tq >> 6] = inc;
		MSD_STAMP(4); // counters read + byte sums + wave scan
		__syncthreads();
		uint32_t pos = inc - totk, all = 0;
#pragma unroll
		for (uint32_t ww = 0; ww < TH / 64; ++ww) {
			const uint32_t t = wtot[ww];
			if (ww < w) pos += t;
			all += t;
		}
		// a byte that overflowed carried into its neighbour: the sum of all bytes then falls short of n
		const bool ok = fits && all == n && *crowded == 0;
		MSD_STAMP(5);
		if (ok) {
			uint32_t run = 0;
#pragma unroll
			for (int j = 0; j < WPT / 4; ++j) {
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const uint32_t x = cr[4 * j + e], y = x * 0x01010101u; // bytes of y: inclusive sums inside the word
					cr[4 * j + e] = (y - x) + run * 0x01010101u;
					run += y >> 24;
				}
				cq[j] = u32x4{ cr[4 * j + 0], cr[4 * j + 1], cr[4 * j + 2], cr[4 * j + 3] };
			}
			tbase[tid] = pos + off; // (output positions are on the array's 16-byte grid)
		} else if (tid == 0)
			rejected[atomicAdd(&ctr->nslow16, 1u)] = sg; // untouched
		// ---- the counter registers are dead: the next segment's keys are requested HERE (segments are disjoint and
		// handed out by ticket, nobody writes that one before this workgroup does), so that the look-ups, the LDS
		// output phase and their barriers run under the loads' latency and this segment's stores queue behind
		// nothing.  (The scheduler must not lift the loads into the counter phases: 32 more live registers.)
		__builtin_amdgcn_sched_barrier(0);
		const Segment nsg = uniform(nraw);
		prefetch(rn, nsg, more);
		__builtin_amdgcn_sched_barrier(0);
		if (refill) {
			wtot[12] = drawn + gridDim.x;
			wtot[13] = ntake;
		}
		if (ok) {
			MSD_STAMP(6); // byte prefixes, prefetch issue
			__syncthreads();
			// ---- place of every key: base[owner of its value] + prefix[value] + rank
			// (the place, < 2^15, replaces the rank in bits 16..30)
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
			MSD_STAMP(7); // positions
			__syncthreads(); // counters are dead: the area is the output buffer now
#pragma unroll
			for (int u = 0; u < NK; ++u) {
				uint32_t *o = (rk[u] >> 31) ? junko + lane : out + ((rk[u] >> 16) & 0x7FFFu);
				*o = hi | ((rk[u] & 0xFFFFu) >> vsh);
			}
			__syncthreads();
			MSD_STAMP(8); // output into LDS
			// ---- LDS -> array.  Whole vectors inside [off, tot) leave as 16-byte stores, the partial vectors at both
			// ends element-wise, each by the thread that holds the vector; behind its read every vector of the area is
			// set to zero: the next segment finds its counters clear (no clear phase, one barrier less per segment).
			const uint32_t v_first = off ? 1u : 0u, v_end = tot >> 2; // full vectors: [v_first, v_end)
			auto put = [&](uint32_t q, const u32x4 &t) __attribute__((always_inline)) {
				if (q >= v_first && q < v_end)
					st16<NTS>(reinterpret_cast<u32x4 *>(segb) + q, t);
				else if (q == v_end || q < v_first) { // (one or two vectors per segment)
					const uint32_t e0 = q << 2;
					if (e0 + 0 >= off && e0 + 0 < tot) segb[e0 + 0] = t.x;
					if (e0 + 1 >= off && e0 + 1 < tot) segb[e0 + 1] = t.y;
					if (e0 + 2 >= off && e0 + 2 < tot) segb[e0 + 2] = t.z;
					if (e0 + 3 >= off && e0 + 3 < tot) segb[e0 + 3] = t.w;
				}
			};
			constexpr int SV = MSD_C16_SV < NV ? MSD_C16_SV : NV; // vectors in flight (the counter registers are dead: eight fit beside the next segment's keys)
#pragma unroll
			for (int v0 = 0; v0 < NV; v0 += SV) {
				u32x4 t4[SV];
#pragma unroll
				for (int i = 0; i < SV; ++i) t4[i] = reinterpret_cast<const u32x4 *>(out)[(uint32_t)((v0 + i) * TH) + tq];
#pragma unroll
				for (int i = 0; i < SV; ++i) reinterpret_cast<u32x4 *>(out)[(uint32_t)((v0 + i) * TH) + tq] = u32x4{ zero, zero, zero, zero };
#pragma unroll
				for (int i = 0; i < SV; ++i) put((uint32_t)((v0 + i) * TH) + tq, t4[i]);
				__builtin_amdgcn_sched_barrier(0);
			}
			// the rest of the area (tail elements of full-size segments: at most kC16Cap / 4 - NV * TH = 256 vectors)
			{
				const uint32_t q = (uint32_t)(NV * TH) + tq;
				if (q < kC16Cap / 4) {
					const u32x4 t = reinterpret_cast<const u32x4 *>(out)[q];
					reinterpret_cast<u32x4 *>(out)[q] = u32x4{ zero, zero, zero, zero };
					put(q, t);
				}
			}
		} else if (fits)
			clear_all(); // (the counters of a rejected segment; one that does not fit was not counted)
		MSD_STAMP(10); // store + clear
		if (!more) return false;
		sg = nsg;
		__syncthreads(); // the area is clear for everybody
		return true;
	};
	for (;;) {
		if (!segment(rka, rkb)) break;
		if (!segment(rkb, rka)) break;
	}
	MSD_STAMP_FLUSH(TH / 64);
}

} // namespace msd

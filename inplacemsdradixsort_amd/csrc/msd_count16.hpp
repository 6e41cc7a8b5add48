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

template <bool BIG> // BIG: the array exceeds the memory-side cache, MSD_C16_NT applies (kStreamMinBytes, msd_device.hpp)
__global__ __launch_bounds__(kC16Th, (kC16Th >= 1024 ? 8 : 4)) void count_place16_kernel(uint32_t *__restrict__ keys,
	const Segment *__restrict__ segs, uint32_t nsegs, Segment *__restrict__ rejected, Counters *__restrict__ ctr,
	uint64_t n_total)
{
	using Tile = RegTile<kC16Th, kC16Vec, kC16Tail>; // the segment on the array's 16-byte grid
	constexpr int TH = kC16Th, NV = kC16Vec, NK = Tile::NK;
	static_assert(Tile::CAP == kC16Cap, "the output buffer holds the tile");
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
		if (kEarlyTicket) bc_tickets_in(wtot, atomicAdd(&ctr->count_ticket3, ntake) + gridDim.x, ntake);
	}
	// (segment descriptors are the same in every lane: kept in scalar registers)
	Segment sg = uniform(segs[blockIdx.x]);

	// TWO register sets of one register per key: the key (prefetched) -> value | rank << 16 -> value | place << 16 -> dead.
	// While one set carries a segment through its position look-ups and the LDS output phase, the other already
	// receives the next segment's keys (requested as soon as the 32 counter registers are dead); the loop body exists
	// twice with the sets' roles swapped, so no register is copied and no wait sits between the two segments.
	uint32_t rka[NK], rkb[NK];
	// the segment's elements on the 16-byte grid (Tile::load).  Of a segment this kernel will not take, and when there
	// is no next segment (!live), only the first vector is read.  Addresses come from an opaque copy of the thread index
	// (not hoisted out of the loop).
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
		Tile::load<NTL>(rk, base, take ? (uint32_t)tot : 1u, tp);
	};
	// the whole counter / output area to zero (16-byte stores): before the first segment and behind a rejected one;
	// behind a sorted segment the store phase leaves the area cleared
	auto clear_all = [&]() __attribute__((always_inline)) {
		uint32_t zero = 0, tc = tid;
		asm volatile("" : "+v"(zero), "+v"(tc));
		bc_clear<TH, kC16Cap>(cw, zero, tc);
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
			if (!kEarlyTicket && wtot[13] == 0) bc_tickets_in(wtot, atomicAdd(&ctr->count_ticket3, ntake) + gridDim.x, ntake);
			bc_ticket_next(wtot, nexti); // (a ticket is in hand: drawn before the loop or during the segment before)
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
						const uint32_t el = Tile::elem(u, tid);
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
		const uint32_t nxt = uniform_u32(*nexti), hi = uniform_u32(*hi_l);
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
		if (fits) totk = bc_sums<WPT, 1>(cq, cr, totk);
		if (totk > 255u) *crowded = 1; // (a byte prefix would not fit)
		const uint32_t inc = wg_scan_publish(totk, wtot, tq);
		MSD_STAMP(4); // counters read + byte sums + wave scan
		__syncthreads();
		const WgScan sc = wg_scan_collect<TH>(wtot, w, inc - totk);
		const uint32_t pos = sc.pos, all = sc.all;
		// a byte that overflowed carried into its neighbour: the sum of all bytes then falls short of n
		const bool ok = fits && all == n && *crowded == 0;
		MSD_STAMP(5);
		if (ok) {
			bc_prefixes<WPT, 1>(cq, cr);
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
		if (refill) bc_tickets_in(wtot, drawn + gridDim.x, ntake);
		if (ok) {
			MSD_STAMP(6); // byte prefixes, prefetch issue
			__syncthreads();
			// ---- place of every key: base[owner of its value] + prefix[value] + rank
			bc_places<NK, CH, WPT>(rk, tbase, cw);
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

// msd_radix.hip -- host side of the MI355X in-place MSD radix sort and its C ABI
// (include/msd_radix_hip.h).  The host plans rounds (the role of the reference's
// schedule_passes, src/msb_64.c:1334-1400, re-parameterised for LDS capacity and
// <= 8-bit digits) and launches the kernels of msd_device.hpp; it never touches
// key data itself and has no CPU fallback.
#include "msd_device.hpp"
#include "msd_select.hpp"
#include "msd_select_rows.hpp"
#include "msd_reverse.hpp"
#include "msd_sort_rows.hpp"
#include "msd_runs.hpp"
#include "msd_reduce.hpp"
#include "msd_scan.hpp"
#include "msd_compact.hpp"
#include "msd_search.hpp"
#include "msd_merge2.hpp"
#include "msd_setops.hpp"
#include "msd_join.hpp"
#include "msd_args.hpp" // the argument rules, each stated once (host only)
#include "msd_options.hpp" // the options and the counters of the context, each stated once (host only)
#include "../../include/msd_radix_hip.h"
#include "../../include/msd_sort_keys_hip.h"
#include "../../include/msd_sort_rows_hip.h"
#include "../../include/msd_runs_hip.h"
#include "../../include/msd_reduce_hip.h"
#include "../../include/msd_scan_hip.h"
#include "../../include/msd_compact_hip.h"
#include "../../include/msd_search_hip.h"
#include "../../include/msd_merge_hip.h"
#include "../../include/msd_setops_hip.h"
#include "../../include/msd_join_hip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

using namespace msd;

#define MSD_VERSION "inplacemsdradixsort_amd 0.2 (gfx950)"

struct PhaseRec {
	const char *name;
	hipEvent_t ev; // recorded at the END of the phase
};

struct msd_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	char *slab = nullptr; // device workspace of the current round (dead between rounds)
	size_t slab_bytes = 0;
	char *keep = nullptr; // device workspace that lives for the whole call
	size_t keep_bytes = 0;
	Segment *lists = nullptr; // leaf-segment lists: [general + fallbacks behind it: 3*cap][counting sort: cap]
	size_t lists_cap = 0;
	void *pinned = nullptr; // small host staging (pinned)
	size_t pinned_bytes = 0;
	hipEvent_t ev_early = nullptr; // behind a round's early copy of its counters (SortRun::send_early, read_early)
	std::string err;
	bool profiling = false;
	hipEvent_t ev_start = nullptr;
	std::vector<PhaseRec> phases;
	std::vector<hipEvent_t> ev_pool;
	size_t ev_used = 0;
	std::vector<std::pair<std::string, double>> phase_us;
	uint64_t stat[kStatCount] = {}; // the counters of msd_stat (msd_options.hpp) ...
	uint64_t stat_written = 0;      // ... and which of them the last call has written (bit = slot)
	Options opt;                    // the knobs of msd_set_option (msd_options.hpp)
	int sm_count = 256;
	int chains_per_cu[3] = { 4, 4, 2 }; // resident chains_kernel workgroups per CU: u32 keys, u64 keys, tuples (measured at msd_create)
	const uint32_t *order_keys = nullptr; // msd_order_low16_counts_u32 has run on these keys and its tables are still in the slab
	uint64_t order_n = 0;
	char *sel = nullptr;   // msd_topk_* / msd_select_*: search state, per-pass bins, candidate buffer (lives across the internal sorts)
	size_t sel_bytes = 0;
	char *rows_stage = nullptr; // msd_topk_rows, looped path: one row + k output elements for rows that are not 16-byte aligned
	size_t rows_stage_bytes = 0;
	uint64_t *fix_plan = nullptr; // msd_sort_keys: the plan words of msd_reverse.hpp (kFixWords), allocated by msd_create
	int fix_stats = 0;            // "sort_keys_split" / "sort_keys_reversed" of the last typed sort: 0 none yet, 1 fix_split and 0 (nothing was launched), 2 in the plan words
	uint64_t fix_split = 0;
};

static int fail(msd_ctx *c, int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	if (c) c->err = buf;
	return code;
}

#define HIPCHK(c, call)                                                                   \
	do {                                                                              \
		hipError_t e_ = (call);                                                   \
		if (e_ != hipSuccess)                                                     \
			return fail(c, MSD_EHIP, "%s failed: %s (%s:%d)", #call,          \
				    hipGetErrorString(e_), __FILE__, __LINE__);           \
	} while (0)

// Every kernel of this file is launched here: on the context's stream, the launch checked at once (reported with the call
// site's file and line, like HIPCHK).  The arguments are converted to the kernel's own parameter types: a call site
// needs no casts, and an argument the kernel cannot take does not compile.
template <typename... P, typename... A>
static int launch_at(msd_ctx *c, const char *what, const char *file, int line, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A &...args)
{
	hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, static_cast<P>(args)...);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? MSD_OK : fail(c, MSD_EHIP, "launch of %s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}
// (an expression: MSD_OK or the error)
#define LAUNCH_RC(c, kernel, grid, block, lds, ...) launch_at(c, #kernel, __FILE__, __LINE__, kernel, dim3(grid), dim3(block), lds, __VA_ARGS__)
// (a statement, like HIPCHK: returns the error from the calling function)
#define LAUNCH(c, kernel, grid, block, lds, ...)                                                    \
	do {                                                                                        \
		if (int rc_ = LAUNCH_RC(c, kernel, grid, block, lds, __VA_ARGS__)) return rc_;      \
	} while (0)

static void set_stat(msd_ctx *c, Stat slot, uint64_t v)
{
	c->stat[slot] = v;
	c->stat_written |= 1ull << slot;
}
static void add_stat(msd_ctx *c, Stat slot, uint64_t v)
{
	set_stat(c, slot, (c->stat_written >> slot & 1 ? c->stat[slot] : 0) + v);
}

// ------------------------------------------------------------ workspace slab

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// (exact: msd_reserve's sizes are the planner's own worst case for the shape; a buffer that has to grow in the middle of a
// sort gets an eighth on top, so that the next slightly bigger round does not allocate again)
static int dev_reserve(msd_ctx *c, char *&p, size_t &have, size_t bytes, bool exact = false)
{
	if (bytes <= have) return MSD_OK;
	if (p) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipFree(p));
		p = nullptr;
		have = 0;
	}
	bytes = align_up(exact ? bytes : bytes + bytes / 8, 1 << 20);
	hipError_t e = hipMalloc((void **)&p, bytes);
	if (e != hipSuccess) return fail(c, MSD_ENOMEM, "workspace hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
	have = bytes;
	return MSD_OK;
}
static int slab_reserve(msd_ctx *c, size_t bytes, bool exact = false)
{
	c->order_keys = nullptr; // (whoever reserves the slab overwrites the tables a pending msd_order_low16_scatter_u32 would read)
	return dev_reserve(c, c->slab, c->slab_bytes, bytes, exact);
}
static int keep_reserve(msd_ctx *c, size_t bytes, bool exact = false) { return dev_reserve(c, c->keep, c->keep_bytes, bytes, exact); }

// Leaf lists grow between rounds (the host knows how many children a round can add);
// live entries are carried over.
static int lists_reserve(msd_ctx *c, size_t need, size_t live_general, size_t live_count, bool exact = false)
{
	if (need <= c->lists_cap) return MSD_OK;
	const size_t cap = align_up(exact ? need : need + need / 2, 4096);
	Segment *nb = nullptr;
	hipError_t e = hipMalloc((void **)&nb, 4 * cap * sizeof(Segment));
	if (e != hipSuccess) return fail(c, MSD_ENOMEM, "leaf list hipMalloc failed: %s", hipGetErrorString(e));
	if (c->lists) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		if (live_general) HIPCHK(c, hipMemcpy(nb, c->lists, live_general * sizeof(Segment), hipMemcpyDeviceToDevice));
		if (live_count) HIPCHK(c, hipMemcpy(nb + 3 * cap, c->lists + 3 * c->lists_cap, live_count * sizeof(Segment), hipMemcpyDeviceToDevice));
		HIPCHK(c, hipFree(c->lists));
	}
	c->lists = nb;
	c->lists_cap = cap;
	return MSD_OK;
}

struct Bump { // sizing pass (base == nullptr) or carving pass
	char *base;
	size_t off = 0;
	explicit Bump(char *b) : base(b) {}
	template <typename T> T *take(size_t n)
	{
		off = align_up(off, 256);
		T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
		off += n * sizeof(T);
		return p;
	}
};

static int pinned_reserve(msd_ctx *c, size_t bytes)
{
	if (bytes <= c->pinned_bytes) return MSD_OK;
	if (c->pinned) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipHostFree(c->pinned));
		c->pinned = nullptr;
	}
	bytes = align_up(bytes * 2, 4096);
	HIPCHK(c, hipHostMalloc(&c->pinned, bytes, hipHostMallocDefault));
	c->pinned_bytes = bytes;
	return MSD_OK;
}

// The slab in two passes: `carve` (a function of a Bump) sizes it, the slab grows to that (at least to `min_bytes`), and
// `carve` lays it out
template <typename F> static int slab_carve(msd_ctx *c, F &&carve, size_t min_bytes = 0, bool exact = false)
{
	Bump sz(nullptr);
	carve(sz);
	if (int rc = slab_reserve(c, std::max(sz.off + 4096, min_bytes), exact)) return rc;
	Bump real(c->slab);
	carve(real);
	return MSD_OK;
}

// The slab as it stands -- whoever reserved it knows that `carve` fits -- laid out once more
template <typename F> static void slab_recarve(msd_ctx *c, F &&carve)
{
	Bump real(c->slab);
	carve(real);
}

// ------------------------------------------------------------ host <-> device through the pinned staging buffer

struct ToDevice { void *dst; const void *src; size_t bytes; };
// Host arrays to the device: one wait until the staging buffer's last contents have left (the caller has reserved it big
// enough), then one hipMemcpyAsync per non-empty piece, the pieces one behind the other in the buffer
static int upload(msd_ctx *c, std::initializer_list<ToDevice> pieces)
{
	HIPCHK(c, hipStreamSynchronize(c->stream)); // the staging buffer may still be in flight
	char *at = (char *)c->pinned;
	for (const ToDevice &p : pieces) {
		if (!p.bytes) continue;
		memcpy(at, p.src, p.bytes);
		HIPCHK(c, hipMemcpyAsync(p.dst, at, p.bytes, hipMemcpyHostToDevice, c->stream));
		at += p.bytes;
	}
	return MSD_OK;
}

struct ToHost { size_t at; const void *src; size_t bytes; void *out = nullptr; }; // (at: offset in the staging buffer; out: where the host wants a copy)
// The counters, and with them the non-empty `extra` device ranges (to their places in the staging buffer): one synchronisation
static int read_counters(msd_ctx *c, const Counters *ctr, Counters &hc, std::initializer_list<ToHost> extra = {})
{
	HIPCHK(c, hipMemcpyAsync(c->pinned, ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
	for (const ToHost &p : extra)
		if (p.bytes) HIPCHK(c, hipMemcpyAsync((char *)c->pinned + p.at, p.src, p.bytes, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	memcpy(&hc, c->pinned, sizeof hc);
	for (const ToHost &p : extra)
		if (p.out) memcpy(p.out, (const char *)c->pinned + p.at, p.bytes);
	return MSD_OK;
}

// `count` values of a device array to `out` on the host (the caller has reserved the staging buffer; one copy, one synchronisation)
template <typename T> static int read_back(msd_ctx *c, const T *src, T *out, size_t count = 1)
{
	HIPCHK(c, hipMemcpyAsync(c->pinned, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	memcpy(out, c->pinned, count * sizeof(T));
	return MSD_OK;
}

// `count` elements of a device array appended to `out` (the staging buffer grows to fit; one copy, one synchronisation)
template <typename T> static int fetch(msd_ctx *c, const T *src, size_t count, std::vector<T> &out)
{
	if (int rc = pinned_reserve(c, count * sizeof(T))) return rc;
	HIPCHK(c, hipMemcpyAsync(c->pinned, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	out.insert(out.end(), (const T *)c->pinned, (const T *)c->pinned + count);
	return MSD_OK;
}

static void sort_by_start(std::vector<Segment> &v)
{
	std::sort(v.begin(), v.end(), [](const Segment &a, const Segment &b) { return a.start < b.start; });
}

// A device Segment list appended to `out`, then `out` in the order of `start` (atomic appends arrive in any order; the plan
// must be deterministic).  A list of up to `ahead` entries came back with the counters, to `pre`: no copy then.
static int fetch_segments(msd_ctx *c, const Segment *src, uint32_t count, std::vector<Segment> &out, const void *pre = nullptr,
			  size_t ahead = 0)
{
	if (count <= ahead)
		out.insert(out.end(), (const Segment *)pre, (const Segment *)pre + count);
	else if (int rc = fetch(c, src, count, out))
		return rc;
	sort_by_start(out);
	return MSD_OK;
}

// ------------------------------------------------------------ phase timing

static void phase_begin(msd_ctx *c)
{
	c->phases.clear();
	c->ev_used = 0;
	c->phase_us.clear();
	if (!c->profiling) return;
	if (!c->ev_start) (void)hipEventCreate(&c->ev_start);
	(void)hipEventRecord(c->ev_start, c->stream);
}
static void phase_mark(msd_ctx *c, const char *name)
{
	if (!c->profiling) return;
	if (c->ev_used == c->ev_pool.size()) {
		hipEvent_t e;
		(void)hipEventCreate(&e);
		c->ev_pool.push_back(e);
	}
	hipEvent_t e = c->ev_pool[c->ev_used++];
	(void)hipEventRecord(e, c->stream);
	c->phases.push_back({ name, e });
}
// add to the entry of that name, or append one
static void phase_add(std::vector<std::pair<std::string, double>> &list, const std::string &name, double us)
{
	for (auto &q : list)
		if (q.first == name) {
			q.second += us;
			return;
		}
	list.emplace_back(name, us);
}
static void phase_end(msd_ctx *c)
{
	if (!c->profiling) return;
	(void)hipStreamSynchronize(c->stream);
	hipEvent_t prev = c->ev_start;
	for (auto &p : c->phases) {
		float ms = 0;
		(void)hipEventElapsedTime(&ms, prev, p.ev);
		phase_add(c->phase_us, p.name, ms * 1000.0);
		prev = p.ev;
	}
}

// ------------------------------------------------------------ round planning

struct RoundPlan {
	std::vector<Parent> parents;
	std::vector<Stripe> stripes;
	uint32_t nchildren = 0;
	uint64_t lo_elems = 0;   // leftover area, elements
	uint64_t nslots = 0;     // slots covered by the stripes
	uint64_t round_keys = 0;
};

static uint32_t ceil_log2_u64(uint64_t x)
{
	uint32_t p = 0;
	while (((uint64_t)1 << p) < x) ++p;
	return p;
}

// Digit width for a parent: 8 bits for big parents, fewer when that already brings
// the children down to about half the LDS-sort capacity.  `leaf_bits` > 0 (keys without
// payload): children that are leaves should keep <= leaf_bits open bits so that the
// one-pass counting sort can finish them.
static uint32_t pick_width(uint64_t count, uint32_t bits, uint64_t small_max, uint32_t leaf_bits)
{
	uint64_t target = small_max / 2;
	uint32_t w = ceil_log2_u64((count + target - 1) / target);
	w = std::max(1u, std::min(8u, w));
	w = std::min(w, bits);
	// widen only while the leaves stay big enough to amortise the counting sort's 64 KiB of counters
	if (leaf_bits && bits - w > leaf_bits && bits <= leaf_bits + 8 && (count >> (bits - leaf_bits)) <= small_max &&
	    (count >> (bits - leaf_bits)) >= 2048)
		w = bits - leaf_bits;
	return w;
}

template <typename K, typename V>
static void plan_round(const std::vector<Segment> &segs, uint64_t small_max, int sm_count, RoundPlan &rp, uint32_t leaf_bits = 0,
		       uint32_t forced_width = 0, uint32_t nsplit = 0)
{
	using C = Cfg<K, V>;
	constexpr uint64_t B = C::B, T = C::T;
	rp = RoundPlan();
	uint64_t total = 0;
	for (auto &s : segs) total += s.count;
	rp.round_keys = total;
	// stripe length: enough stripes to fill the chip a few times over, whole tiles
	// (experiment knobs, compiled in with -DMSD_STRIPE_WANT= / -DMSD_STRIPE_CAP_LOG= for variant builds only:
	// tools/variant_run.py.  They used to be read from the environment, unchecked, by every context of the process.)
#ifndef MSD_STRIPE_WANT
#define MSD_STRIPE_WANT 4
#endif
#ifndef MSD_STRIPE_CAP_LOG
#define MSD_STRIPE_CAP_LOG 20
#endif
	static_assert(MSD_STRIPE_WANT >= 1 && MSD_STRIPE_WANT <= 64 && MSD_STRIPE_CAP_LOG >= 12 && MSD_STRIPE_CAP_LOG <= 20, "stripe geometry knobs out of range (a stripe has at most 2^20 elements)");
	constexpr int want_mul = MSD_STRIPE_WANT, cap_log = MSD_STRIPE_CAP_LOG;
	uint64_t want = std::max<uint64_t>(1, (uint64_t)sm_count * want_mul);
	uint64_t slen = (total + want - 1) / want;
	slen = std::max<uint64_t>(slen, 4 * T);
	slen = std::min<uint64_t>(slen, (uint64_t)1 << cap_log);
	slen = (slen + T - 1) / T * T;
	for (auto &s : segs) {
		Parent p;
		p.start = s.start;
		p.count = s.count;
		p.width = forced_width ? forced_width : pick_width(s.count, s.bits, small_max, leaf_bits);
		p.shift = s.bits - p.width;
		p.child_base = rp.nchildren;
		p.stripe_lo = (uint32_t)rp.stripes.size();
		p.pad = nsplit; // range partitioning: number of delimiters
		rp.nchildren += 1u << p.width;
		const uint64_t end = s.start + s.count;
		const uint64_t a0 = (s.start + B - 1) / B * B; // first aligned position
		uint64_t b = s.start;
		while (b < end) {
			uint64_t e = (b == s.start ? a0 : b) + slen;
			if (e + slen / 2 > end) e = end; // do not leave a short last stripe
			Stripe st;
			st.begin = b;
			st.end = e;
			st.parent = (uint32_t)rp.parents.size();
			st.slot_lo = (uint32_t)((b + B - 1) / B);
			st.slot_hi = (uint32_t)(e / B);
			if (st.slot_hi < st.slot_lo) st.slot_hi = st.slot_lo;
			st.lo_base = rp.lo_elems;
			st.pad = 0;
			// leftovers: < B per bucket (2^width buckets) from the stream, plus < B head keys
			rp.lo_elems += std::min<uint64_t>(e - b, ((uint64_t)1 << p.width) * (B - 1) + 2 * B);
			rp.nslots += st.slot_hi - st.slot_lo;
			rp.stripes.push_back(st);
			b = e;
		}
		p.stripe_hi = (uint32_t)rp.stripes.size();
		rp.parents.push_back(p);
	}
}

struct RoundBufs {
	Parent *parents;
	Stripe *stripes;
	uint32_t *fb, *lo_cnt, *lo_off, *lo_dst, *nfull;
	void *lo_keys;
	uint64_t *lo_vals;
	ChildArrays ca;
	ListEntry *list, *holes;
	void *xkeys;
	uint64_t *xvals;
	unsigned long long *scan_state;
	uint32_t *scan_ctr;
	Segment *next_parents;
	DirectPlan *plans; // per parent (direct placement)
	uint32_t *scan_part; // child_scan_part_kernel's sums per (parent, stripe group), where the round's child scan is split
};

// Workgroups per parent of the round's child scan: 1 = child_scan_kernel, more = the split pair (msd_device.hpp)
static uint32_t child_scan_groups(const RoundPlan &rp)
{
	uint32_t longest = 0;
	for (const Parent &p : rp.parents) longest = std::max(longest, p.stripe_hi - p.stripe_lo);
	if (longest < kChildScanSplit || rp.parents.size() > kChildScanSplitParents) return 1;
	return std::min(kChildScanGroupsMax, (longest + kChildScanGroup - 1) / kChildScanGroup);
}

// direct placement is tried on rounds of at most this many parents
constexpr size_t kDirectMaxParents = 4096;

template <typename K, typename V>
static void carve_round(Bump &b, const RoundPlan &rp, uint64_t small_max, RoundBufs &rb)
{
	using C = Cfg<K, V>;
	constexpr bool HV = has_val<V>::value;
	const size_t np = rp.parents.size(), ns = rp.stripes.size(), nc = rp.nchildren;
	rb.parents = b.take<Parent>(np);
	rb.stripes = b.take<Stripe>(ns);
	rb.fb = b.take<uint32_t>(ns * kP);
	rb.lo_cnt = b.take<uint32_t>(ns * kP);
	rb.lo_off = b.take<uint32_t>(ns * kP);
	rb.lo_dst = b.take<uint32_t>(ns * kP);
	rb.nfull = b.take<uint32_t>(ns);
	rb.lo_keys = b.take<K>(rp.lo_elems);
	rb.lo_vals = HV ? b.take<uint64_t>(rp.lo_elems) : nullptr;
	rb.ca.start = b.take<uint64_t>(nc);
	rb.ca.count = b.take<uint64_t>(nc);
	rb.ca.F = b.take<uint32_t>(nc);
	rb.ca.is = b.take<uint32_t>(nc);
	rb.ca.I = b.take<uint32_t>(nc);
	rb.ca.lsum = b.take<uint32_t>(nc);
	rb.ca.n_int = b.take<uint32_t>(nc);
	rb.ca.n_fr = b.take<uint32_t>(nc);
	rb.ca.n_int0 = b.take<uint32_t>(nc);
	rb.ca.cur_int = b.take<uint32_t>(nc);
	rb.ca.cur_fr = b.take<uint32_t>(nc);
	rb.ca.list_len = b.take<uint64_t>(nc);
	rb.ca.list_base = b.take<uint64_t>(nc);
	rb.ca.rpos = b.take<uint32_t>((size_t)nc * kRposStride);
	rb.ca.flags = b.take<uint32_t>(nc);
	rb.ca.rot = b.take<uint32_t>(nc);
	rb.ca.nev = b.take<uint32_t>(nc);
	rb.ca.xfirst = b.take<uint32_t>(nc);
	rb.ca.hot_cur = b.take<uint32_t>((size_t)kHotMax * kHotShards * kRposStride);
	rb.ca.lmeta = b.take<u32x4>(nc);
	rb.list = b.take<ListEntry>(rp.nslots + 1);
	// holes: tail slots (< kP + 2 per stripe) + one eviction + one excess per child
	// + the eviction pool: what it takes to reach kMinChains chains (shared out in proportion to the list
	// lengths, rounded up per child) plus the one parked block a list without a chain-ending entry needs
	const uint64_t pool = 2ull * nc + kMinChains;
	const uint64_t hmax = std::min<uint64_t>(rp.nslots, (uint64_t)ns * (kP + 2)) + 2ull * nc + pool + 1;
	rb.holes = b.take<ListEntry>(hmax);
	rb.xkeys = b.take<K>((size_t)(2 * nc + pool) * C::B);
	rb.xvals = HV ? b.take<uint64_t>((size_t)(2 * nc + pool) * C::B) : nullptr;
	const size_t ntiles = (nc + kScanTile - 1) / kScanTile + 1;
	rb.scan_state = b.take<unsigned long long>(ntiles);
	rb.scan_ctr = b.take<uint32_t>(4);
	// children that stay big: each has > small_max elements
	rb.next_parents = b.take<Segment>(rp.round_keys / (small_max + 1) + 2);
	rb.plans = b.take<DirectPlan>(np <= kDirectMaxParents ? np : 1);
	const uint32_t groups = child_scan_groups(rp);
	rb.scan_part = b.take<uint32_t>(groups > 1 ? np * groups * 2 * kP : 1);
}

// ------------------------------------------------------------------ the sort

// Leaf-list entries msd_reserve() provides up front: what evenly spread keys need (two 8-bit rounds over 2^30 u32 keys
// leave 2^16 counting segments; a round reserves room for one entry per child on top of the live ones), not the most
// any input could need -- the lists grow between rounds when an input leaves more, smaller segments (lists_reserve).
// (Round 2 reserved n / 1024 + 6 n / leaf capacity entries, 1.5 times over: 189 MB of the 646 MB at 2^30 u32 keys.)
template <typename K, typename V> static uint64_t leaf_list_guess(uint64_t n)
{
	return std::min<uint64_t>(n / 8192 + 4096, n / 2 + 16);
}

namespace { // (the sort's own types: not exported)

// Device buffers that live for a whole sort call of n elements (the context's `keep` area)
struct KeepBufs {
	uint8_t *block_map, *slot_full; // bucket of every block slot; slots a direct round filled
	Counters *ctr;       // counters + scratch for the varying-bit reduction
	uint32_t big_cap;
	Segment *big;        // big counting-sort segments
	Segment *dev_list;   // (u64 keys) parents of a device-planned round
	template <typename K, typename V> void carve_keep(Bump &b, uint64_t n)
	{
		constexpr uint64_t B = Cfg<K, V>::B, small_max = (uint64_t)Cfg<K, V>::SORT_TH * Cfg<K, V>::SORT_KPT;
		block_map = b.take<uint8_t>(n / B + 2);
		slot_full = b.take<uint8_t>(n / B + 2);
		ctr = b.take<Counters>(3); // ([1]: scratch of the varying-bit reduction, [2]: a finished round's counters, parked by round_init_kernel)
		big_cap = (uint32_t)std::min<uint64_t>(n / small_max + 16, 0x7FFFFFFFu);
		big = b.take<Segment>(big_cap);
		dev_list = sizeof(K) == 8 ? b.take<Segment>(n / (small_max + 1) + 2) : nullptr;
	}
};

template <typename K, typename V> static size_t keep_bytes_for(uint64_t n)
{
	Bump b(nullptr);
	KeepBufs().carve_keep<K, V>(b, n);
	return b.off + 4096;
}

// Per-round workspace for the two shapes the headline sizes produce: one parent
// covering everything, and 256 equal parents.  Other shapes grow the slab between
// rounds (nothing in it is live there).
template <typename K, typename V>
static size_t round_bytes_estimate(uint64_t n, int sm_count)
{
	using C = Cfg<K, V>;
	const uint64_t small_max = (uint64_t)C::SORT_TH * C::SORT_KPT;
	size_t worst = 0;
	for (int shape = 0; shape < 2; ++shape) {
		std::vector<Segment> segs;
		if (shape == 0)
			segs.push_back({ 0, n, (uint32_t)(sizeof(K) * 8), 0 });
		else if (n > 512 * small_max)
			for (int i = 0; i < 256; ++i) segs.push_back({ n / 256 * i, n / 256, (uint32_t)(sizeof(K) * 8 - 8), 0 });
		if (segs.empty()) continue;
		RoundPlan rp;
		plan_round<K, V>(segs, small_max, sm_count, rp);
		Bump b(nullptr);
		RoundBufs rb;
		carve_round<K, V>(b, rp, small_max, rb);
		worst = std::max(worst, b.off);
	}
	return worst + 4096;
}

// What one call of sort_impl does.  Every entry point builds one; sort_impl checks the arguments that go with it.
template <typename K> struct SortJob {
	enum Kind {
		kWhole,   // sort every key (on its low end_bit bits) ...
		kDigit,   // ... or one round on a caller-chosen digit (msd_partition_*)
		kRanges,  // ... or one round whose buckets are the key's range among nsplit ascending delimiters (msd_partition_by_splitters_*)
		kOffsets, // ... or a sort of nseg independent segments [seg_off[i], seg_off[i + 1]) (msd_sort_*_segments)
		kList,    // ... or of explicit disjoint segments, each with its own number of open bits (internal: what the merge leaf rejected)
	} kind = kWhole;
	uint32_t stop_bits = 0;            // kWhole: stop early, the keys are only to be ordered by key >> stop_bits (msd_sort_*_top)
	unsigned shift = 0, width = 0;     // kDigit: the digit; kRanges: its width
	uint64_t *counts = nullptr;        // kDigit, kRanges: bucket sizes (optional)
	const K *splitters = nullptr;      // kRanges (nsplit of them)
	const uint64_t *seg_off = nullptr; // kOffsets (nseg + 1 of them)
	uint32_t nsplit = 0, nseg = 0;
	const std::vector<Segment> *segs = nullptr; // kList

	static SortJob whole(uint32_t stop_bits = 0) { return { kWhole, stop_bits }; }
	static SortJob digit(unsigned shift, unsigned width, uint64_t *counts) { return { kDigit, 0, shift, width, counts }; }
	static SortJob ranges(const K *delims, uint32_t nsplit, unsigned width, uint64_t *counts) { return { kRanges, 0, 0, width, counts, delims, nullptr, nsplit }; }
	static SortJob offsets(const uint64_t *seg_off, uint32_t nseg) { return { kOffsets, 0, 0, 0, nullptr, nullptr, seg_off, 0, nseg }; }
	static SortJob list(const std::vector<Segment> &segs) { return { kList, 0, 0, 0, nullptr, nullptr, nullptr, 0, 0, &segs }; }
	bool single_pass() const { return kind == kDigit || kind == kRanges; }
	bool segmented() const { return kind == kOffsets || kind == kList; }
};

// a stage's verdict that the exact check behind a sampled leading-bit skip failed: the sort starts over (not an MSD_ code)
constexpr int kRestart = 1;

// One sort call: its state between the stages, and the stages
template <typename K, typename V> struct SortRun : KeepBufs {
	using C = Cfg<K, V>;
	static constexpr bool HV = has_val<V>::value;
	static constexpr int B = C::B;
	static constexpr uint64_t small_max = (uint64_t)C::SORT_TH * C::SORT_KPT;
	// keys without payload whose last <= 16 bits are open are finished by the counting sort
	static constexpr uint32_t count_bits = HV ? (uint32_t)kLeafCountBits : (uint32_t)kCountMaxBits;

	msd_ctx *const c;
	K *const keys;
	uint64_t *const vals;
	const uint64_t n, low_mask;
	const int end_bit;
	const SortJob<K> &job;

	std::vector<Segment> cur; // parents of the next round, in the order of `start` ...
	uint32_t dev_np = 0;      // ... or this many, left on the device (dev_list) by the last round
	uint32_t nsmall_host = 0, ncount_host = 0, nbig_host = 0; // leaf-list lengths as the host last read them
	unsigned long long *vres = nullptr;                       // OR / AND words of the varying-bit reduction
	int round = 0;
	// the previous round placed its blocks directly (its digit was evenly spread); segments handed in by the caller are
	// taken to be such a round's children (the shards of a multi-GPU sort after their top-digit pass and exchange)
	bool prev_direct;
	bool unverified = false;    // a leading-bit skip stands on the sample alone (skip_leading_bits)
	uint64_t claimed_const = 0; // bits below end_bit the sample found constant
	uint64_t exact_vary = 0;    // with kRestart: the bits the exact check found varying
	bool leaf17_ok = true;      // (tuples) leaf17_kernel has rejected nothing yet in this call
	uint32_t nfallback_known = 0xFFFFFFFFu; // segments the counting leaves have handed to the general LDS sort, once the host has seen it

	SortRun(msd_ctx *c_, K *keys_, uint64_t *vals_, uint64_t n_, int end_bit_, const SortJob<K> &job_)
		: c(c_), keys(keys_), vals(vals_), n(n_), low_mask(end_bit_ >= 64 ? ~0ull : ((1ull << end_bit_) - 1ull)), end_bit(end_bit_), job(job_),
		  prev_direct(job_.kind == SortJob<K>::kOffsets) {}

	// the leaf lists (they move when they grow): LDS leaves (the general LDS sort's fallbacks behind them), counting leaves
	Segment *small() const { return c->lists; }
	Segment *small_count() const { return c->lists + 3 * c->lists_cap; }

	// ---- the segments the sort starts on
	int initial_segments()
	{
		if (job.single_pass()) {
			if (job.width < 1 || job.width > 8 || job.shift + job.width > sizeof(K) * 8)
				return fail(c, MSD_EINVAL, "partition: radix_bits must be 1..8 and shift+radix_bits within the key");
			cur.push_back({ 0, n, job.shift + job.width, 0 });
		} else if (job.kind == SortJob<K>::kOffsets) {
			const uint64_t *off = job.seg_off;
			for (uint32_t i = 0; i < job.nseg; ++i) {
				if (off[i] > off[i + 1] || off[i + 1] > n) return fail(c, MSD_EINVAL, "segments: offsets must ascend and stay within n");
				if (end_bit > 0 && off[i + 1] - off[i] > 1) cur.push_back({ off[i], off[i + 1] - off[i], (uint32_t)end_bit, 0 });
			}
		} else if (job.kind == SortJob<K>::kList) {
			for (auto &sg : *job.segs) {
				if (sg.start + sg.count > n || sg.bits > sizeof(K) * 8) return fail(c, MSD_EINVAL, "segments: a segment lies outside the array");
				if (sg.bits > 0 && sg.count > 1) cur.push_back(sg);
			}
			sort_by_start(cur);
		} else if (end_bit > 0 && n > 1 && (uint32_t)end_bit > job.stop_bits)
			cur.push_back({ 0, n, (uint32_t)end_bit, 0 });
		return MSD_OK;
	}

	// ---- buffers that live for the whole call
	int reserve_keep()
	{
		int rc = keep_reserve(c, keep_bytes_for<K, V>(n), true);
		if (!rc) rc = pinned_reserve(c, 1 << 16);
		if (!rc) rc = lists_reserve(c, 4096, 0, 0);
		if (rc) return rc;
		Bump kb(c->keep);
		carve_keep<K, V>(kb, n);
		vres = reinterpret_cast<unsigned long long *>(ctr + 1);
		HIPCHK(c, hipMemsetAsync(ctr, 0, sizeof(Counters), c->stream));
		return MSD_OK;
	}

	int vres_init() // OR accumulator 0, AND accumulator all ones (no host round trip)
	{
		HIPCHK(c, hipMemsetAsync(vres, 0x00, sizeof(unsigned long long), c->stream));
		HIPCHK(c, hipMemsetAsync(vres + 1, 0xFF, sizeof(unsigned long long), c->stream));
		return MSD_OK;
	}
	// the bits in which the keys at every stride-th position differ
	int run_vary(uint64_t stride, uint64_t *vary_out)
	{
		if (int rc = vres_init()) return rc;
		const uint64_t cnt = (n + stride - 1) / stride;
		const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 8, (cnt + 255) / 256);
		LAUNCH(c, (vary_kernel<K>), grid, 256, 0, keys, n, stride, vres);
		unsigned long long h[2];
		if (int rc = read_back(c, vres, h, 2)) return rc;
		*vary_out = h[0] ^ h[1];
		return MSD_OK;
	}

	// ---- leading-bit skipping: a cheap strided sample decides whether an exact OR/AND pass over
	// all keys can pay off (it does when whole leading digits are constant, e.g. keys whose upper
	// half is zero); all-equal inputs are finished here.
	// A skip decided from the sample alone is `unverified`: the rounds only permute keys, so the exact check may come
	// later -- on the exact histogram pass of the second round if that reads every key (it costs that pass nothing:
	// 1.4 ms less for 2^30 tuples with 32 constant key bits), else in a pass of its own before the leaves, which
	// re-generate keys from a common prefix and must not run on a wrong one.  If the check fails (some key differs
	// in a bit the sample found constant) the sort starts over on all bits the exact pass found varying: the data is
	// still the same multiset.
	int skip_leading_bits()
	{
		if (job.single_pass() || job.segmented() || cur.empty() || n < 4096) return MSD_OK;
		uint64_t vary = 0;
		int rc = run_vary(std::max<uint64_t>(1, n / 8192), &vary);
		if (rc) return rc;
		vary &= low_mask;
		const int top_sample = vary ? 64 - __builtin_clzll(vary) : 0;
		if (top_sample + 8 <= end_bit) { // at least one whole leading digit looks constant
			if (top_sample > 0 && c->opt.direct_mode != 0 && n >= c->opt.direct_min && n >= ((uint64_t)1 << 24)) {
				unverified = true;
				claimed_const = low_mask & ~(((uint64_t)1 << top_sample) - 1ull);
				cur[0].bits = (uint32_t)top_sample;
				set_stat(c, kStatSkippedBits, (uint64_t)(end_bit - top_sample));
			} else { // make sure at once
				rc = run_vary(1, &vary);
				if (rc) return rc;
				vary &= low_mask;
				const int top = vary ? 64 - __builtin_clzll(vary) : 0;
				set_stat(c, kStatSkippedBits, (uint64_t)(end_bit - top));
				if (top == 0)
					cur.clear(); // every key is the same on the bits in question: already sorted
				else
					cur[0].bits = (uint32_t)top;
			}
		}
		phase_mark(c, "bit skip");
		if (!cur.empty() && cur[0].bits <= job.stop_bits) cur.clear(); // (a sort that stops above every varying bit)
		return MSD_OK;
	}

	// ---- the front pass (msd_front16.hpp): a whole-array sort of u32 keys whose plan is two direct 8-bit rounds counts the
	// top 16 key bits once, before round 0.  ONE readback then tells the host what it used to learn in three instalments
	// (the bit-skip sample, round 0's sample, round 1's exact count): the exact OR / AND of the keys, round 0's children =
	// round 1's parents, both rounds' verdicts on direct placement, and that every child of round 1 is a counting leaf.
	// Both rounds are placed from exact counts (front_apply_kernel where direct_sample_kernel / direct_hist_kernel ran), and
	// the host enqueues round 0, round 1 and the leaves without waiting in between (plan_next_early, early_summary).
	// Declined -- the sort goes on as it always did, the keys are untouched -- if a whole leading digit is constant, if
	// either round is uneven or has runs, if a counter overflowed, or if some child is no counting leaf.  Inputs that a
	// sample of 2^15 keys shows to be hopeless (front_probe_kernel: Zipf keys, small key ranges, sorted input) are declined
	// without the read: the counting kernel returns at once, the same readback says so.
	bool front = false; // this sort takes the front path
	FrontSummary fsum;  // the summary as read back
	// (device) the 2^16 counts and the summary live in the second quarter of the leaf lists, which nothing uses before the
	// leaves run; the per-workgroup partials in the round slab, which is free before round 0
	uint32_t *front_hist() const { return reinterpret_cast<uint32_t *>(c->lists + c->lists_cap); }
	FrontSummary *front_sum() const { return reinterpret_cast<FrontSummary *>(front_hist() + (size_t)kP * kP); }
	int front_count()
	{
		if constexpr (!HV && sizeof(K) == 4) {
			if (!c->opt.front_count || job.kind != SortJob<K>::kWhole || job.stop_bits || end_bit != 32 || cur.size() != 1 || c->opt.direct_mode == 0 ||
			    n < c->opt.direct_min || n < c->opt.front_min || n < ((uint64_t)1 << 20) || n >= ((uint64_t)1 << 32))
				return MSD_OK;
			{ // would today's plan run two direct 8-bit rounds on evenly spread keys?  (Round 1's parents an eighth below and
			  // above the mean must still get 8-bit digits: near the size where the planner changes its mind -- 2^27 -- half
			  // of them do not, and the count would be paid for nothing.)
				const uint64_t mean = n / kP;
				if (pick_width(n, 32, small_max, count_bits) != 8 || mean - mean / 8 < c->opt.direct_min_parent ||
				    pick_width(mean - mean / 8, 24, small_max, count_bits) != 8 || pick_width(mean + mean / 8, 24, small_max, count_bits) != 8)
					return MSD_OK;
			}
			// (the slab as round 0 reserves it, the lists as round 1 does: nothing grows because of this pass, and the
			// lists do not move between here and round 1)
			int rc = slab_reserve(c, round_bytes_estimate<K, V>(n, c->sm_count), true);
			if (!rc) rc = lists_reserve(c, (size_t)kP * kP + 16, 0, 0);
			if (rc) return rc;
			static_assert(((size_t)kP * kP + 16) * sizeof(Segment) >= (size_t)kP * kP * 4 + sizeof(FrontSummary), "the counts and the summary fit a quarter of the lists");
			const unsigned grid = (unsigned)std::min<uint64_t>({ (uint64_t)c->sm_count, std::max<uint64_t>(1, n >> 18), c->slab_bytes / (kF16Words * sizeof(uint32_t)) });
			if (!grid) return MSD_OK;
			uint32_t *partials = nullptr;
			slab_recarve(c, [&](Bump &b) { partials = b.take<uint32_t>((size_t)grid * kF16Words); });
			LAUNCH(c, (front_probe_kernel<K>), 1, 1024, 0, keys, n, 16u, front_sum()); // (clears the summary first)
			LAUNCH(c, (front_count16_kernel<K>), grid, kF16Th, kF16Lds, keys, n, 16u, partials, front_sum());
			LAUNCH(c, front_plan_kernel, kP, 256, 0, partials, grid, front_hist(), front_sum(), 16u, job.stop_bits, count_bits, small_max,
			       std::max<uint64_t>(small_max, kCountMedMax));
			LAUNCH(c, front_top_kernel, 1, 256, 0, front_sum());
			if ((rc = read_back(c, front_sum(), &fsum))) return rc;
			phase_mark(c, "front count");
			const uint64_t vary = (fsum.v_or ^ fsum.v_and) & low_mask;
			const int top = vary ? 64 - __builtin_clzll(vary) : 0;
			if (fsum.hopeless) { // front_probe_kernel: skewed or in runs by a sample, nothing was counted
				add_stat(c, kStatFrontCountDeclined, 1);
				return MSD_OK;
			}
			bool ok = !fsum.overflow && top + 8 > end_bit && !fsum.uneven[0] && !fsum.uneven[1] && fsum.nroute[kRouteCount + 1] == (uint32_t)kP * kP;
			std::vector<Segment> next = front_parents();
			uint64_t total = 0;
			for (const Segment &sg : next) { // round 1 as the host will plan it: every parent big enough, with an 8-bit digit
				ok = ok && sg.count >= c->opt.direct_min_parent && pick_width(sg.count, sg.bits, small_max, count_bits) == 8;
				total += sg.count;
			}
			if (!fsum.overflow && total != n) return fail(c, MSD_EINTERNAL, "front count: the counts add up to %llu of %llu keys", (unsigned long long)total, (unsigned long long)n);
			add_stat(c, ok ? kStatFrontCountSorts : kStatFrontCountDeclined, 1);
			front = ok;
		}
		return MSD_OK;
	}
	// round 0's children, which are round 1's parents, from the front pass's summary
	std::vector<Segment> front_parents() const
	{
		std::vector<Segment> v;
		uint64_t at = 0;
		for (int d = 0; d < kP; ++d) {
			v.push_back({ at, fsum.top[d], (uint32_t)end_bit - 8u, 0 });
			at += fsum.top[d];
		}
		return v;
	}

	// ---- segments that need no partition round go to the leaf lists at once
	int route_to_leaves()
	{
		if (job.segmented() && !cur.empty()) {
			// collect_kernel's rule (route_child), with the limits of a keys-only round; tuples: no counting leaves here
			std::vector<Segment> l_small, l_count, l_big, parents;
			for (auto &sg : cur) {
				Route to = route_child(sg.count, sg.bits, job.stop_bits, HV ? 0u : count_bits, small_max, std::max<uint64_t>(small_max, kCountMedMax), !HV);
				if (to == kRouteDone) continue;
				if (to == kRouteBig && l_big.size() >= big_cap) to = kRouteNext; // the big list is full: a round instead
				(to == kRouteSmall ? l_small : to == kRouteCount ? l_count : to == kRouteBig ? l_big : parents).push_back(sg);
			}
			int rc = lists_reserve(c, std::max(l_small.size(), l_count.size()) + 16, 0, 0);
			if (!rc) rc = pinned_reserve(c, (l_small.size() + l_count.size() + l_big.size()) * sizeof(Segment) + sizeof(Counters));
			if (rc) return rc;
			nsmall_host = (uint32_t)l_small.size();
			ncount_host = (uint32_t)l_count.size();
			nbig_host = (uint32_t)l_big.size();
			Counters hc0 = {}; // the lists' counters continue from here
			hc0.nsmall = nsmall_host;
			hc0.ncount = ncount_host;
			hc0.nbig = nbig_host;
			rc = upload(c, { { small(), l_small.data(), l_small.size() * sizeof(Segment) },
					 { small_count(), l_count.data(), l_count.size() * sizeof(Segment) },
					 { big, l_big.data(), l_big.size() * sizeof(Segment) },
					 { ctr, &hc0, sizeof hc0 } });
			if (rc) return rc;
			cur = parents;
		}
		const bool whole = !job.single_pass() && !job.segmented();
		if constexpr (!HV) { // <= 16 open bits from the start (small key range): no partition round at all
			if (whole && !cur.empty() && n > small_max && cur[0].bits <= count_bits && n < 0xFFFF0000ull) {
				if (int rc = upload(c, { { big, &cur[0], sizeof(Segment) } })) return rc;
				nbig_host = 1;
				cur.clear();
			}
		}
		if (whole && !cur.empty() && n <= small_max) { // fits LDS: no partition round at all
			if (int rc = upload(c, { { small(), &cur[0], sizeof(Segment) } })) return rc;
			nsmall_host = 1;
			cur.clear();
		}
		return MSD_OK;
	}

	// ---- partition rounds until every segment is a leaf (kRestart: a sampled leading-bit skip did not hold)
	int rounds()
	{
		while (!cur.empty() || dev_np) {
			int rc;
			if constexpr (sizeof(K) == 8) {
				// ---- segments that fit the registers of one workgroup take ONE register-resident pass (msd_regpart.hpp) instead
				// of a general round: the last partition round of the tuple sort (65536 parents of about 2^14 tuples at 2^30)
				// (dev_np: the previous round left only parents that fit, and their list stayed on the device -- it is
				// planned there too, regpart_plan_kernel; otherwise the host sorts the fitting parents out of its list)
				if (!job.single_pass() && c->opt.regpart) {
					std::vector<Segment> fit, rest;
					if (!dev_np)
						for (auto &sg : cur) (register_parent(sg) ? fit : rest).push_back(sg);
					if (dev_np || register_pass(fit.size(), cur.size())) {
						if (parked.open) return fail(c, MSD_EINTERNAL, "a register-resident pass behind a round whose summary is parked");
						const uint32_t np = dev_np ? dev_np : (uint32_t)fit.size(); // (dev_np of them on the device: `fit` is empty)
						dev_np = 0;
						// (tuples: such a segment is finished by leaf17_kernel instead, while nothing stands against it)
						if constexpr (HV)
							rc = c->opt.leaf17 && leaf17_ok && !unverified ? leaf17_pass(fit, rest, np) : regpart_round(fit, rest, np);
						else
							rc = regpart_round(fit, rest, np);
						if (rc) return rc;
						continue;
					}
				}
			}
			// ---- the general round: plan + upload, A classify, B block metadata + permutation, C cleanup + collect, summary
			Round r;
			if ((rc = plan_upload(r)) || (rc = classify(r))) return rc;
			choose_end(r);
			if ((rc = permute_blocks(r)) || (rc = cleanup_collect(r))) return rc;
			// an early ending that declines (it says why) has changed nothing: the ordinary summary then
			bool ended = false;
			switch (r.end) {
			case Round::kLeavesFollow: rc = early_summary(r, ended); break;
			case Round::kPlanAhead: rc = plan_next_early(r, ended); break;
			case Round::kOrdinary: break;
			}
			if (!rc && !ended) rc = round_summary(r);
			if (rc) return rc;
		}
		return MSD_OK;
	}

	// ---- the register-pass rule (8-byte keys): a parent that fits the registers of one workgroup and no leaf takes a
	// register-resident pass, if at least kRegPassMin parents of the round do, or all of them
	static constexpr size_t kRegPassMin = 64;
	static bool fits_registers(uint64_t count) { return count + 1 <= kRpCap; }
	static bool register_parent(const Segment &sg) { return fits_registers(sg.count) && sg.count > small_max; }
	static bool register_pass(size_t fit, size_t all) { return fit >= kRegPassMin || (fit && fit == all); }

	// ---- tuples: a segment that fits the registers is FINISHED in one pass by leaf17_kernel (msd_leaf17.hpp: read once, sorted
	// in registers and LDS, written once) instead of a register partition + the small leaves; what it rejects (a group of > 48
	// tuples equal on the counted bits) takes that way.  A leaf must not run behind an unconfirmed leading-bit skip.
	// (segments with <= 16 open bits -- tuples whose upper key half is constant, config 5b -- too: the leaf counts up to
	// 16 bits, such a segment has no groups to put in order at all)
	int leaf17_pass(const std::vector<Segment> &fit, const std::vector<Segment> &rest, const uint32_t np)
	{
		const bool on_device = fit.empty();
		Segment *d_segs = nullptr, *d_rej = nullptr;
		int rc = slab_carve(c, [&](Bump &b) {
			d_segs = b.take<Segment>(np);
			d_rej = b.take<Segment>(np);
		});
		if (!rc) rc = pinned_reserve(c, (size_t)np * sizeof(Segment) + 4096);
		if (rc) return rc;
		if (on_device)
			HIPCHK(c, hipMemcpyAsync(d_segs, dev_list, (size_t)np * sizeof(Segment), hipMemcpyDeviceToDevice, c->stream));
		else if ((rc = upload(c, { { d_segs, fit.data(), (size_t)np * sizeof(Segment) } })))
			return rc;
		HIPCHK(c, hipMemsetAsync(&ctr->nslow2, 0, sizeof(uint32_t), c->stream));
		HIPCHK(c, hipMemsetAsync(&ctr->l17_slow, 0, sizeof(uint32_t), c->stream));
		phase_mark(c, "plan+upload");
		LAUNCH(c, (leaf17_kernel<V>), std::min<uint32_t>(np, (uint32_t)c->sm_count), kL17Th, kL17Lds, keys, vals, d_segs, np, d_rej, &ctr->nslow2, ctr, 0);
		phase_mark(c, "leaf17");
		Counters hc;
		if ((rc = read_counters(c, ctr, hc))) return rc;
		if (hc.errors) return fail(c, MSD_EINTERNAL, "leaf17: %u internal invariant violations (checks 0x%x)", hc.errors, hc.err_sites);
		add_stat(c, kStatLeaf17Segments, np - hc.nslow2);
		add_stat(c, kStatLeaf17SlowSegments, hc.l17_slow);
		cur = rest;
		if (hc.nslow2) { // rejected segments: the register partition + the small leaves finish them
			if ((rc = fetch_segments(c, d_rej, hc.nslow2, cur))) return rc;
			leaf17_ok = false; // (for the rest of this call)
			add_stat(c, kStatLeaf17Rejected, hc.nslow2);
		}
		phase_mark(c, "readback");
		return MSD_OK;
	}

	// ---- the register-resident partition round (msd_regpart.hpp)
	int regpart_round(const std::vector<Segment> &fit, const std::vector<Segment> &rest, const uint32_t np)
	{
		const bool on_device = fit.empty();
		const uint32_t wmax = regpart_width(kRpCap, 64, small_max); // (the widest digit of the rule)
		std::vector<Parent> ps;
		uint32_t nc = 0;
		for (const Segment &sg : fit) {
			const uint32_t w = regpart_width(sg.count, sg.bits, small_max);
			ps.push_back({ sg.start, sg.count, sg.bits - w, w, nc, 0, 0, 0 }); // (shift, width, child_base, no stripes)
			nc += 1u << w;
		}
		if (on_device) nc = np << wmax; // (an upper bound)
		const size_t next_cap = (size_t)nc + 2; // (children above the leaf capacity: none on sane input, all at worst)
		Parent *d_parents = nullptr;
		ChildArrays ca = {};
		Segment *d_next = nullptr;
		uint32_t *d_scr = nullptr;
		int rc = slab_carve(c, [&](Bump &b) {
			d_parents = b.take<Parent>(np);
			ca.start = b.take<uint64_t>(nc);
			ca.count = b.take<uint64_t>(nc);
			d_next = b.take<Segment>(next_cap);
			d_scr = b.take<uint32_t>(64);
		});
		if (!rc) rc = lists_reserve(c, (size_t)std::max(nsmall_host, ncount_host) + nc + 16, nsmall_host, ncount_host);
		if (!rc) rc = pinned_reserve(c, std::max<size_t>(on_device ? 0 : np * sizeof(Parent), offsetof(Staging, sum.early))); // (the counters, the next parents)
		if (rc) return rc;
		LAUNCH(c, round_init_kernel, 1, 256, 0, ctr, d_scr + 16, 0, reinterpret_cast<unsigned long long *>(d_scr + 32), 0, d_scr,
		       nullptr, nullptr, 0, nullptr, 0, nullptr); // (this round's plan is uploaded or made on the device below)
		if (on_device)
			LAUNCH(c, regpart_plan_kernel, (np + 255) / 256, 256, 0, dev_list, np, small_max, d_parents, ctr);
		else if ((rc = upload(c, { { d_parents, ps.data(), np * sizeof(Parent) } })))
			return rc;
		phase_mark(c, "plan+upload");
		LAUNCH(c, (regpart_kernel<V>), std::min<uint32_t>(np, (uint32_t)c->sm_count), kRpTh, kRpLds, keys, vals, d_parents, np, ca, ctr);
		phase_mark(c, "A register partition");
		LAUNCH(c, collect_kernel, (np + (256u >> wmax) - 1) / (256u >> wmax), 256, 0, d_parents, np, wmax, ca, small_max, small_max,
		       std::min<size_t>(c->lists_cap, 0xFFFFFFFFu), count_bits, d_next, small(), small_count(), HV ? nullptr : big, big_cap, ctr,
		       nullptr, nc, job.stop_bits);
		phase_mark(c, "C cleanup");
		Counters hc;
		const size_t ahead = std::min<size_t>(next_cap, kReadAhead); // (next parents that travel with the counters)
		if ((rc = read_counters(c, ctr, hc, { { offsetof(Staging, sum.segs), d_next, ahead * sizeof(Segment) } }))) return rc;
		if (hc.errors) return fail(c, MSD_EINTERNAL, "register partition round: %u internal invariant violations (checks 0x%x)", hc.errors, hc.err_sites);
		adopt(hc, false);
		add_stat(c, kStatRounds, 1);
		add_stat(c, kStatRegpartRounds, 1);
		add_stat(c, kStatParents, np);
		add_stat(c, kStatChildren, nc);
		cur = rest;
		if (hc.next_parents && (rc = fetch_segments(c, d_next, hc.next_parents, cur, staged(offsetof(Staging, sum.segs)), ahead))) return rc;
		next_round();
		return MSD_OK;
	}

	struct Round { // one general round
		RoundPlan rp;
		RoundBufs rb;
		uint32_t np = 0, ns = 0, nc = 0;
		bool tried_direct = false; // a direct placement was attempted (its verdict stays on the device until the summary)
		bool hist_checks = false;  // its exact histogram pass carries the check behind a sampled leading-bit skip
		// how the round ends (choose_end): with round_summary; with early_summary -- by the plan no child can become a parent, the
		// counters travel early and the leaves go behind at once; or with plan_next_early -- the counters and early_segs next
		// parents travel early, for the next round's plan
		enum End { kOrdinary, kLeavesFollow, kPlanAhead } end = kOrdinary;
		size_t early_segs = 0;
	};
	// The pinned staging buffer as the rounds lay it out: `sum` is what an ordinary summary reads; behind it, for a round
	// planned while the one before it still runs (early_plan), the early copy of that round's counters and first next
	// parents, its parked counters once they are read, and a staging region of its own for the plan -- the first one is
	// only free after a synchronisation.
	static constexpr size_t kReadAhead = 2048;
	struct Staging {
		struct Summary {
			Counters ctr; // where read_counters lands the counters: in front of a 256-byte head, the OR / AND words at its end
			char gap[256 - sizeof(Counters) - 2 * sizeof(unsigned long long)];
			unsigned long long vres[2];
			Segment segs[kReadAhead]; // the first next parents
			Counters early;           // the early copy of the counters of a round that the leaves follow
		} sum;
		alignas(256) Counters plan_ctr;             // the early copy of a round that plans ahead: its counters ...
		alignas(256) Segment plan_segs[kReadAhead]; // ... and first next parents
		Counters parked;                            // a parked round's counters (Deferred::kParkSlot)
		alignas(256) char stage2[256];              // where the second staging region starts
	};
	char *staged(size_t at) const { return (char *)c->pinned + at; }
	// (pinned bytes the second staging region needs for a plan)
	static size_t stage2_bytes(size_t np, size_t ns) { return offsetof(Staging, stage2) + np * sizeof(Parent) + ns * sizeof(Stripe); }

	// A round whose summary comes later, because its fix-up was still running when the host went on: to the leaves
	// (early_summary; the summary comes with the leaves' counters, count_leaves) or to the next round (plan_next_early; that
	// round's round_init_kernel parks the counters, and they come with the next readback, parked_piece).  One of each at most.
	struct Deferred {
		enum Source { kLeavesCounters, kParkSlot } source;
		bool open = false;
		int round = 0;
		uint32_t np = 0, ns = 0, nc = 0;
		uint64_t nslots = 0;
		const char *direct = ""; // "direct placement ..." of the message
	};
	Deferred pending = { Deferred::kLeavesCounters }, parked = { Deferred::kParkSlot };
	bool enqueue_ahead = false; // the round being enqueued now goes behind a running one: no synchronisation, no allocation
	Counters *park() const { return ctr + 2; }
	static constexpr uint32_t kCountWalkSites = 1u << kErrBigListFull; // msd_note_error sites in the leaves' counters that are no round's: count_walk_kernel's
	// (behind adopt, ahead of next_round)
	void defer(Deferred &d, const Round &r) { d = { d.source, true, round, r.np, r.ns, r.nc, r.rp.nslots, prev_direct ? "used" : "not used" }; }
	ToHost parked_piece() const { return { offsetof(Staging, parked), park(), parked.open ? sizeof(Counters) : 0 }; }
	// A readback has brought the deferred summary's counters -- `hc` itself, or behind it the park slot's (parked_piece): the
	// round's errors, under its own number and shape, or its statistics
	int settle(Deferred &d, Counters hc)
	{
		if (!d.open) return MSD_OK;
		d.open = false;
		const bool slot = d.source == Deferred::kParkSlot;
		if (slot) memcpy(&hc, staged(offsetof(Staging, parked)), sizeof hc);
		// (a scan tile's time-out leaves no site)
		if (hc.errors && (hc.err_sites & ~(slot ? 0u : kCountWalkSites) || !hc.err_sites)) return round_errors(hc, d.round, d.np, d.ns, d.direct);
		round_stats(hc, d.np, d.ns, d.nc, d.nslots);
		return MSD_OK;
	}
	void plan_next(const std::vector<Segment> &segs, RoundPlan &rp) const
	{
		plan_round<K, V>(segs, small_max, c->sm_count, rp, count_bits, job.single_pass() ? job.width : 0u, job.splitters ? job.nsplit : 0u);
	}
	int plan_upload(Round &r)
	{
		const bool ahead = enqueue_ahead; // (plan_next_early has made sure that nothing below has to grow)
		enqueue_ahead = false;
		plan_next(cur, r.rp);
		// (between rounds nothing in the slab is live; the first round reserves the usual shapes' worst case at once)
		const bool first = round == 0;
		int rc = slab_carve(c, [&](Bump &b) { carve_round<K, V>(b, r.rp, small_max, r.rb); },
				    first && !job.single_pass() ? round_bytes_estimate<K, V>(n, c->sm_count) : 0, first);
		if (rc) return rc;
		r.np = (uint32_t)r.rp.parents.size(), r.ns = (uint32_t)r.rp.stripes.size(), r.nc = r.rp.nchildren;
		// every child of this round may become a leaf
		if ((rc = lists_reserve(c, (size_t)std::max(nsmall_host, ncount_host) + r.nc + 16, nsmall_host, ncount_host))) return rc;
		{ // per-round counters, per-parent plans, scan state, and the plan itself from the staging buffer: one launch
			static_assert(sizeof(Parent) % 4 == 0 && sizeof(Stripe) % 4 == 0, "the plan travels as 32-bit words");
			const uint64_t plan_words = (r.np <= kDirectMaxParents ? r.np : 1) * sizeof(DirectPlan) / sizeof(uint32_t);
			const uint64_t ntiles = (r.nc + kScanTile - 1) / kScanTile + 1;
			const uint64_t parent_words = r.np * sizeof(Parent) / 4, stripe_words = r.ns * sizeof(Stripe) / 4;
			// (with room for the plan of a next round that goes behind this one: at most kReadAhead parents, and about as many
			// stripes as a round of all n keys has, one more per parent)
			const size_t next_stripes = (size_t)std::max<uint64_t>((uint64_t)c->sm_count * MSD_STRIPE_WANT, n >> MSD_STRIPE_CAP_LOG) + 2 * kReadAhead + 64;
			const size_t want = !ahead && c->opt.early_plan && !job.single_pass() ? stage2_bytes(kReadAhead, next_stripes) : 0;
			if ((rc = pinned_reserve(c, std::max({ sizeof(typename Staging::Summary), r.np * sizeof(Parent) + r.ns * sizeof(Stripe), want })))) return rc;
			char *stage = staged(ahead ? offsetof(Staging, stage2) : 0);
			if (!ahead) HIPCHK(c, hipStreamSynchronize(c->stream)); // the staging buffer may still be in flight
			memcpy(stage, r.rp.parents.data(), r.np * sizeof(Parent));
			memcpy(stage + r.np * sizeof(Parent), r.rp.stripes.data(), r.ns * sizeof(Stripe));
			void *staged = nullptr; // (pinned memory is mapped: an error here, never a guess at the address)
			HIPCHK(c, hipHostGetDevicePointer(&staged, c->pinned, 0));
			staged = (char *)staged + (stage - (char *)c->pinned);
			const unsigned grid = (unsigned)std::min<uint64_t>(1024, (std::max({ plan_words, ntiles, parent_words, stripe_words }) + 255) / 256 + 1);
			LAUNCH(c, round_init_kernel, grid, 256, 0, ctr, reinterpret_cast<uint32_t *>(r.rb.plans), plan_words, r.rb.scan_state, ntiles, r.rb.scan_ctr,
			       static_cast<const uint32_t *>(staged), reinterpret_cast<uint32_t *>(r.rb.parents), parent_words,
			       reinterpret_cast<uint32_t *>(r.rb.stripes), stripe_words, ahead ? park() : nullptr);
		}
		phase_mark(c, "plan+upload");
		return MSD_OK;
	}

	// ---- A (direct placement, DESIGN.md section 2, A'): the first round from a sample, later rounds -- only after a direct
	// first round -- from exact counts (a read-only pass).
	// (the read schedule hands a bucket one slot per tile: with fewer than 256 buckets the tiles
	// are not filled, so narrower digits keep the streaming kernel unless forced)
	int classify_direct(Round &r)
	{
		const RoundPlan &rp = r.rp;
		const uint32_t np = r.np, ns = r.ns;
		bool try_direct = c->opt.direct_mode != 0 && rp.round_keys >= c->opt.direct_min && !job.splitters;
		for (size_t i = 0; i < np && try_direct; ++i) try_direct = rp.parents[i].width == 8 || c->opt.direct_mode == 2;
		if (try_direct && np > 1) {
			try_direct = prev_direct && np <= kDirectMaxParents;
			for (size_t i = 0; i < np && try_direct; ++i) try_direct = rp.parents[i].count >= c->opt.direct_min_parent;
		}
		// A workgroup of a direct round reads its pieces, not its stripe: up to one slot per bucket more than
		// the stripe holds.  Its leftovers (< B per bucket + head/tail) must fit the stripe's leftover area,
		// which is capped by the stripe's own size: no direct placement for stripes smaller than that bound.
		for (size_t i = 0; i < ns && try_direct; ++i)
			try_direct = rp.stripes[i].end - rp.stripes[i].begin >= (((uint64_t)1 << rp.parents[rp.stripes[i].parent].width) * (B - 1) + 2 * B);
		uint64_t max_piece = 0; // a piece is at most one stripe's share of its parent's slots; the kernel counts it in 16 bits
		for (size_t i = 0; i < np && try_direct; ++i)
			max_piece = std::max<uint64_t>(max_piece, rp.parents[i].count / B / (rp.parents[i].stripe_hi - rp.parents[i].stripe_lo) + 2);
		// (the front path stands on both rounds being direct and shaped as planned: otherwise the sort goes on from here
		// with the usual readbacks)
		if (front && (round > 1 || np != (round == 0 ? 1u : (uint32_t)kP))) front = false;
		if (!try_direct || max_piece >= 65535) {
			front = false;
			return MSD_OK;
		}
		const RoundBufs &rb = r.rb;
		if (front) {
			// exact counts from the front pass: round 0's are the row sums, round 1's parent d has row d
			LAUNCH(c, front_apply_kernel, np, 256, 0, rb.plans, front_hist(), front_sum(), (uint32_t)round);
		} else if (np == 1) {
			// sample about 2^22 keys or more, as runs of 256 spread evenly over the parent
			const uint64_t nruns = rp.parents[0].count / 256;
			const uint32_t every = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, nruns / 16384));
			const uint32_t sgrid = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, nruns / every / 4));
			LAUNCH(c, (direct_sample_kernel<K>), sgrid, 256, 0, keys, rb.parents, rb.plans, every);
		} else {
			// (the exact check behind a sampled leading-bit skip rides on this pass if it reads every key)
			r.hist_checks = unverified && rp.round_keys == n;
			if (r.hist_checks) {
				if (int rc = vres_init()) return rc;
				add_stat(c, kStatBitSkipCheckedByHistogram, 1);
			}
			LAUNCH(c, (direct_hist_kernel<K>), ns, 1024, 0, keys, rb.stripes, rb.parents, rb.plans, r.hist_checks ? vres : nullptr);
		}
		LAUNCH(c, (direct_plan_kernel<B>), np, 256, 0, rb.parents, rb.plans, ctr);
		phase_mark(c, front ? "A front counts" : np == 1 ? "A sample" : "A histogram");
		// The plan's verdict (Counters::direct_uneven: some parent's children are too unequal, or its keys come in
		// runs) stays on the device: the direct kernel returns at once if it is non-zero, the streaming kernel
		// launched behind it if it is zero.  The host learns it with the round's summary.
		r.tried_direct = true;
		const uint32_t force = c->opt.direct_mode == 2 ? 1u : 0u;
		// (an array beyond the memory-side cache is streamed with the kernel's nontemporal policy: kStreamMinBytes)
		const bool big = (uint64_t)n * (sizeof(K) + (HV ? sizeof(uint64_t) : 0)) >= kStreamMinBytes;
		LAUNCH(c, (big ? classify_direct2_kernel<K, V, true> : classify_direct2_kernel<K, V, false>), ns, (Direct2Cfg<K, V>::TH), (Direct2Lds<K, V>::bytes), keys,
		       vals, rb.stripes, rb.parents, rb.plans, block_map, slot_full, rb.fb, rb.lo_cnt, rb.lo_off, rb.lo_keys, rb.lo_vals, rb.nfull, ctr, force);
		phase_mark(c, "A classify direct");
		return MSD_OK;
	}

	// ---- A: classify (the histogram falls out of it): a direct attempt, and the streaming kernel (msd_stream2.hpp) -- behind
	// a direct attempt it runs only if that declined
	int classify(Round &r)
	{
		if (int rc = classify_direct(r)) return rc;
		if (!r.tried_direct || c->opt.direct_mode != 2) {
			const RoundBufs &rb = r.rb;
			const uint32_t *run_if = r.tried_direct ? &ctr->direct_uneven : nullptr;
			if (job.splitters)
				LAUNCH(c, (classify_stream2_kernel<K, V, true>), r.ns, (Stream2Cfg<K, V>::TH), (Stream2Lds<K, V>::range_bytes), keys, vals, rb.stripes,
				       rb.parents, block_map, rb.fb, rb.lo_cnt, rb.lo_off, rb.lo_keys, rb.lo_vals, rb.nfull, job.splitters, run_if);
			else
				LAUNCH(c, (classify_stream2_kernel<K, V, false>), r.ns, (Stream2Cfg<K, V>::TH), (Stream2Lds<K, V>::bytes), keys, vals, rb.stripes,
				       rb.parents, block_map, rb.fb, rb.lo_cnt, rb.lo_off, rb.lo_keys, rb.lo_vals, rb.nfull, nullptr, run_if);
		}
		phase_mark(c, "A classify");
		return MSD_OK;
	}

	// ---- B: block metadata (child geometry, misplaced-block lists, holes), then the block permutation
	int permute_blocks(Round &r)
	{
		const RoundBufs &rb = r.rb;
		const uint32_t np = r.np, ns = r.ns, nc = r.nc;
		const uint8_t *full_map = r.tried_direct ? slot_full : nullptr;
		const uint32_t force_map = c->opt.direct_mode == 2 ? 1u : 0u;
		if (const uint32_t groups = child_scan_groups(r.rp); groups > 1) {
			LAUNCH(c, child_scan_part_kernel, dim3(np, groups), 256, 0, rb.parents, rb.fb, rb.lo_cnt, rb.scan_part);
			LAUNCH(c, (child_scan_split_kernel<B>), dim3(np, groups), 256, 0, rb.parents, rb.lo_cnt, rb.scan_part, rb.lo_dst, rb.ca);
			add_stat(c, kStatChildScanSplitRounds, 1);
		} else
			LAUNCH(c, (child_scan_kernel<B>), np, 1024, 0, rb.parents, rb.fb, rb.lo_cnt, rb.lo_dst, rb.ca);
		// every child's start and count are final: the children go to the next round or the leaf lists now, so that the
		// host can have the lists' lengths while the fix-up runs
		if (int rc = collect(r)) return rc;
		LAUNCH(c, (slot_classify_kernel<false>), ns * kSlotParts, 256, 0, rb.stripes, rb.parents, block_map, rb.nfull, rb.ca, rb.list, rb.holes, ctr,
		       full_map, force_map);
		LAUNCH(c, list_prepare_kernel, (nc + 255) / 256, 256, 0, nc, rb.ca, ctr, std::min<uint64_t>(r.rp.nslots, 0xFFFFFFFFu), 2 * nc + kMinChains);
		LAUNCH(c, scan_lookback_kernel, (unsigned)((nc + kScanTile - 1) / kScanTile), kScanTh, 0, // (its state: round_init_kernel)
		       rb.ca.list_len, rb.ca.list_base, nc, rb.scan_state, rb.scan_ctr, &ctr->errors);
		LAUNCH(c, (slot_classify_kernel<true>), ns * kSlotParts, 256, 0, rb.stripes, rb.parents, block_map, rb.nfull, rb.ca, rb.list, rb.holes, ctr,
		       full_map, force_map);
		// per child: up to 64 waves when there are few children, one thread when there are very many
		const uint32_t evict_waves = nc > 16384 ? 0u : (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, 16384 / nc));
		const unsigned evict_grid = evict_waves ? (unsigned)(((uint64_t)nc * evict_waves + 3) / 4) : (unsigned)((nc + 255) / 256);
		LAUNCH(c, (evict_kernel<K, V>), evict_grid, 256, 0, nc, rb.ca, rb.list, rb.holes, ctr, keys, vals, rb.xkeys, rb.xvals, evict_waves);
		phase_mark(c, "B metadata");

		// Exactly the workgroups the chip holds at once: a wave's first 64 chain starts are its own by position and the
		// rest come from the cursor as its chains end, so every hole is in the hands of a running wave from the start.
		// (Twice as many workgroups: those of the second half whose share held holes started when the first finished
		// -- 2^30 Zipf keys: 1.3 ms where a wave's own work takes 0.7.)
		const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * c->chains_per_cu[HV ? 2 : sizeof(K) == 8 ? 1 : 0],
								 std::max<uint64_t>(1, (r.rp.nslots + 255) / 256));
		LAUNCH(c, (chains_kernel<K, V>), grid, 256, 0, rb.ca, rb.list, rb.holes, ctr, keys, vals, rb.xkeys, rb.xvals, n / B, 4 * nc + kMinChains);
		phase_mark(c, "B block permute");
		return MSD_OK;
	}

	// Is the average child of some parent too long for a leaf (and, 8-byte keys, for the register-resident pass)?  If not, the
	// round is most likely the last general one and the early copy for the next round's plan would travel for nothing.
	bool may_leave_parents(const Round &r) const
	{
		uint64_t leaf_max = small_max;
		if constexpr (sizeof(K) == 8)
			if (c->opt.regpart) leaf_max = std::max<uint64_t>(leaf_max, kRpCap - 1);
		for (const Parent &p : r.rp.parents)
			if ((p.count >> p.width) > leaf_max) return true;
		return false;
	}

	// ---- the children to the next round or the leaf lists (behind the child scan); a round with an early ending sends
	// a copy of the counters to the host behind it (send_early) -- the kernels behind the copy do not wait for the host
	int collect(Round &r)
	{
		const RoundBufs &rb = r.rb;
		const uint32_t np = r.np, nc = r.nc;
		const bool sp = job.single_pass();
		uint32_t wmax = 1;
		for (size_t i = 0; i < np; ++i) wmax = std::max(wmax, r.rp.parents[i].width);
		const uint32_t small_cap = (uint32_t)std::min<size_t>(c->lists_cap, 0xFFFFFFFFu);
		LAUNCH(c, collect_kernel, (np + (256u >> wmax) - 1) / (256u >> wmax), 256, 0, rb.parents, np, wmax, rb.ca,
		       sp ? ~0ull : small_max, (HV || sp) ? small_max : std::max<uint64_t>(small_max, kCountMedMax),
		       small_cap, sp ? 0u : count_bits,
		       rb.next_parents, small(), small_count(), (HV || sp) ? nullptr : big, big_cap, ctr,
		       (sp && job.counts) ? job.counts : nullptr, job.splitters ? job.nsplit + 1u : nc, job.stop_bits);
		return send_early(r);
	}

	// ---- how the round ends, decided once its plan and its classify pass are known
	void choose_end(Round &r) const
	{
		const bool sp = job.single_pass();
		// A keys-only round in which no parent leaves more open bits than one counting pass takes has no next parents
		// (route_child; a full big list or a child of 2^32 keys would make one: the early counters show it).  Not behind an
		// unconfirmed leading-bit skip: no leaf may run before the check.
		bool leaves_follow = !HV && !sp && !unverified && c->opt.early_leaves;
		for (size_t i = 0; i < r.np && leaves_follow; ++i) leaves_follow = r.rp.parents[i].shift <= count_bits;
		if (leaves_follow)
			r.end = Round::kLeavesFollow;
		else if (c->opt.early_plan && !sp && !r.hist_checks && !parked.open && c->pinned_bytes >= offsetof(Staging, stage2) && may_leave_parents(r)) {
			// a round that may leave parents (one that carries the check behind a sampled bit skip decides about a restart
			// first; one parked round at a time): the counters and the first next parents travel early, so that the host can
			// plan the next round while this one's fix-up runs
			r.end = Round::kPlanAhead;
			r.early_segs = std::min<size_t>(r.rp.round_keys / (small_max + 1) + 2, kReadAhead);
		}
	}

	// ---- the early copy of a round's counters (and of its first early_segs next parents) to its region of the staging buffer,
	// with an event behind it: send_early enqueues it (collect), read_early waits for it.  The front path knows what the copy
	// would say, so nothing is sent and nothing is waited for: round 0 (it plans ahead) leaves the front pass's row sums as
	// next parents and no leaf -- its errors come with its parked counters like everything else; in round 1 (the leaves follow)
	// every child is a counting leaf, as front_plan_kernel has counted them.
	bool early_known(const Round &r) const { return front && round == (r.end == Round::kPlanAhead ? 0 : 1); }
	static size_t early_at(const Round &r) { return r.end == Round::kPlanAhead ? offsetof(Staging, plan_ctr) : offsetof(Staging, sum.early); }
	int send_early(const Round &r)
	{
		if (r.end == Round::kOrdinary || early_known(r)) return MSD_OK;
		if (!c->ev_early) HIPCHK(c, hipEventCreateWithFlags(&c->ev_early, hipEventDisableTiming));
		HIPCHK(c, hipMemcpyAsync(staged(early_at(r)), ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
		if (r.early_segs)
			HIPCHK(c, hipMemcpyAsync(staged(offsetof(Staging, plan_segs)), r.rb.next_parents, r.early_segs * sizeof(Segment), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipEventRecord(c->ev_early, c->stream));
		return MSD_OK;
	}
	int read_early(const Round &r, Counters &hc, std::vector<Segment> *next = nullptr) // (next: the next parents, if all of them travelled)
	{
		hc = {};
		if (early_known(r)) {
			if (r.end == Round::kLeavesFollow)
				hc.ncount = fsum.nroute[kRouteCount + 1];
			else
				hc.next_parents = kP, *next = front_parents();
			return MSD_OK;
		}
		HIPCHK(c, hipEventSynchronize(c->ev_early));
		memcpy(&hc, staged(early_at(r)), sizeof hc);
		if (next && hc.next_parents <= r.early_segs) {
			const Segment *sg = (const Segment *)staged(offsetof(Staging, plan_segs));
			next->assign(sg, sg + hc.next_parents);
		}
		return MSD_OK;
	}

	// ---- C: cleanup (with it: the check that the chains used up every list, the excess blocks)
	int cleanup_collect(Round &r)
	{
		const RoundBufs &rb = r.rb;
		LAUNCH(c, (cleanup_kernel<K, V>), r.ns, 256, 0, rb.stripes, rb.parents, rb.lo_cnt, rb.lo_off, rb.lo_dst, rb.ca, rb.lo_keys, rb.lo_vals, keys, vals,
		       rb.xkeys, rb.xvals, ctr);
		phase_mark(c, "C cleanup");
		return MSD_OK;
	}

	// what a round's counters say once its last kernel has run
	int round_errors(const Counters &hc, int rnd, uint32_t np, uint32_t ns, const char *direct)
	{
		return fail(c, MSD_EINTERNAL, "round %d: %u internal invariant violations (checks 0x%x: bit = site of msd_note_error in csrc/; 0 = a scan tile's look-back timed out; "
					      "%u parents, %u stripes, direct placement %s)",
			    rnd, hc.errors, hc.err_sites, np, ns, direct);
	}
	void round_stats(const Counters &hc, uint32_t np, uint32_t ns, uint32_t nc, uint64_t nslots)
	{
		add_stat(c, kStatRounds, 1);
		add_stat(c, kStatParents, np);
		add_stat(c, kStatStripes, ns);
		add_stat(c, kStatChildren, nc);
		add_stat(c, kStatSlots, nslots);
		add_stat(c, kStatHoles, hc.nholes);
		set_stat(c, kStatChainSteps, hc.chain_steps);
		set_stat(c, kStatExcessBlocks, hc.nexcess);
	}

	// ---- a round's counters have reached the host, early or with its summary: whether it placed directly, and the leaf lists'
	// lengths (regpart_round: a round that tries no direct placement); next_round closes the round on the host
	void adopt(const Counters &hc, bool tried_direct)
	{
		prev_direct = tried_direct && (hc.direct_uneven == 0 || c->opt.direct_mode == 2);
		if (prev_direct) add_stat(c, kStatDirectRounds, 1);
		nsmall_host = hc.nsmall, ncount_host = hc.ncount, nbig_host = hc.nbig;
	}
	void next_round() { phase_mark(c, "readback"), ++round; }

	// ---- a round that is not the last: the next round is planned from the early copy of the counters and the next parents
	// and enqueued behind this round's cleanup while its fix-up still runs; this round's summary is parked.  Declined, with
	// nothing enqueued ahead ...
	int plan_next_early(Round &r, bool &ended)
	{
		Counters hc;
		std::vector<Segment> next;
		if (int rc = read_early(r, hc, &next)) return rc;
		// ... if the round failed a check, or left no parent or more than travelled,
		if (hc.errors || hc.next_parents == 0 || hc.next_parents > r.early_segs) return MSD_OK;
		sort_by_start(next);
		// ... if its next parents take a register-resident pass or stay on the device (rounds(), round_summary),
		if constexpr (sizeof(K) == 8)
			if (c->opt.regpart && register_pass((size_t)std::count_if(next.begin(), next.end(), register_parent), next.size())) return MSD_OK;
		{ // ... or if a buffer of the next round would have to grow (that synchronises)
			RoundPlan rp;
			RoundBufs rb;
			plan_next(next, rp);
			Bump sz(nullptr);
			carve_round<K, V>(sz, rp, small_max, rb);
			if (sz.off + 4096 > c->slab_bytes || (size_t)std::max(hc.nsmall, hc.ncount) + rp.nchildren + 16 > c->lists_cap ||
			    stage2_bytes(rp.parents.size(), rp.stripes.size()) > c->pinned_bytes)
				return MSD_OK;
		}
		adopt(hc, r.tried_direct);
		defer(parked, r);
		enqueue_ahead = true;
		add_stat(c, kStatRoundsPlannedEarly, 1);
		cur = std::move(next);
		next_round();
		ended = true;
		return MSD_OK;
	}

	// ---- the summary of a round that the leaves follow: the lists' lengths from the early copy of the counters, while the
	// round's fix-up still runs; the rest of the summary (errors, holes, chain steps) comes with the leaves' counters
	// (count_leaves).  Declined if the round left a parent after all, or no counting leaf, or failed a check.
	int early_summary(Round &r, bool &ended)
	{
		Counters hc;
		if (int rc = read_early(r, hc)) return rc;
		if (hc.next_parents || hc.ncount == 0 || hc.errors) return MSD_OK;
		adopt(hc, r.tried_direct);
		defer(pending, r);
		add_stat(c, kStatLeavesBehindRound, 1);
		cur.clear();
		next_round();
		ended = true;
		return MSD_OK;
	}

	// ---- round summary + next parents back to the host (which plans the next round): ONE synchronisation; the
	// first kReadAhead next parents travel with the counters (more than that only on the odd input: fetched then)
	int round_summary(Round &r)
	{
		const size_t np_cap = r.rp.round_keys / (small_max + 1) + 2, ahead = job.single_pass() ? 0 : std::min(np_cap, kReadAhead);
		Counters hc;
		int rc = pinned_reserve(c, sizeof(typename Staging::Summary));
		if (rc || (rc = read_counters(c, ctr, hc, { { offsetof(Staging, sum.segs), r.rb.next_parents, ahead * sizeof(Segment) },
							    { offsetof(Staging, sum.vres), vres, r.hist_checks ? 2 * sizeof(unsigned long long) : 0 }, parked_piece() })))
			return rc;
		if ((rc = settle(parked, hc))) return rc;
		if (hc.errors) return round_errors(hc, round, r.np, r.ns, r.tried_direct ? (hc.direct_uneven ? "declined" : "used") : "not tried");
		if (r.hist_checks) {
			const unsigned long long *h = (const unsigned long long *)staged(offsetof(Staging, sum.vres));
			if ((h[0] ^ h[1]) & claimed_const) { // some key differs in a bit the sample found constant
				exact_vary = h[0] ^ h[1];
				phase_mark(c, "readback");
				return kRestart;
			}
			unverified = false;
		}
		adopt(hc, r.tried_direct);
		round_stats(hc, r.np, r.ns, r.nc, r.rp.nslots);
		cur.clear();
		if (job.single_pass()) return MSD_OK;
		bool stays_on_device = false;
		if constexpr (sizeof(K) == 8) {
			// every next parent fits a workgroup's registers, and they are enough for a pass (rounds()): the list stays on the
			// device and is planned there
			if (c->opt.regpart && hc.next_parents >= kRegPassMin && fits_registers(hc.next_max)) {
				HIPCHK(c, hipMemcpyAsync(dev_list, r.rb.next_parents, (size_t)hc.next_parents * sizeof(Segment), hipMemcpyDeviceToDevice, c->stream));
				dev_np = hc.next_parents;
				stays_on_device = true;
			}
		}
		if (hc.next_parents && !stays_on_device &&
		    (rc = fetch_segments(c, r.rb.next_parents, hc.next_parents, cur, staged(offsetof(Staging, sum.segs)), ahead)))
			return rc;
		next_round();
		return MSD_OK;
	}

	// ---- no round's histogram pass carried the exact check behind a sampled skip: a pass of its own, before any leaf runs
	int verify_skip()
	{
		if (!unverified) return MSD_OK;
		uint64_t vary = 0;
		if (int rc = run_vary(1, &vary)) return rc;
		phase_mark(c, "bit skip");
		if (vary & claimed_const) {
			exact_vary = vary;
			return kRestart;
		}
		unverified = false;
		return MSD_OK;
	}

	// ---- the check behind a sampled skip failed: the sort starts over on the bits that really vary (exact_vary)
	int start_over()
	{
		const uint64_t vary = exact_vary & low_mask;
		const int top = vary ? 64 - __builtin_clzll(vary) : 0;
		set_stat(c, kStatSkippedBits, (uint64_t)(end_bit - top));
		add_stat(c, kStatBitSkipRestarts, 1);
		cur.clear();
		if (top > 0 && (uint32_t)top > job.stop_bits) cur.push_back({ 0, n, (uint32_t)top, 0 });
		nsmall_host = ncount_host = nbig_host = dev_np = 0;
		round = 0;
		pending.open = parked.open = enqueue_ahead = false;
		prev_direct = unverified = front = false;
		HIPCHK(c, hipMemsetAsync(ctr, 0, sizeof(Counters), c->stream));
		return MSD_OK;
	}

	// ---- leaves, stage 1: one unstable counting pass over all remaining bits (one workgroup per segment)
	int count_leaves()
	{
		if constexpr (!HV) {
			if (!ncount_host || job.single_pass()) return MSD_OK;
			// persistent workgroups (two per CU fit the LDS), segments handed out by ticket; what the fast
			// kernel cannot place directly is queued (in the round slab, dead by now) for the walking kernel
			Segment *slow = nullptr, *rej16 = nullptr, *slow2 = nullptr;
			int rc = slab_carve(c, [&](Bump &b) {
				slow = b.take<Segment>(ncount_host);
				rej16 = b.take<Segment>(ncount_host);
				slow2 = b.take<Segment>(ncount_host);
			});
			if (rc) return rc;
			const uint32_t count_grid = std::min<uint32_t>(ncount_host, (uint32_t)c->sm_count * 2);
			// u32 keys with 16 open bits (what the planner aims for): the specialised kernel first, the general one
			// takes what that leaves (other bit counts, long or crowded segments)
			// (it pays for segments of about 2^14 keys -- 2^30-key inputs; on shorter ones the per-segment work on the
			// 2^16 counters dominates and 1024-thread workgroups hide its latency better: 1.15 vs 1.44 ms at 2^28)
			const bool c16 = sizeof(K) == 4 && (c->opt.count16 == 2 || (c->opt.count16 == 1 && n / ncount_host >= 12000));
			if constexpr (sizeof(K) == 4)
				if (c16) LAUNCH(c, ((uint64_t)n * sizeof(K) >= kStreamMinBytes ? count_place16_kernel<true> : count_place16_kernel<false>), count_grid, kC16Th, kC16Lds, keys, small_count(), ncount_host, rej16, ctr, n);
			LAUNCH(c, (count_place_kernel<K>), count_grid, kCountTh, kCountLds, keys, c16 ? rej16 : small_count(), c16 ? 0u : ncount_host,
			       c16 ? &ctr->nslow16 : nullptr, slow, ctr);
			const uint32_t *walk_n = &ctr->nslow;
			const Segment *walk_list = slow;
			if constexpr (sizeof(K) == 4) {
				// What the register-resident kernels left -- segments of 17 Ki .. 128 Ki keys (the mid-size buckets of skewed
				// inputs), crowded ones -- takes the 16-bit-counter leaf (msd_merge16.hpp, list mode: one workgroup per
				// segment, all of it counted before the first key is written back, so the sort is in place); only what that
				// does not take either (a key with >= 2^16 copies, a 256-value group with >= 2^16 keys) walks its counters.
				if (c->opt.mid_leaf) {
					LAUNCH(c, (merge_count_kernel<true>), std::min<uint32_t>(ncount_host, (uint32_t)c->sm_count), kMcTh, kMcLds, keys, keys, nullptr,
					       nullptr, nullptr, 0, 0, 0, 0, slow, &ctr->nslow, slow2, &ctr->nslow2, &ctr->count_ticket4, nullptr);
					walk_n = &ctr->nslow2;
					walk_list = slow2;
				}
			}
			LAUNCH(c, (count_walk_kernel<K>), count_grid, kCountTh, kCountLds, keys, walk_list, walk_n, small(), nsmall_host, small_max, big, big_cap, ctr);
			phase_mark(c, "count sort");
			// byte-counter overflows of segments above the LDS-sort capacity joined the big list
			Counters hc;
			// (the last round's summary travels with the leaves' counters: early_summary)
			if ((rc = read_counters(c, ctr, hc, { parked_piece() })) || (rc = settle(parked, hc)) || (rc = settle(pending, hc))) return rc;
			if (hc.errors) return fail(c, MSD_EINTERNAL, "counting leaf: %u segments could not be queued", hc.errors);
			set_stat(c, kStatCount16Rejected, hc.nslow16);     // segments count_place16_kernel left to count_place_kernel
			set_stat(c, kStatCountSlowSegments, hc.nslow);     // segments the register-resident kernels left to the 16-bit-counter leaf / the walk
			nbig_host = hc.nbig;
			nfallback_known = hc.nfallback;
		}
		return MSD_OK;
	}

	// ---- keys-only segments of any size with <= 16 open bits: multi-workgroup counting sort
	int big_count_sort()
	{
		if constexpr (!HV) {
			if (!nbig_host || job.single_pass()) return MSD_OK;
			std::vector<Segment> bs;
			int rc = fetch(c, big, nbig_host, bs);
			if (rc) return rc;
			const uint32_t batch_max = 4096; // 256 KiB of histogram per segment: 1 GiB per batch
			for (uint32_t b0 = 0; b0 < nbig_host; b0 += batch_max) {
				const uint32_t nb = std::min(batch_max, nbig_host - b0);
				// work items -> segments: first[i] = index of segment i's first histogram chunk / group of output tiles
				constexpr uint32_t tile_elems = big_tile_elems<K>() * kBigGroup;
				std::vector<uint32_t> first(2 * ((size_t)nb + 1));
				uint32_t *first_chunk = first.data(), *first_tile = first.data() + nb + 1;
				uint64_t nchunks = 0, ntiles = 0;
				for (uint32_t i = 0; i < nb; ++i) {
					first_chunk[i] = (uint32_t)nchunks;
					first_tile[i] = (uint32_t)ntiles;
					nchunks += (bs[b0 + i].count + kBigChunk - 1) / kBigChunk;
					ntiles += (bs[b0 + i].count + tile_elems - 1) / tile_elems;
				}
				first_chunk[nb] = (uint32_t)nchunks;
				first_tile[nb] = (uint32_t)ntiles;
				uint32_t *ghist = nullptr, *d_first = nullptr;
				K *seg_hi = nullptr;
				uint16_t *tile_v = nullptr;
				rc = slab_carve(c, [&](Bump &b) { // (the round slab is dead by now)
					ghist = b.take<uint32_t>((size_t)nb * 65536);
					seg_hi = b.take<K>(nb);
					d_first = b.take<uint32_t>(first.size());
					tile_v = b.take<uint16_t>(ntiles * kBigGroup + nb + 8);
				});
				if (!rc) rc = pinned_reserve(c, first.size() * sizeof(uint32_t));
				if (!rc) rc = upload(c, { { d_first, first.data(), first.size() * sizeof(uint32_t) } });
				if (rc) return rc;
				HIPCHK(c, hipMemsetAsync(ghist, 0, (size_t)nb * 65536 * sizeof(uint32_t), c->stream));
				LAUNCH(c, (bigcount_hist_kernel<K>), (unsigned)std::min<uint64_t>(nchunks, (uint64_t)c->sm_count), kBigHistTh, kBigHistLds, keys, big + b0,
				       d_first, nb, ghist);
				LAUNCH(c, (bigcount_scan_kernel<K>), nb, 1024, 0, keys, big + b0, d_first + nb + 1, ghist, seg_hi, tile_v, ctr);
				LAUNCH(c, (bigcount_write_kernel<K>), (unsigned)ntiles, kBigWriteTh, kBigWriteLds, keys, big + b0, d_first + nb + 1, nb, ghist, seg_hi, tile_v);
			}
			phase_mark(c, "big count sort");
			Counters hc;
			if ((rc = read_counters(c, ctr, hc))) return rc;
			if (hc.errors) return fail(c, MSD_EINTERNAL, "counting sort: %u histogram totals disagree with segment sizes", hc.errors);
		}
		return MSD_OK;
	}

	// ---- leaves, stage 2: everything else that fits LDS (payloads, > 16 open bits): counting leaf on the
	// top varying bits; its rare failures (long groups of equal top bits) and the byte-counter overflows
	// of stage 1 go to the general LDS sort (their number is only known on the device)
	int lds_leaves()
	{
		if (job.single_pass()) return MSD_OK;
		// persistent workgroups with prefetch of the next segment: as many per CU as the LDS holds
		constexpr size_t leaf_lds = LeafCountLds<K, V>::bytes;
		const uint32_t leaf_per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(2048 / C::SORT_TH, (160 * 1024) / (leaf_lds + 512)));
		const auto leaf_grid = [&](uint32_t nsegs) { return std::min<uint32_t>(nsegs, (uint32_t)c->sm_count * leaf_per_cu); };
		bool small_done = false;
		if constexpr (!HV && sizeof(K) == 8) {
			// u64 keys, segments of about 2^14 (what two 8-bit rounds leave of 2^30 keys): leaf17_kernel -- counters for up to
			// 16 bits where the staging buffer will be, one lane per group of equal counted bits -- finishes a segment in 0.6
			// of this leaf's time; what it leaves (segments shorter than 4096 keys, a group of more than 48) goes on to it.
			if (c->opt.leaf17 && nsmall_host && n / nsmall_host >= 8192) {
				Segment *d_rej = nullptr;
				if (int rc = slab_carve(c, [&](Bump &b) { d_rej = b.take<Segment>(nsmall_host); })) return rc;
				HIPCHK(c, hipMemsetAsync(&ctr->nslow2, 0, sizeof(uint32_t), c->stream));
				HIPCHK(c, hipMemsetAsync(&ctr->l17_slow, 0, sizeof(uint32_t), c->stream));
				LAUNCH(c, (leaf17_kernel<NoVal>), std::min<uint32_t>(nsmall_host, (uint32_t)c->sm_count), kL17Th, kL17Lds, keys, nullptr, small(), nsmall_host,
				       d_rej, &ctr->nslow2, ctr, 4096);
				LAUNCH(c, (leaf_count_sort_kernel<K, V>), leaf_grid(nsmall_host), C::SORT_TH, leaf_lds, keys, vals, d_rej, nsmall_host, small() + nsmall_host,
				       ctr, &ctr->leaf_ticket[0], &ctr->nslow2);
				add_stat(c, kStatLeaf17Launches, 1);
				small_done = true;
			}
		}
		if (nsmall_host && !small_done)
			LAUNCH(c, (leaf_count_sort_kernel<K, V>), leaf_grid(nsmall_host), C::SORT_TH, leaf_lds, keys, vals, small(), nsmall_host, small() + nsmall_host, ctr,
			       &ctr->leaf_ticket[0], nullptr);
		if (HV && ncount_host) // (tuples whose last <= 16 bits are open -- 5b after its rounds: same kernel, its own ticket)
			LAUNCH(c, (leaf_count_sort_kernel<K, V>), leaf_grid(ncount_host), C::SORT_TH, leaf_lds, keys, vals, small_count(), ncount_host, small() + nsmall_host,
			       ctr, &ctr->leaf_ticket[1], nullptr);
		// (keys only, no small segments, and the counting leaves are known to have handed nothing on: no launch -- 2^30 uniform
		// u32 keys: 0.03 ms for workgroups that look at an empty list)
		const bool may_fall_back = HV || nsmall_host != 0 || nfallback_known != 0;
		if (may_fall_back && nsmall_host + ncount_host)
			LAUNCH(c, (lds_sort_kernel<K, V>), std::min<uint32_t>(nsmall_host + ncount_host, 2 * c->sm_count), C::SORT_TH, (SortLds<K, V>::bytes), keys, vals,
			       small() + nsmall_host, 0, &ctr->nfallback);
		phase_mark(c, "LDS sort");
		return MSD_OK;
	}
};

} // namespace

template <typename K, typename V>
static int sort_impl(msd_ctx *c, K *keys, uint64_t *vals, uint64_t n, int end_bit, const SortJob<K> &job)
{
	constexpr bool HV = has_val<V>::value;
	if (n == 0) return MSD_OK;
	if (!keys || (HV && !vals)) return fail(c, MSD_EINVAL, "null data pointer");
	if (!aligned16(keys) || (HV && !aligned16(vals)))
		return fail(c, MSD_EINVAL, "keys/rids must be 16-byte aligned (the reference asserts the same, src/msb_64.c:2273)");
	if (end_bit < 0 || end_bit > (int)sizeof(K) * 8) return fail(c, MSD_EINVAL, "end_bit out of range");
	if (n >= ((uint64_t)1 << 36)) return fail(c, MSD_EINVAL, "n too large for 32-bit block slots");
	HIPCHK(c, hipSetDevice(c->device));
	c->stat_written = 0;
	phase_begin(c);
	SortRun<K, V> s(c, keys, vals, n, end_bit, job);
	int rc = s.initial_segments();
	if (!rc) rc = s.reserve_keep();
	if (!rc) rc = s.front_count();
	if (!rc && !s.front) rc = s.skip_leading_bits(); // (the front pass has the exact OR / AND: no whole leading digit is constant)
	if (!rc) rc = s.route_to_leaves();
	// the partition rounds; if the exact check behind a sampled leading-bit skip fails -- on a round's histogram pass or on
	// a pass of its own behind the rounds -- they start over on the bits that really vary (the data is the same multiset)
	while (!rc) {
		rc = s.rounds();
		if (!rc) rc = s.verify_skip();
		if (rc != kRestart) break;
		rc = s.start_over();
	}
	if (!rc) rc = s.count_leaves();
	if (!rc) rc = s.big_count_sort();
	if (rc) return rc;
	set_stat(c, kStatBigCountSegments, s.nbig_host);
	if ((rc = s.lds_leaves())) return rc;
	set_stat(c, kStatCountSegments, s.ncount_host);
	set_stat(c, kStatSmallSegments, s.nsmall_host);
	set_stat(c, kStatWorkspaceBytes, c->slab_bytes + c->keep_bytes + 4 * c->lists_cap * sizeof(Segment));
	phase_end(c);
	return MSD_OK;
}

// what msd_reserve() provides for n elements
template <typename K, typename V> static int reserve_for(msd_ctx *c, uint64_t n)
{
	int rc = slab_reserve(c, round_bytes_estimate<K, V>(n, c->sm_count), true);
	if (!rc) rc = keep_reserve(c, keep_bytes_for<K, V>(n), true);
	if (!rc) rc = pinned_reserve(c, 1 << 20);
	if (!rc) rc = lists_reserve(c, leaf_list_guess<K, V>(n), 0, 0, true);
	return rc;
}

// (key_bytes, val_bytes) -> the element layout: f(K(), V()), or kNoLayout (not an MSD_ code) where there is none
constexpr int kNoLayout = 1;
template <typename F> static int with_layout(int key_bytes, int val_bytes, F &&f)
{
	if (key_bytes == 4 && val_bytes == 0) return f(uint32_t(), NoVal());
	if (key_bytes == 8 && val_bytes == 0) return f(uint64_t(), NoVal());
	if (key_bytes == 8 && val_bytes == 8) return f(uint64_t(), uint64_t());
	return kNoLayout;
}

// ---- the entry points' jobs (the C ABI below: one instance per element type)
template <typename K, typename V> static int sort_bits(msd_ctx *c, K *k, uint64_t *r, uint64_t n, int end_bit)
{
	if (!c) return MSD_EINVAL;
	return sort_impl<K, V>(c, k, r, n, end_bit, SortJob<K>::whole());
}
template <typename K, typename V> static int partition(msd_ctx *c, K *k, uint64_t *r, uint64_t n, unsigned shift, unsigned rb, uint64_t *cnt)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	if (cnt && rb <= 8) HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(uint64_t) << rb, c->stream));
	return sort_impl<K, V>(c, k, r, n, (int)sizeof(K) * 8, SortJob<K>::digit(shift, rb, cnt));
}
// a sort that stops early: afterwards the keys are ordered by key >> begin_bit
template <typename K, typename V> static int sort_top(msd_ctx *c, K *k, uint64_t *r, uint64_t n, int end_bit, int begin_bit)
{
	if (!c) return MSD_EINVAL;
	if (begin_bit < 0 || begin_bit > end_bit) return fail(c, MSD_EINVAL, "begin_bit must lie in [0, end_bit]");
	return sort_impl<K, V>(c, k, r, n, end_bit, SortJob<K>::whole((uint32_t)begin_bit));
}
template <typename K, typename V>
static int sort_segments(msd_ctx *c, K *k, uint64_t *r, uint64_t n, const uint64_t *seg_off, uint32_t nseg, int end_bit)
{
	if (!c) return MSD_EINVAL;
	if (nseg == 0) return MSD_OK;
	if (!seg_off) return fail(c, MSD_EINVAL, "segments: null offsets");
	return sort_impl<K, V>(c, k, r, n, end_bit, SortJob<K>::offsets(seg_off, nseg));
}

// the most dynamic LDS `kernel` is launched with
template <typename F> static hipError_t max_lds(F *kernel, size_t bytes)
{
	return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// the two row kernels (msd_topk_rows, msd_sort_rows): every K x IDX x LANES instance
template <typename K, bool IDX, int LANES> static int set_row_kernels_lds_attrs_for(msd_ctx *c)
{
	HIPCHK(c, max_lds(&topk_rows_kernel<K, IDX, LANES>, RowsLds<K, IDX, LANES>::bytes));
	HIPCHK(c, max_lds(&sort_rows_kernel<K, IDX, LANES>, SortRowsLds<K, IDX, LANES>::bytes));
	return MSD_OK;
}
static int set_row_kernels_lds_attrs(msd_ctx *c)
{
	int rc = MSD_OK;
	for (const int key_bytes : { 4, 8 })
		for (const bool with_idx : { false, true })
			for (const int lanes_per_row : { 64, 256, 1024 })
				if (!rc) rc = with_width(key_bytes, [&](auto k0) {
					return with_flag(with_idx, [&](auto idx) {
						return with_lanes(lanes_per_row, [&](auto lanes) { return set_row_kernels_lds_attrs_for<decltype(k0), decltype(idx)::value, decltype(lanes)::value>(c); });
					});
				});
	return rc;
}

template <typename K, typename V> static int set_lds_attrs(msd_ctx *c)
{
	{ // the block permutation is launched with exactly the workgroups the chip holds at once (see chains_grid)
		int per_cu = 0;
		HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, chains_kernel<K, V>, 256, 0));
		c->chains_per_cu[has_val<V>::value ? 2 : sizeof(K) == 8 ? 1 : 0] = std::max(1, per_cu);
	}
	HIPCHK(c, max_lds(&classify_stream2_kernel<K, V, false>, Stream2Lds<K, V>::bytes));
	HIPCHK(c, max_lds(&classify_stream2_kernel<K, V, true>, Stream2Lds<K, V>::range_bytes));
	HIPCHK(c, max_lds(&lds_sort_kernel<K, V>, SortLds<K, V>::bytes));
	HIPCHK(c, max_lds(&classify_direct2_kernel<K, V, false>, Direct2Lds<K, V>::bytes));
	HIPCHK(c, max_lds(&classify_direct2_kernel<K, V, true>, Direct2Lds<K, V>::bytes));
	if constexpr (sizeof(K) == 8) {
		HIPCHK(c, max_lds(&regpart_kernel<V>, kRpLds));
		HIPCHK(c, max_lds(&leaf17_kernel<V>, kL17Lds));
	}
	HIPCHK(c, max_lds(&leaf_count_sort_kernel<K, V>, LeafCountLds<K, V>::bytes));
	if constexpr (!has_val<V>::value) {
		if constexpr (sizeof(K) == 4) {
			HIPCHK(c, max_lds(&front_count16_kernel<K>, kF16Lds));
			HIPCHK(c, max_lds(&count_place16_kernel<false>, kC16Lds));
			HIPCHK(c, max_lds(&count_place16_kernel<true>, kC16Lds));
			HIPCHK(c, max_lds(&merge_place16_kernel<2>, kC16Lds));
			HIPCHK(c, max_lds(&merge_place16_kernel<4>, kC16Lds));
			HIPCHK(c, max_lds(&merge_place16_kernel<8>, kC16Lds));
			HIPCHK(c, max_lds(&merge_count_kernel<false, uint32_t>, kMcLds));
			HIPCHK(c, max_lds(&merge_count_kernel<false, uint16_t>, kMcLds));
			HIPCHK(c, max_lds(&merge_count_kernel<false, Hist2>, kMcLds));
			HIPCHK(c, max_lds(&hist2_pack_kernel<uint32_t>, kH2Lds));
			HIPCHK(c, max_lds(&hist2_pack_kernel<uint16_t>, kH2Lds));
			HIPCHK(c, max_lds(&scatter_low16_kernel, kS16Lds));
			HIPCHK(c, max_lds(&merge_count_kernel<true, uint32_t>, kMcLds));
		}
		HIPCHK(c, max_lds(&count_place_kernel<K>, kCountLds));
		HIPCHK(c, max_lds(&count_walk_kernel<K>, kCountLds));
		HIPCHK(c, max_lds(&bigcount_hist_kernel<K>, kBigHistLds));
		HIPCHK(c, max_lds(&bigcount_write_kernel<K>, kBigWriteLds));
	}
	return MSD_OK;
}

template <typename K>
static int gather_impl(msd_ctx *c, K *dst, const K *src, const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, uint32_t nruns)
{
	if (!c) return MSD_EINVAL;
	if (nruns == 0) return MSD_OK;
	if (!dst || !src || !src_off || !dst_off || !len) return fail(c, MSD_EINVAL, "gather: null pointer");
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<GatherRun> runs;
	uint64_t nchunks = 0;
	for (uint32_t i = 0; i < nruns; ++i) {
		if (!len[i]) continue;
		runs.push_back({ src_off[i], dst_off[i], len[i], (uint32_t)nchunks, 0 });
		nchunks += (len[i] + kGatherChunk - 1) / kGatherChunk;
	}
	if (runs.empty()) return MSD_OK;
	if (nchunks >= 0xFFFFFFFFull) return fail(c, MSD_EINVAL, "gather: too many elements");
	runs.push_back({ 0, 0, 0, (uint32_t)nchunks, 0 }); // sentinel
	const size_t nreal = runs.size() - 1, ncoarse = (size_t)(nchunks >> 6) + 2;
	std::vector<uint32_t> coarse(ncoarse); // the run of every 64th chunk
	for (size_t i = 0, r = 0; i < ncoarse; ++i) {
		const uint64_t ch = std::min<uint64_t>((uint64_t)i << 6, nchunks - 1);
		while (r + 1 < nreal && runs[r + 1].first_chunk <= ch) ++r;
		coarse[i] = (uint32_t)r;
	}
	// (one block, the runs in front of the coarse index, so that one copy takes both to the device)
	const size_t runs_bytes = align_up(runs.size() * sizeof(GatherRun), 256), bytes = runs_bytes + ncoarse * sizeof(uint32_t);
	std::vector<char> block(bytes);
	memcpy(block.data(), runs.data(), runs.size() * sizeof(GatherRun));
	memcpy(block.data() + runs_bytes, coarse.data(), ncoarse * sizeof(uint32_t));
	char *d_block = nullptr;
	int rc = pinned_reserve(c, bytes);
	if (!rc) rc = slab_carve(c, [&](Bump &b) { d_block = b.take<char>(bytes); }); // (between sorts nothing in the slab is live)
	if (!rc) rc = upload(c, { { d_block, block.data(), bytes } });
	if (rc) return rc;
	const GatherRun *d_runs = reinterpret_cast<const GatherRun *>(d_block);
	const uint32_t *d_coarse = reinterpret_cast<const uint32_t *>(d_block + runs_bytes);
	// (one workgroup per 8 KiB chunk, no loop: 4.3-4.5 TB/s; persistent workgroups with larger chunks: 3.6)
	const unsigned grid = (unsigned)nchunks;
	LAUNCH(c, (gather_runs_kernel<K>), grid, 256, 0, dst, src, d_runs, runs.size() - 1, nchunks, d_coarse);
	return MSD_OK;
}

// ------------------------------------------------------------------ C ABI

extern "C" {

const char *msd_version(void) { return MSD_VERSION; }

int msd_create(msd_ctx **out, int device, void *stream)
{
	if (!out) return MSD_EINVAL;
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MSD_EHIP; // no CPU fallback exists
	if (device < 0 || device >= ndev) return MSD_EINVAL;
	msd_ctx *c = new msd_ctx();
	c->device = device;
	c->stream = (hipStream_t)stream;
	if (hipSetDevice(device) != hipSuccess) {
		delete c;
		return MSD_EHIP;
	}
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->sm_count = prop.multiProcessorCount;
	// A/B switches for benchmarks: the same knobs as msd_set_option, through the same range checks (an out-of-range
	// value is reported and ignored)
	for (const OptionEntry &e : kOptions) {
		const char *v = e.env ? getenv(e.env) : nullptr;
		if (!v) continue;
		char *end = nullptr;
		const long x = strtol(v, &end, 10);
		if (end == v || *end || msd_set_option(c, e.name, x) != MSD_OK) fprintf(stderr, "msd_create: ignoring %s=%s\n", e.env, v);
	}
	const auto attrs = [c](auto k, auto v) { return set_lds_attrs<decltype(k), decltype(v)>(c); };
	int rc = with_layout(4, 0, attrs);
	if (!rc) rc = with_layout(8, 0, attrs);
	if (!rc) rc = with_layout(8, 8, attrs);
	if (!rc) rc = set_row_kernels_lds_attrs(c);
	if (!rc && hipMalloc((void **)&c->fix_plan, kFixWords * sizeof(uint64_t)) != hipSuccess) rc = fail(c, MSD_ENOMEM, "plan words hipMalloc failed");
	if (rc) {
		fprintf(stderr, "msd_create: %s\n", c->err.c_str());
		delete c;
		return rc;
	}
	*out = c;
	return MSD_OK;
}

int msd_destroy(msd_ctx *c)
{
	if (!c) return MSD_EINVAL;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	if (c->slab) (void)hipFree(c->slab);
	if (c->keep) (void)hipFree(c->keep);
	if (c->lists) (void)hipFree(c->lists);
	if (c->sel) (void)hipFree(c->sel);
	if (c->rows_stage) (void)hipFree(c->rows_stage);
	if (c->fix_plan) (void)hipFree(c->fix_plan);
	if (c->pinned) (void)hipHostFree(c->pinned);
	if (c->ev_start) (void)hipEventDestroy(c->ev_start);
	if (c->ev_early) (void)hipEventDestroy(c->ev_early);
	for (auto e : c->ev_pool) (void)hipEventDestroy(e);
	delete c;
	return MSD_OK;
}

int msd_set_stream(msd_ctx *c, void *stream)
{
	if (!c) return MSD_EINVAL;
	c->stream = (hipStream_t)stream;
	return MSD_OK;
}

void *msd_get_stream(const msd_ctx *c) { return c ? (void *)c->stream : nullptr; }
int msd_get_device(const msd_ctx *c) { return c ? c->device : -1; }

int msd_reserve(msd_ctx *c, uint64_t n, int key_bytes, int val_bytes)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	const int rc = with_layout(key_bytes, val_bytes, [&](auto k, auto v) { return reserve_for<decltype(k), decltype(v)>(c, n); });
	return rc != kNoLayout ? rc : fail(c, MSD_EINVAL, "unsupported element layout %d+%d bytes", key_bytes, val_bytes);
}

uint64_t msd_workspace_bytes(const msd_ctx *c) { return c ? c->slab_bytes + c->keep_bytes + 4 * c->lists_cap * sizeof(Segment) + c->sel_bytes + c->rows_stage_bytes : 0; }
const char *msd_last_error(const msd_ctx *c) { return c ? c->err.c_str() : "null context"; }

int msd_sort_u32_bits(msd_ctx *c, uint32_t *k, uint64_t n, int end_bit) { return sort_bits<uint32_t, NoVal>(c, k, nullptr, n, end_bit); }
int msd_sort_u64_bits(msd_ctx *c, uint64_t *k, uint64_t n, int end_bit) { return sort_bits<uint64_t, NoVal>(c, k, nullptr, n, end_bit); }
int msd_sort_pairs_u64_bits(msd_ctx *c, uint64_t *k, uint64_t *r, uint64_t n, int end_bit) { return sort_bits<uint64_t, uint64_t>(c, k, r, n, end_bit); }
int msd_sort_u32(msd_ctx *c, uint32_t *k, uint64_t n) { return msd_sort_u32_bits(c, k, n, 32); }
int msd_sort_u64(msd_ctx *c, uint64_t *k, uint64_t n) { return msd_sort_u64_bits(c, k, n, 64); }
int msd_sort_pairs_u64(msd_ctx *c, uint64_t *k, uint64_t *r, uint64_t n) { return msd_sort_pairs_u64_bits(c, k, r, n, 64); }

int msd_partition_u32(msd_ctx *c, uint32_t *k, uint64_t n, unsigned shift, unsigned rb, uint64_t *cnt) { return partition<uint32_t, NoVal>(c, k, nullptr, n, shift, rb, cnt); }
int msd_partition_u64(msd_ctx *c, uint64_t *k, uint64_t n, unsigned shift, unsigned rb, uint64_t *cnt) { return partition<uint64_t, NoVal>(c, k, nullptr, n, shift, rb, cnt); }
int msd_partition_pairs_u64(msd_ctx *c, uint64_t *k, uint64_t *r, uint64_t n, unsigned shift, unsigned rb, uint64_t *cnt) { return partition<uint64_t, uint64_t>(c, k, r, n, shift, rb, cnt); }

// ---- a sort that stops early: afterwards the keys are ordered by key >> begin_bit (the top-digit passes of a rank of the
// multi-GPU sort before its exchange; keys that agree above begin_bit may be in any order)
int msd_sort_u32_top(msd_ctx *c, uint32_t *k, uint64_t n, int end_bit, int begin_bit) { return sort_top<uint32_t, NoVal>(c, k, nullptr, n, end_bit, begin_bit); }
int msd_sort_u64_top(msd_ctx *c, uint64_t *k, uint64_t n, int end_bit, int begin_bit) { return sort_top<uint64_t, NoVal>(c, k, nullptr, n, end_bit, begin_bit); }
int msd_sort_pairs_u64_top(msd_ctx *c, uint64_t *k, uint64_t *r, uint64_t n, int end_bit, int begin_bit) { return sort_top<uint64_t, uint64_t>(c, k, r, n, end_bit, begin_bit); }

} // extern "C"

template <typename K>
static int bounds_impl(msd_ctx *c, const K *k, uint64_t n, unsigned shift, uint64_t first, uint32_t nbuckets, uint64_t *bounds)
{
	if (!c) return MSD_EINVAL;
	if (!bounds || (n && !k)) return fail(c, MSD_EINVAL, "bucket_bounds: null pointer");
	if (shift >= sizeof(K) * 8 || nbuckets == 0 || nbuckets > (1u << 24)) return fail(c, MSD_EINVAL, "bucket_bounds: shift or bucket count out of range");
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, (bucket_bounds_kernel<K>), (nbuckets + 1 + 255) / 256, 256, 0, k, n, shift, first, nbuckets, bounds);
	return MSD_OK;
}

// The counting leaf of a rank after a fine-grained exchange (msd_merge16.hpp): every bucket = nsrc extents in d_src.
template <typename IN>
static int merge_impl(msd_ctx *c, const IN *src, uint64_t src_cap, const uint64_t *d_counts, const uint64_t *src_base, uint32_t nsrc,
		      uint32_t nb, int open_bits, uint32_t first_prefix, uint32_t *dst, uint64_t dst_cap, uint64_t n_expected)
{
	constexpr bool IN16 = sizeof(IN) == 2, HIST = sizeof(IN) == 1; // (HIST: src = records of hist2_pack_kernel, src_cap in bytes)
	if (!c) return MSD_EINVAL;
	if (!src || !dst || !d_counts || !src_base) return fail(c, MSD_EINVAL, "merge_buckets: null pointer");
	if (nsrc < 1 || nsrc > 8) return fail(c, MSD_EINVAL, "merge_buckets: 1..8 source runs per bucket");
	if (nb == 0 || nb > (1u << 24)) return fail(c, MSD_EINVAL, "merge_buckets: bucket count out of range");
	if (open_bits < 1 || open_bits > 16) return fail(c, MSD_EINVAL, "merge_buckets: 1..16 open bits");
	if ((IN16 || HIST) && open_bits != 16) return fail(c, MSD_EINVAL, "merge_buckets: extents of low halves need 16 open bits");
	if (HIST && src_cap < (uint64_t)nsrc * nb * kH2Rec) return fail(c, MSD_EINVAL, "merge_buckets: %u x %u records of %u bytes do not fit the source buffer", nsrc, nb, kH2Rec);
	if (!aligned16(src) || !aligned16(dst)) return fail(c, MSD_EINVAL, "merge_buckets: buffers must be 16-byte aligned");
	if (n_expected > dst_cap) return fail(c, MSD_EINVAL, "merge_buckets: the output buffer is too small");
	if ((uint64_t)first_prefix + nb > (1ull << (32 - open_bits))) return fail(c, MSD_EINVAL, "merge_buckets: bucket numbers exceed the key's prefix");
	// (the leaf reads extents while other workgroups write finished buckets)
	if (ranges_overlap(src, src_cap * sizeof(IN), dst, dst_cap * 4)) return fail(c, MSD_EINVAL, "merge_buckets: source and destination overlap");
	HIPCHK(c, hipSetDevice(c->device));
	c->stat_written = 0;
	phase_begin(c);
	if (n_expected == 0) return MSD_OK;
	struct Zeroed { // (cleared by one memset before the plan kernel)
		Counters ctr;
		alignas(256) uint32_t status[64]; // [0]: the counts do not add up (merge_plan_kernel)
	} *zeroed = nullptr;
	uint32_t *cnt32 = nullptr;
	uint64_t *soff = nullptr, *doff = nullptr;
	Segment *rej = nullptr;
	int rc = slab_carve(c, [&](Bump &b) {
		zeroed = b.take<Zeroed>(1);
		cnt32 = b.take<uint32_t>((size_t)nsrc * nb);
		soff = b.take<uint64_t>((size_t)nsrc * nb);
		doff = b.take<uint64_t>((size_t)nb + 1);
		rej = b.take<Segment>(nb);
	});
	if (!rc) rc = pinned_reserve(c, 4096);
	if (rc) return rc;
	Counters *ctr = &zeroed->ctr;
	uint32_t *status = zeroed->status;
	HIPCHK(c, hipMemsetAsync(zeroed, 0, sizeof *zeroed, c->stream));
	MergeBase mb = {};
	for (uint32_t x = 0; x < nsrc; ++x) mb.b[x] = src_base[x];
	LAUNCH(c, merge_plan_kernel, nsrc + 1, 1024, 0, d_counts, mb, nsrc, nb, n_expected, cnt32, soff, doff, status);
	// buckets that fit the registers of a workgroup (shards of <= 2^27 keys at 8 ranks) take merge_place16_kernel, larger
	// ones (2^30 keys per rank: nsrc x 2^14 keys per bucket) merge_count_kernel
	// (low halves: merge_count_kernel at every bucket size -- shorter buckets cost it more per key, the exchange it follows
	// cost half)
	const bool in_regs = !IN16 && !HIST && (c->opt.merge_leaf == 1 || (c->opt.merge_leaf == 0 && n_expected / nb <= 12000 && open_bits >= (int)kC16MinBits));
	if (in_regs) {
		if constexpr (!IN16 && !HIST) { // (whole keys only)
			const unsigned grid = (unsigned)std::min<uint64_t>(nb, (uint64_t)c->sm_count * 2);
			const auto place16 = nsrc <= 2 ? merge_place16_kernel<2> : nsrc <= 4 ? merge_place16_kernel<4> : merge_place16_kernel<8>;
			LAUNCH(c, place16, grid, kC16Th, kC16Lds, src, src_cap, dst, cnt32, soff, doff, nsrc, nb, open_bits, first_prefix, rej, ctr, status);
		}
	} else {
		const unsigned grid = (unsigned)std::min<uint64_t>(nb, (uint64_t)c->sm_count);
		LAUNCH(c, (merge_count_kernel<false, IN>), grid, kMcTh, kMcLds, src, dst, cnt32, soff, doff, nsrc, nb, open_bits, first_prefix, nullptr, nullptr,
		       rej, &ctr->nslow16, &ctr->count_ticket3, status);
	}
	phase_mark(c, "merge leaf");
	// what the leaf did not take (rare: long or crowded buckets) lies unsorted at its place in dst: the general leaves finish it
	Counters hc;
	uint32_t bad_counts = 0;
	if ((rc = read_counters(c, ctr, hc, { { sizeof(Counters), status, sizeof bad_counts, &bad_counts } }))) return rc;
	if (bad_counts) return fail(c, MSD_EINVAL, "merge_buckets: the counts do not add up to the expected %llu keys (or a count exceeds 32 bits)", (unsigned long long)n_expected);
	const uint32_t nrej = hc.nslow16;
	phase_end(c);
	if (nrej) {
		std::vector<Segment> segs;
		if ((rc = fetch(c, rej, nrej, segs))) return rc;
		if ((rc = sort_impl<uint32_t, NoVal>(c, dst, nullptr, n_expected, 32, SortJob<uint32_t>::list(segs)))) return rc;
	}
	set_stat(c, kStatMergeRejected, nrej);
	return MSD_OK;
}

extern "C" {

int msd_bucket_bounds_u32(msd_ctx *c, const uint32_t *k, uint64_t n, unsigned shift, uint64_t first, uint32_t nbuckets, uint64_t *bounds)
{
	return bounds_impl<uint32_t>(c, k, n, shift, first, nbuckets, bounds);
}
int msd_bucket_bounds_u64(msd_ctx *c, const uint64_t *k, uint64_t n, unsigned shift, uint64_t first, uint32_t nbuckets, uint64_t *bounds)
{
	return bounds_impl<uint64_t>(c, k, n, shift, first, nbuckets, bounds);
}
int msd_merge_buckets_u32(msd_ctx *c, const uint32_t *d_src, uint64_t src_cap, const uint64_t *d_counts, const uint64_t *src_base, uint32_t nsrc,
			  uint32_t nbuckets, int open_bits, uint32_t first_prefix, uint32_t *d_dst, uint64_t dst_cap, uint64_t n_expected)
{
	return merge_impl<uint32_t>(c, d_src, src_cap, d_counts, src_base, nsrc, nbuckets, open_bits, first_prefix, d_dst, dst_cap, n_expected);
}
int msd_merge_buckets_u32_low16(msd_ctx *c, const uint16_t *d_src, uint64_t src_cap, const uint64_t *d_counts, const uint64_t *src_base, uint32_t nsrc,
				uint32_t nbuckets, uint32_t first_prefix, uint32_t *d_dst, uint64_t dst_cap, uint64_t n_expected)
{
	return merge_impl<uint16_t>(c, d_src, src_cap, d_counts, src_base, nsrc, nbuckets, 16, first_prefix, d_dst, dst_cap, n_expected);
}
int msd_merge_buckets_u32_hist2(msd_ctx *c, const void *d_rec, uint64_t rec_bytes, const uint64_t *d_counts, uint32_t nsrc, uint32_t nbuckets,
				uint32_t first_prefix, uint32_t *d_dst, uint64_t dst_cap, uint64_t n_expected)
{
	const uint64_t zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; // (records lie at fixed places: source x's at x * nbuckets * record size)
	return merge_impl<Hist2>(c, (const Hist2 *)d_rec, rec_bytes, d_counts, zero, nsrc, nbuckets, 16, first_prefix, d_dst, dst_cap, n_expected);
}
uint64_t msd_hist2_record_bytes(void) { return kH2Rec; }
} // extern "C"
template <typename IN>
static int hist2_pack_impl(msd_ctx *c, const IN *d_keys, uint64_t n, const uint64_t *d_bounds, uint32_t nbuckets, void *d_rec, uint64_t rec_bytes,
			   uint32_t *d_overflow)
{
	if (!c) return MSD_EINVAL;
	if (!d_keys || !d_bounds || !d_rec || !d_overflow) return fail(c, MSD_EINVAL, "hist2_pack: null pointer");
	if (nbuckets == 0 || nbuckets > 65536) return fail(c, MSD_EINVAL, "hist2_pack: 1..65536 buckets");
	if (!aligned16(d_keys) || !aligned16(d_rec)) return fail(c, MSD_EINVAL, "hist2_pack: buffers must be 16-byte aligned");
	if (rec_bytes < (uint64_t)nbuckets * kH2Rec) return fail(c, MSD_EINVAL, "hist2_pack: %u records of %u bytes do not fit the output buffer", nbuckets, kH2Rec);
	if (ranges_overlap(d_keys, n * sizeof(IN), d_rec, (uint64_t)nbuckets * kH2Rec)) return fail(c, MSD_EINVAL, "hist2_pack: source and destination overlap");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemsetAsync(d_overflow, 0, sizeof(uint32_t), c->stream));
	const unsigned grid = (unsigned)std::min<uint64_t>(nbuckets, (uint64_t)c->sm_count * 2);
	LAUNCH(c, (hist2_pack_kernel<IN>), grid, kH2Th, kH2Lds, d_keys, d_bounds, nbuckets, d_rec, d_overflow);
	return MSD_OK;
}
namespace {
// the tables msd_order_low16_counts_u32 leaves in the slab for msd_order_low16_scatter_u32
struct Low16Tables {
	uint64_t *pb;             // bounds of the 256 top-digit buckets
	uint32_t *wg;             // per workgroup and bucket: keys counted
	unsigned long long *base; // per workgroup and bucket: where its share goes
	void carve(Bump &b)
	{
		pb = b.take<uint64_t>(257);
		wg = b.take<uint32_t>((size_t)65536 * kS16Chunks);
		base = b.take<unsigned long long>((size_t)65536 * kS16Chunks + 1);
	}
};
} // namespace
extern "C" {
int msd_hist2_pack_u32(msd_ctx *c, const uint32_t *d_keys, uint64_t n, const uint64_t *d_bounds, uint32_t nbuckets, void *d_rec, uint64_t rec_bytes,
		       uint32_t *d_overflow)
{
	return hist2_pack_impl<uint32_t>(c, d_keys, n, d_bounds, nbuckets, d_rec, rec_bytes, d_overflow);
}
int msd_hist2_pack_u32_low16(msd_ctx *c, const uint16_t *d_low, uint64_t n, const uint64_t *d_bounds, uint32_t nbuckets, void *d_rec, uint64_t rec_bytes,
			     uint32_t *d_overflow)
{
	return hist2_pack_impl<uint16_t>(c, d_low, n, d_bounds, nbuckets, d_rec, rec_bytes, d_overflow);
}
int msd_bounds_from_counts16(msd_ctx *c, const uint64_t *d_counts, uint64_t *d_bounds)
{
	if (!c) return MSD_EINVAL;
	if (!d_counts || !d_bounds) return fail(c, MSD_EINVAL, "bounds_from_counts16: null pointer");
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, bounds16_kernel, 1, 1024, 0, d_counts, d_bounds);
	return MSD_OK;
}
// msd_order_low16_u32 in two halves: the counts are ready (asynchronously) after the first, so that the caller can start its
// count exchange with the other ranks while the second -- the scatter, 2 ms per 2^30 keys -- runs
int msd_order_low16_counts_u32(msd_ctx *c, uint32_t *d_keys, uint64_t n, uint64_t *d_counts)
{
	if (!c) return MSD_EINVAL;
	c->order_keys = nullptr;
	if (!d_counts || (n && !d_keys)) return fail(c, MSD_EINVAL, "order_low16: null pointer");
	if (!aligned16(d_keys)) return fail(c, MSD_EINVAL, "order_low16: buffers must be 16-byte aligned");
	if (n >= (1ull << 40)) return fail(c, MSD_EINVAL, "order_low16: too many keys");
	// one in-place round on the top 8 bits (the direct-placement round 0) ...
	int rc = sort_impl<uint32_t, NoVal>(c, d_keys, nullptr, n, 32, SortJob<uint32_t>::whole(24u));
	if (rc) return rc;
	// ... exact counts of all upper halves and the place of every workgroup's share of every bucket
	HIPCHK(c, hipSetDevice(c->device));
	Low16Tables t;
	if ((rc = slab_carve(c, [&](Bump &b) { t.carve(b); }))) return rc;
	LAUNCH(c, (bucket_bounds_kernel<uint32_t>), 2, 256, 0, d_keys, n, 24, 0, 256, t.pb);
	LAUNCH(c, hist16_kernel, 256 * kS16Chunks, kS16Th, 0, d_keys, n, t.pb, t.wg);
	LAUNCH(c, scan16_kernel, 256, 256, 0, t.wg, t.pb, reinterpret_cast<unsigned long long *>(d_counts), t.base);
	c->order_keys = d_keys; // (the tables of the scatter lie in the slab: the scatter must be this context's next call)
	c->order_n = n;
	return MSD_OK;
}
int msd_order_low16_scatter_u32(msd_ctx *c, const uint32_t *d_keys, uint64_t n, uint16_t *d_out)
{
	if (!c) return MSD_EINVAL;
	if (!d_out || (n && !d_keys)) return fail(c, MSD_EINVAL, "order_low16: null pointer");
	if (c->order_keys != d_keys || c->order_n != n) return fail(c, MSD_EINVAL, "order_low16_scatter: not preceded by msd_order_low16_counts_u32 on the same keys");
	c->order_keys = nullptr;
	if (!aligned16(d_out)) return fail(c, MSD_EINVAL, "order_low16: buffers must be 16-byte aligned");
	if (ranges_overlap(d_keys, n * 4, d_out, n * 2)) return fail(c, MSD_EINVAL, "order_low16: source and destination overlap");
	HIPCHK(c, hipSetDevice(c->device));
	Low16Tables t;
	slab_recarve(c, [&](Bump &b) { t.carve(b); }); // (as msd_order_low16_counts_u32 left it)
	if (n) LAUNCH(c, scatter_low16_kernel, 256 * kS16Chunks, kS16Th, kS16Lds, d_keys, n, t.pb, t.base, d_out);
	return MSD_OK;
}
int msd_order_low16_u32(msd_ctx *c, uint32_t *d_keys, uint64_t n, uint16_t *d_out, uint64_t *d_counts)
{
	if (!c) return MSD_EINVAL;
	if (!d_out) return fail(c, MSD_EINVAL, "order_low16: null pointer");
	int rc = msd_order_low16_counts_u32(c, d_keys, n, d_counts);
	if (!rc) rc = msd_order_low16_scatter_u32(c, d_keys, n, d_out);
	return rc;
}
int msd_pack_low16_u32(msd_ctx *c, const uint32_t *d_keys, uint64_t n, uint16_t *d_out)
{
	if (!c) return MSD_EINVAL;
	if (n == 0) return MSD_OK;
	if (!d_keys || !d_out) return fail(c, MSD_EINVAL, "pack_low16: null pointer");
	if (!aligned16(d_keys) || !aligned16(d_out)) return fail(c, MSD_EINVAL, "pack_low16: buffers must be 16-byte aligned");
	if (ranges_overlap(d_keys, n * 4, d_out, n * 2)) return fail(c, MSD_EINVAL, "pack_low16: source and destination overlap");
	HIPCHK(c, hipSetDevice(c->device));
	const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 16, (n / 8 + 255) / 256 + 1);
	LAUNCH(c, pack_low16_kernel, grid, 256, 0, d_keys, n, d_out);
	return MSD_OK;
}

// ---- segmented sort and run gather: what a rank of the multi-GPU sort does with the keys it received

int msd_sort_u32_segments(msd_ctx *c, uint32_t *k, uint64_t n, const uint64_t *seg_off, uint32_t nseg, int end_bit) { return sort_segments<uint32_t, NoVal>(c, k, nullptr, n, seg_off, nseg, end_bit); }
int msd_sort_u64_segments(msd_ctx *c, uint64_t *k, uint64_t n, const uint64_t *seg_off, uint32_t nseg, int end_bit) { return sort_segments<uint64_t, NoVal>(c, k, nullptr, n, seg_off, nseg, end_bit); }
int msd_sort_pairs_u64_segments(msd_ctx *c, uint64_t *k, uint64_t *r, uint64_t n, const uint64_t *seg_off, uint32_t nseg, int end_bit) { return sort_segments<uint64_t, uint64_t>(c, k, r, n, seg_off, nseg, end_bit); }

int msd_gather_runs_u32(msd_ctx *c, uint32_t *dst, const uint32_t *src, const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, uint32_t nruns)
{
	return gather_impl<uint32_t>(c, dst, src, src_off, dst_off, len, nruns);
}
int msd_gather_runs_u64(msd_ctx *c, uint64_t *dst, const uint64_t *src, const uint64_t *src_off, const uint64_t *dst_off, const uint64_t *len, uint32_t nruns)
{
	return gather_impl<uint64_t>(c, dst, src, src_off, dst_off, len, nruns);
}

// ---- splitter service (reference: sampling src/msb_64.c:1511-1521, extract_delimiters :1304-1322, range function :188-204)

} // extern "C"

template <typename K> static int sample_impl(msd_ctx *c, const K *k, uint64_t n, uint64_t m, uint64_t seed, K *out)
{
	if (!c) return MSD_EINVAL;
	if (m && (!k || !out || n == 0)) return fail(c, MSD_EINVAL, "sample: null pointer or empty input");
	HIPCHK(c, hipSetDevice(c->device));
	if (m == 0) return MSD_OK;
	const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 8, (m + 255) / 256);
	LAUNCH(c, (sample_kernel<K>), grid, 256, 0, k, n, m, seed, out);
	return MSD_OK;
}

template <typename K> static int splitters_impl(msd_ctx *c, const K *sorted_sample, uint64_t m, unsigned parts, K *delims)
{
	if (!c) return MSD_EINVAL;
	if (parts < 1 || parts > 256) return fail(c, MSD_EINVAL, "splitters: parts must be 1..256");
	if (parts == 1) return MSD_OK;
	if (!sorted_sample || !delims || m == 0) return fail(c, MSD_EINVAL, "splitters: null pointer or empty sample");
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, (splitters_kernel<K>), 1, 256, 0, sorted_sample, m, parts, delims);
	return MSD_OK;
}

template <typename K, typename V>
static int range_partition_impl(msd_ctx *c, K *k, uint64_t *r, uint64_t n, const K *delims, unsigned parts, uint64_t *cnt)
{
	if (!c) return MSD_EINVAL;
	if (parts < 1 || parts > 256) return fail(c, MSD_EINVAL, "partition_by_splitters: parts must be 1..256");
	if (parts > 1 && !delims) return fail(c, MSD_EINVAL, "partition_by_splitters: null delimiters");
	HIPCHK(c, hipSetDevice(c->device));
	if (parts == 1) { // one range: nothing moves; its size goes to the device on the context's stream (ordered with the caller's work there)
		if (cnt) {
			int rcp = pinned_reserve(c, 64);
			if (!rcp) rcp = upload(c, { { cnt, &n, sizeof n } });
			if (rcp) return rcp;
			HIPCHK(c, hipStreamSynchronize(c->stream));
		}
		return MSD_OK;
	}
	if (cnt) HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(uint64_t) * parts, c->stream));
	unsigned width = 1;
	while ((1u << width) < parts) ++width;
	// one in-place round whose buckets are the ranges (parts - 1 delimiters; the buckets beyond `parts` stay empty)
	return sort_impl<K, V>(c, k, r, n, (int)sizeof(K) * 8, SortJob<K>::ranges(delims, parts - 1, width, cnt));
}

extern "C" {

int msd_sample_u32(msd_ctx *c, const uint32_t *k, uint64_t n, uint64_t m, uint64_t seed, uint32_t *out) { return sample_impl<uint32_t>(c, k, n, m, seed, out); }
int msd_sample_u64(msd_ctx *c, const uint64_t *k, uint64_t n, uint64_t m, uint64_t seed, uint64_t *out) { return sample_impl<uint64_t>(c, k, n, m, seed, out); }
int msd_splitters_u32(msd_ctx *c, const uint32_t *s, uint64_t m, unsigned parts, uint32_t *d) { return splitters_impl<uint32_t>(c, s, m, parts, d); }
int msd_splitters_u64(msd_ctx *c, const uint64_t *s, uint64_t m, unsigned parts, uint64_t *d) { return splitters_impl<uint64_t>(c, s, m, parts, d); }
int msd_partition_by_splitters_u32(msd_ctx *c, uint32_t *k, uint64_t n, const uint32_t *delims, unsigned parts, uint64_t *cnt)
{
	return range_partition_impl<uint32_t, NoVal>(c, k, nullptr, n, delims, parts, cnt);
}
int msd_partition_by_splitters_u64(msd_ctx *c, uint64_t *k, uint64_t n, const uint64_t *delims, unsigned parts, uint64_t *cnt)
{
	return range_partition_impl<uint64_t, NoVal>(c, k, nullptr, n, delims, parts, cnt);
}
int msd_partition_by_splitters_pairs_u64(msd_ctx *c, uint64_t *k, uint64_t *r, uint64_t n, const uint64_t *delims, unsigned parts, uint64_t *cnt)
{
	if (c && !r) return fail(c, MSD_EINVAL, "partition_by_splitters: null rids");
	return range_partition_impl<uint64_t, uint64_t>(c, k, r, n, delims, parts, cnt);
}

} // extern "C"

template <typename K>
static int histogram_impl(msd_ctx *c, const K *k, uint64_t n, unsigned shift, unsigned rb, uint64_t *cnt)
{
	if (!c) return MSD_EINVAL;
	if (!cnt || (n && !k)) return fail(c, MSD_EINVAL, "null pointer");
	if (rb < 1 || rb > 12 || shift + rb > sizeof(K) * 8) return fail(c, MSD_EINVAL, "radix_bits must be 1..12 and shift+radix_bits within the key");
	if (!aligned16(k)) return fail(c, MSD_EINVAL, "keys must be 16-byte aligned");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(uint64_t) << rb, c->stream));
	if (n == 0) return MSD_OK;
	const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 8, (n + 4095) / 4096);
	LAUNCH(c, (histogram_kernel<K>), grid, 256, sizeof(uint32_t) << rb, k, n, shift, rb, reinterpret_cast<unsigned long long *>(cnt));
	return MSD_OK;
}
extern "C" {

int msd_histogram_u32(msd_ctx *c, const uint32_t *k, uint64_t n, unsigned s, unsigned rb, uint64_t *cnt) { return histogram_impl(c, k, n, s, rb, cnt); }
int msd_histogram_u64(msd_ctx *c, const uint64_t *k, uint64_t n, unsigned s, unsigned rb, uint64_t *cnt) { return histogram_impl(c, k, n, s, rb, cnt); }

int msd_exclusive_scan_u64(msd_ctx *c, const uint64_t *in, uint64_t *out, uint64_t n)
{
	if (!c) return MSD_EINVAL;
	if (n && (!in || !out)) return fail(c, MSD_EINVAL, "null pointer");
	HIPCHK(c, hipSetDevice(c->device));
	if (n == 0) return MSD_OK;
	const size_t ntiles = (n + kScanTile - 1) / kScanTile;
	uint32_t *ctr = nullptr; // [0] tile counter, [2] error flag
	unsigned long long *state = nullptr;
	int rc = slab_carve(c, [&](Bump &b) {
		ctr = b.take<uint32_t>(64);
		state = b.take<unsigned long long>(ntiles);
	});
	if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(ctr, 0, 64 * sizeof(uint32_t), c->stream));
	HIPCHK(c, hipMemsetAsync(state, 0, ntiles * 8, c->stream));
	LAUNCH(c, scan_lookback_kernel, (unsigned)ntiles, kScanTh, 0, in, out, n, state, ctr, ctr + 2);
	// the look-back gives up after a bounded number of polls and sets a flag: report it (one small readback)
	rc = pinned_reserve(c, 64);
	if (rc) return rc;
	uint32_t timed_out = 0;
	if ((rc = read_back(c, ctr + 2, &timed_out))) return rc;
	if (timed_out) return fail(c, MSD_EINTERNAL, "exclusive scan: a tile's look-back timed out");
	return MSD_OK;
}

} // extern "C"

// ------------------------------------------------------------ radix select / top-k (kernels: msd_select.hpp)

#ifndef MSD_TOPK_PACKED_STOP // (overridable for experiments: 0 or 32)
#define MSD_TOPK_PACKED_STOP 0
#endif

// key_type (valid) -> the unsigned type that carries the key and whether the key is its own code (raw):
// f(K(), std::true_type or std::false_type)
template <typename F> static int with_key_type(int key_type, F &&f)
{
	if (key_type_bytes(key_type) == 4) return key_type == kKeyU32 ? f(uint32_t(), std::true_type()) : f(uint32_t(), std::false_type());
	return key_type == kKeyU64 ? f(uint64_t(), std::true_type()) : f(uint64_t(), std::false_type());
}

// the phases of an internal sort, added to the ones collected so far (every sort_impl starts its own list)
static void phases_append(msd_ctx *c, std::vector<std::pair<std::string, double>> &all)
{
	for (auto &p : c->phase_us) phase_add(all, p.first, p.second);
}

// A stage behind an internal sort: what `launches` starts is the phase `name`, added to the phases the sort has left
template <typename F> static int tail_phase(msd_ctx *c, const char *name, F &&launches)
{
	std::vector<std::pair<std::string, double>> phases = c->phase_us;
	phase_begin(c);
	if (int rc = launches()) return rc;
	phase_mark(c, name);
	phase_end(c);
	phases_append(c, phases);
	c->phase_us = phases;
	return MSD_OK;
}

// TOPK: out[0 .. k) = the k smallest keys in the order of key ^ flip, sorted ascending as plain keys; otherwise
// *value = the key of rank k in that order.  One readback of the search state behind the filter pass, the internal
// sorts' own, and (select) one of the value.
// EMIT (msd_select.hpp) != kSelRaw: typed keys (msd_topk_keys / msd_select_key).  The search, the candidates and the
// output work on the keys' codes under `codec`; `out` holds the elements the filter writes (codes, or packed
// code << 32 | position elements in the caller's index array) and is sorted as plain unsigned keys; `rids` is not used
// (positions are generated); a finishing pass decodes the k elements -- into `final_keys` for packed elements, in place
// otherwise.
template <typename K, typename V, bool TOPK, int EMIT = kSelRaw>
static int select_impl(msd_ctx *c, const K *keys, const uint64_t *rids, uint64_t n, uint64_t k, int which, typename sel_elem<K, EMIT>::type *out,
		       uint64_t *out_rids, K *value, KeyCodec<K> codec = KeyCodec<K>{ 0, 0 }, K *final_keys = nullptr)
{
	typedef typename sel_elem<K, EMIT>::type E;
	constexpr bool HV = has_val<V>::value;
	constexpr bool LOADS_RIDS = HV && EMIT == kSelRaw;
	constexpr bool PACKED = EMIT == kSelPacked;
	constexpr int EB = sizeof(E) * 8;
	constexpr uint32_t KB = sizeof(K) * 8;
	constexpr uint32_t PASSES = sel_max_passes<K>();
	if (!c) return MSD_EINVAL;
	if (which != MSD_SMALLEST && which != MSD_LARGEST) return fail(c, MSD_EINVAL, "which must be MSD_SMALLEST or MSD_LARGEST");
	if (TOPK ? k > n : k >= n) return fail(c, MSD_EINVAL, TOPK ? "k must not exceed n" : "k must be smaller than n");
	if (!TOPK && !value) return fail(c, MSD_EINVAL, "null result pointer");
	if (TOPK && k == 0) return MSD_OK;
	if (!keys || (LOADS_RIDS && !rids) || (TOPK && !out) || (TOPK && HV && !out_rids) || (PACKED && !final_keys))
		return fail(c, MSD_EINVAL, "null data pointer");
	if (!aligned16(keys) || (LOADS_RIDS && !aligned16(rids)) || (TOPK && !aligned16(out)) || (TOPK && HV && !aligned16(out_rids)) || (PACKED && !aligned16(final_keys)))
		return fail(c, MSD_EINVAL, "input and output buffers must be 16-byte aligned");
	if (n >= ((uint64_t)1 << 36)) return fail(c, MSD_EINVAL, "n too large");
	if (PACKED && n > ((uint64_t)1 << 32)) return fail(c, MSD_EINVAL, "indices of a 32-bit key type need n <= 2^32 (the position travels in 32 bits)");
	if (TOPK) {
		const size_t ib = n * sizeof(K), ob = k * sizeof(E), rb = LOADS_RIDS ? n * 8 : 0, orb = HV ? k * 8 : 0, fb = PACKED ? k * sizeof(K) : 0;
		if (ranges_overlap(keys, ib, out, ob) || ranges_overlap(keys, ib, out_rids, orb) || ranges_overlap(rids, rb, out, ob) ||
		    ranges_overlap(rids, rb, out_rids, orb) || ranges_overlap(out, ob, out_rids, orb) || ranges_overlap(keys, ib, final_keys, fb) ||
		    ranges_overlap(out, ob, final_keys, fb))
			return fail(c, MSD_EINVAL, "the output must not overlap the input");
	}
	HIPCHK(c, hipSetDevice(c->device));
	const uint64_t cap = c->opt.select_cap;
	const K flip = which == MSD_LARGEST ? (K)~(K)0 : (K)0;
	// what the kernels do with a key (msd_select.hpp): plain keys have instances of their own
	typedef typename std::conditional<EMIT == kSelRaw, SelPlain<K>, SelCoded<K>>::type HOW;
	HOW how;
	how.flip = flip;
	if constexpr (EMIT != kSelRaw) how.codec = codec;
	// the workspace of the search: state | one histogram per pass | candidate keys | candidate rids
	Bump b(nullptr);
	b.take<SelectState>(1);
	b.take<unsigned long long>((size_t)PASSES * kSelBins);
	const size_t zero_bytes = b.off;
	b.take<E>(cap);
	if (HV) b.take<uint64_t>(cap);
	int rc = dev_reserve(c, c->sel, c->sel_bytes, b.off, true);
	if (!rc) rc = pinned_reserve(c, 4096);
	if (rc) return rc;
	Bump r(c->sel);
	SelectState *st = r.take<SelectState>(1);
	unsigned long long *bins = r.take<unsigned long long>((size_t)PASSES * kSelBins);
	E *cand = r.take<E>(cap);
	uint64_t *cand_rids = HV ? r.take<uint64_t>(cap) : nullptr;

	c->stat_written = 0;
	phase_begin(c);
	HIPCHK(c, hipMemsetAsync(c->sel, 0, zero_bytes, c->stream));
	const uint64_t nvec = n / Vec16<K>::N;
	const unsigned hist_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->sm_count * 8, (nvec + kSelTh * kSelHistU - 1) / (kSelTh * kSelHistU)));
	const uint64_t rank = TOPK ? k - 1 : k;
	for (uint32_t p = 0; p < PASSES; ++p) {
		unsigned long long *const pb = bins + (size_t)p * kSelBins;
		LAUNCH(c, (p == 0 ? select_hist_kernel<K, true, HOW> : select_hist_kernel<K, false, HOW>), hist_grid, kSelTh, 0, keys, n, how, st, pb);
		LAUNCH(c, (select_pivot_kernel<K>), 1, kSelPivotTh, 0, st, pb, p, n, rank, cap);
	}
	phase_mark(c, "select_hist");
	const uint64_t tile_vecs = (uint64_t)kSelTh * kSelFilterU;
	const unsigned filter_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->sm_count * 4, (nvec + tile_vecs - 1) / tile_vecs));
	// staging buffers of the filter: long runs per reservation where much of the input goes to the output (more than 1/32 of it)
	constexpr uint32_t elem = sizeof(E) + (HV ? 8 : 0);
	// (the candidates too: when the bits run out on a heavy value they go to the output as well)
	const bool dense = TOPK && k > n / 32;
	const uint32_t stage_cand = (dense ? kSelStageLargeCand : kSelStageSmall) / elem;
	const uint32_t stage_below = !TOPK ? 0 : (dense ? kSelStageLargeBelow : kSelStageSmall) / elem;
	LAUNCH(c, (select_filter_kernel<K, V, TOPK, EMIT, HOW>), filter_grid, kSelTh, (size_t)(stage_cand + stage_below) * elem, keys, rids, n, how, st, out,
	       out_rids, cand, cand_rids, stage_cand, stage_below);
	phase_mark(c, "select_filter");
	SelectState h;
	if ((rc = read_back(c, st, &h))) return rc;
	phase_end(c);
	std::vector<std::pair<std::string, double>> phases = c->phase_us;
	const uint64_t needed = h.rank + 1; // candidates that belong to the answer (top-k)
	if (!h.done || h.consumed > KB || h.rank >= h.bucket || (!h.exhausted && h.bucket > cap) || (TOPK && h.below + needed != k) ||
	    (TOPK && h.out_cursor != h.below) || (!h.exhausted && h.cand_cursor != h.bucket))
		return fail(c, MSD_EINTERNAL, "select: inconsistent search state (bucket %llu, below %llu, rank %llu, consumed %u, cursors %llu/%llu)",
			    h.bucket, h.below, h.rank, h.consumed, h.out_cursor, h.cand_cursor);
	const int open = (int)(KB - h.consumed);
	const bool smallest = which == MSD_SMALLEST;
	// (packed elements: the code is the upper half.  MSD_TOPK_PACKED_STOP = 0 sorts the whole element: equal keys come out
	// in the order of their positions; 32 orders by the code alone and stops there, which measured no faster: DESIGN.md
	// section 10)
	const SortJob<E> job = SortJob<E>::whole(PACKED ? MSD_TOPK_PACKED_STOP : 0);
	if (TOPK) {
		if (!h.exhausted) {
			// only the order of the candidates decides which of them belong to the answer
			if (needed < h.bucket && open > 0) {
				if ((rc = sort_impl<E, V>(c, cand, cand_rids, h.bucket, open + (EB - (int)KB), job))) return rc;
				phases_append(c, phases);
			}
			const uint64_t from = smallest ? 0 : h.bucket - needed;
			HIPCHK(c, hipMemcpyAsync(out + h.below, cand + from, needed * sizeof(E), hipMemcpyDeviceToDevice, c->stream));
			if (HV) HIPCHK(c, hipMemcpyAsync(out_rids + h.below, cand_rids + from, needed * 8, hipMemcpyDeviceToDevice, c->stream));
		}
		if ((rc = sort_impl<E, V>(c, out, out_rids, k, EB, job))) return rc;
		phases_append(c, phases);
		if constexpr (EMIT != kSelRaw) {
			phase_begin(c);
			const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 8, (k + kSelFinishTh - 1) / kSelFinishTh);
			if constexpr (PACKED)
				LAUNCH(c, (select_finish_kernel<K, true>), grid, kSelFinishTh, 0, out, final_keys, k, codec);
			else
				LAUNCH(c, (select_finish_kernel<K, false>), grid, kSelFinishTh, 0, nullptr, out, k, codec);
			phase_mark(c, "select_finish");
			phase_end(c);
			phases_append(c, phases);
		}
	} else if (h.exhausted || open == 0) {
		*value = codec.dec((K)h.prefix ^ flip); // every bit is decided: the prefix is the key (its code)
	} else {
		if (h.bucket > 1) {
			if ((rc = sort_impl<E, V>(c, cand, nullptr, h.bucket, open, SortJob<E>::whole()))) return rc;
			phases_append(c, phases);
		}
		K found;
		if ((rc = read_back(c, reinterpret_cast<const K *>(cand + (smallest ? h.rank : h.bucket - 1 - h.rank)), &found))) return rc;
		*value = codec.dec(found);
	}
	c->phase_us = phases;
	set_stat(c, kStatSelectHistPasses, h.passes);
	set_stat(c, kStatSelectSkippedBits, h.skipped);
	set_stat(c, kStatSelectCandidates, h.bucket);
	set_stat(c, kStatSelectBelow, TOPK ? h.below : 0);
	return MSD_OK;
}

extern "C" {

int msd_topk_u32(msd_ctx *c, const uint32_t *k, uint64_t n, uint64_t kk, int which, uint32_t *out)
{
	return select_impl<uint32_t, NoVal, true>(c, k, nullptr, n, kk, which, out, nullptr, nullptr);
}
int msd_topk_u64(msd_ctx *c, const uint64_t *k, uint64_t n, uint64_t kk, int which, uint64_t *out)
{
	return select_impl<uint64_t, NoVal, true>(c, k, nullptr, n, kk, which, out, nullptr, nullptr);
}
int msd_topk_pairs_u64(msd_ctx *c, const uint64_t *k, const uint64_t *r, uint64_t n, uint64_t kk, int which, uint64_t *out, uint64_t *out_rids)
{
	return select_impl<uint64_t, uint64_t, true>(c, k, r, n, kk, which, out, out_rids, nullptr);
}
int msd_select_u32(msd_ctx *c, const uint32_t *k, uint64_t n, uint64_t kk, int which, uint32_t *value)
{
	return select_impl<uint32_t, NoVal, false>(c, k, nullptr, n, kk, which, nullptr, nullptr, value);
}
int msd_select_u64(msd_ctx *c, const uint64_t *k, uint64_t n, uint64_t kk, int which, uint64_t *value)
{
	return select_impl<uint64_t, NoVal, false>(c, k, nullptr, n, kk, which, nullptr, nullptr, value);
}

// ---- typed keys and indices (codec: msd_keycodec.hpp)

static bool key_type_ok(int key_type) { return key_type >= 0 && key_type < kKeyTypes; }
static int check_key_type(msd_ctx *c, int key_type)
{
	return key_type_ok(key_type) ? MSD_OK : fail(c, MSD_EINVAL, "unknown key type %d (MSD_KEY_U32 .. MSD_KEY_F64)", key_type);
}
static int check_order(msd_ctx *c, int order)
{
	return order == MSD_ASCENDING || order == MSD_DESCENDING ? MSD_OK : fail(c, MSD_EINVAL, "order must be MSD_ASCENDING or MSD_DESCENDING");
}

int msd_key_encode(int key_type, uint64_t bits, uint64_t *code)
{
	if (!key_type_ok(key_type) || !code) return MSD_EINVAL;
	*code = key_type_bytes(key_type) == 4 ? (uint64_t)key_codec<uint32_t>(key_type).enc((uint32_t)bits) : key_codec<uint64_t>(key_type).enc(bits);
	return MSD_OK;
}
int msd_key_decode(int key_type, uint64_t code, uint64_t *bits)
{
	if (!key_type_ok(key_type) || !bits) return MSD_EINVAL;
	*bits = key_type_bytes(key_type) == 4 ? (uint64_t)key_codec<uint32_t>(key_type).dec((uint32_t)code) : key_codec<uint64_t>(key_type).dec(code);
	return MSD_OK;
}

int msd_topk_keys(msd_ctx *c, const void *d_keys, int key_type, uint64_t n, uint64_t k, int which, void *d_out_keys, uint64_t *d_out_idx)
{
	if (!c) return MSD_EINVAL;
	if (int rc = check_key_type(c, key_type)) return rc;
	return with_key_type(key_type, [&](auto k0, auto raw) {
		typedef decltype(k0) K;
		const K *keys = (const K *)d_keys;
		K *out = (K *)d_out_keys;
		const KeyCodec<K> codec = key_codec<K>(key_type);
		if (d_out_idx) {
			if constexpr (sizeof(K) == 4) // the index array is where the packed elements are filtered to and sorted
				return select_impl<K, NoVal, true, kSelPacked>(c, keys, nullptr, n, k, which, d_out_idx, nullptr, nullptr, codec, out);
			else
				return select_impl<K, uint64_t, true, kSelPos>(c, keys, nullptr, n, k, which, out, d_out_idx, nullptr, codec);
		}
		if constexpr (decltype(raw)::value) return select_impl<K, NoVal, true>(c, keys, nullptr, n, k, which, out, nullptr, nullptr);
		else return select_impl<K, NoVal, true, kSelCodes>(c, keys, nullptr, n, k, which, out, nullptr, nullptr, codec);
	});
}

int msd_select_key(msd_ctx *c, const void *d_keys, int key_type, uint64_t n, uint64_t k, int which, void *value)
{
	if (!c) return MSD_EINVAL;
	if (int rc = check_key_type(c, key_type)) return rc;
	return with_key_type(key_type, [&](auto k0, auto raw) {
		typedef decltype(k0) K;
		if constexpr (decltype(raw)::value) return select_impl<K, NoVal, false>(c, (const K *)d_keys, nullptr, n, k, which, nullptr, nullptr, (K *)value);
		else return select_impl<K, NoVal, false, kSelCodes>(c, (const K *)d_keys, nullptr, n, k, which, nullptr, nullptr, (K *)value, key_codec<K>(key_type));
	});
}

} // extern "C"

// ---- typed and descending sort: the unsigned sort, then range reversals (msd_reverse.hpp)

template <typename E> static int reverse_launch(msd_ctx *c, E *data, uint64_t n, const uint64_t *plan, uint64_t a, uint64_t b)
{
	return LAUNCH_RC(c, (reverse_ranges_kernel<E>), (unsigned)rev_grid_for<E>(n), kRevTh, 0, data, plan, a, b);
}

template <typename K> static int sort_keys_impl(msd_ctx *c, K *keys, uint64_t *rids, int key_type, uint64_t n, int order)
{
	const int kind = key_type % 3; // 0 unsigned, 1 signed, 2 float
	int rc;
	if constexpr (sizeof(K) == 8) // (tuples exist for 64-bit keys only)
		rc = rids ? sort_impl<K, uint64_t>(c, keys, rids, n, 64, SortJob<K>::whole()) : sort_impl<K, NoVal>(c, keys, nullptr, n, 64, SortJob<K>::whole());
	else
		rc = sort_impl<K, NoVal>(c, keys, nullptr, n, 32, SortJob<K>::whole());
	if (rc) return rc;
	if (n == 0 || (kind == 0 && order == MSD_ASCENDING)) { // the unsigned sort is the answer
		c->fix_stats = 1;
		c->fix_split = kind == 0 ? n : 0;
		return MSD_OK;
	}
	return tail_phase(c, "sort_fixup", [&]() -> int {
		LAUNCH(c, (sign_split_kernel<K>), 1, 64, 0, keys, n, kind, order, c->fix_plan);
		c->fix_stats = 2;
		if (n < 2) return MSD_OK;
		// descending needs one stage, ascending two; a stage without work is a launch whose workgroups leave at once
		for (int stage = 0; stage < (order == MSD_DESCENDING ? 1 : 2); ++stage) {
			const uint64_t *plan = c->fix_plan + (stage ? kFixStage2 : kFixStage1);
			if (int r = reverse_launch<K>(c, keys, n, plan, 0, 0)) return r;
			if (rids)
				if (int r = reverse_launch<uint64_t>(c, rids, n, plan, 0, 0)) return r;
		}
		return MSD_OK;
	});
}

static int sort_keys_entry(msd_ctx *c, void *d_keys, int key_type, uint64_t *d_rids, bool pairs, uint64_t n, int order)
{
	if (!c) return MSD_EINVAL;
	if (int rc = check_key_type(c, key_type)) return rc;
	if (int rc = check_order(c, order)) return rc;
	if (pairs && key_type_bytes(key_type) != 8) return fail(c, MSD_EINVAL, "tuples have 64-bit keys (MSD_KEY_U64 / I64 / F64)");
	if (n && (!d_keys || (pairs && !d_rids))) return fail(c, MSD_EINVAL, "null data pointer");
	const Span buf[2] = { span_of(d_keys, n, key_type_bytes(key_type), 16), span_of(pairs ? d_rids : nullptr, n, 8, 16) }; // both sorted in place
	if (first_misaligned(buf) >= 0) return fail(c, MSD_EINVAL, "keys/rids must be 16-byte aligned");
	if (n >= kMaxElems) return fail(c, MSD_EINVAL, "n too large for 32-bit block slots");
	if (outputs_overlap(buf, 1)) return fail(c, MSD_EINVAL, "keys and rids overlap");
	HIPCHK(c, hipSetDevice(c->device));
	return with_key_type(key_type, [&](auto k0, auto) {
		typedef decltype(k0) K;
		return sort_keys_impl<K>(c, (K *)d_keys, pairs ? d_rids : nullptr, key_type, n, order);
	});
}

extern "C" {

int msd_sort_keys(msd_ctx *c, void *d_keys, int key_type, uint64_t n, int order) { return sort_keys_entry(c, d_keys, key_type, nullptr, false, n, order); }
int msd_sort_pairs_keys(msd_ctx *c, void *d_keys, int key_type, uint64_t *d_rids, uint64_t n, int order)
{
	return sort_keys_entry(c, d_keys, key_type, d_rids, true, n, order);
}

int msd_reverse(msd_ctx *c, void *d_data, int elem_bytes, uint64_t first, uint64_t count)
{
	if (!c) return MSD_EINVAL;
	if (elem_bytes != 4 && elem_bytes != 8) return fail(c, MSD_EINVAL, "elem_bytes must be 4 or 8");
	if (count && !d_data) return fail(c, MSD_EINVAL, "null data pointer");
	if (!aligned_to(d_data, (uint32_t)elem_bytes)) return fail(c, MSD_EINVAL, "data must be aligned to its element size");
	if (first + count < first || first + count > UINT64_MAX / (unsigned)elem_bytes) return fail(c, MSD_EINVAL, "first + count overflows");
	HIPCHK(c, hipSetDevice(c->device));
	if (count < 2) return MSD_OK;
	return with_width(elem_bytes, [&](auto e) { return reverse_launch(c, (decltype(e) *)d_data, count, nullptr, first, first + count); });
}

} // extern "C"

// ---- per-row top-k (msd_select_rows.hpp)

static bool rows_in_envelope(uint64_t row_len, uint64_t k) { return row_len <= kRowsMaxLen && k <= kRowsMaxK; }

// Mode 0: does the row kernel beat the loop over msd_topk_keys?  One workgroup per row: with a few rows a call costs what ONE
// row costs one workgroup -- 0.41 ms per 2^20 float32 keys, 0.52 ms per 2^20 int64 keys, whatever k -- and the loop 0.11 to
// 0.15 ms per row whatever its length (profiles/topk_rows_sweep.jsonl; DESIGN.md section 10.2, "Dispatch").  From 4 rows on
// the kernel wins up to the envelope's longest row.
static bool rows_kernel_wins(uint64_t rows, uint64_t row_len) { return rows >= 4 || row_len < (rows << 18); }

// Lanes per row (profiles/topk_rows_sweep.jsonl, the `lanes*` columns): a wave where the row fits its registers; 256 lanes
// for rows below 8192 keys and wherever there are more rows than the chip holds 1024-thread workgroups (2 per CU: six
// 256-thread workgroups per CU then move more bytes), measured up to rows of 1 MiB; the 1024-thread workgroup otherwise --
// with few rows it finishes ONE row 1.3 to 2.6 times sooner.
static int rows_lanes(const msd_ctx *c, uint64_t rows, uint64_t row_len, uint64_t key_bytes)
{
	int by_shape = 1024;
	if (row_len <= kRowsWaveMaxLen)
		by_shape = 64;
	else if (row_len < kRowsMidMaxLen || (rows > 2 * (uint64_t)c->sm_count && row_len * key_bytes <= (1u << 20)))
		by_shape = 256;
	if (c->opt.topk_rows_lanes == 0 || (c->opt.topk_rows_lanes == 64 && row_len > kRowsWaveMaxLen)) return by_shape; // (a wave's buffer holds its whole row)
	return c->opt.topk_rows_lanes;
}

template <typename K>
static int rows_kernel_path(msd_ctx *c, const K *keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t stride, uint64_t k, int which, K *out,
			    uint64_t *out_idx)
{
	const K flip = which == MSD_LARGEST ? (K)~(K)0 : (K)0;
	const KeyCodec<K> codec = key_codec<K>(key_type);
	phase_begin(c);
	const int rc = with_flag(out_idx != nullptr, [&](auto idx) {
		return with_lanes(rows_lanes(c, rows, row_len, sizeof(K)), [&](auto lanes) {
			constexpr bool IDX = decltype(idx)::value;
			constexpr int LANES = decltype(lanes)::value;
			typedef RowsCfg<LANES> C;
			constexpr uint64_t groups = C::BLOCK / LANES;
			const uint64_t per_cu = LANES == 1024 ? 8 : 64; // (workgroups beyond what the chip holds at once walk the rows in a loop)
			const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->sm_count * per_cu, (rows + groups - 1) / groups));
			return LAUNCH_RC(c, (topk_rows_kernel<K, IDX, LANES>), grid, C::BLOCK, (RowsLds<K, IDX, LANES>::bytes), keys, rows, row_len, stride, k, flip, codec, out, out_idx);
		});
	});
	if (rc) return rc;
	phase_mark(c, "select_rows");
	phase_end(c);
	return MSD_OK;
}

// row by row through msd_topk_keys; what is not aligned to 16 bytes (which msd_topk_keys refuses) goes through the stage
static int rows_looped_path(msd_ctx *c, const char *keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t stride, uint64_t k, int which,
			    char *out, uint64_t *out_idx)
{
	const size_t es = (size_t)key_type_bytes(key_type);
	const size_t row_b = align_up(row_len * es, 256), out_b = align_up(k * es, 256), idx_b = align_up(k * 8, 256);
	const bool many = rows > 1;
	const bool stage = !aligned16(keys) || (many && ((stride * es) & 15)) || !aligned16(out) || (many && ((k * es) & 15)) ||
			   (out_idx && (!aligned16(out_idx) || (many && ((k * 8) & 15))));
	if (stage)
		if (int rc = dev_reserve(c, c->rows_stage, c->rows_stage_bytes, row_b + out_b + idx_b)) return rc;
	for (uint64_t r = 0; r < rows; ++r) {
		const char *in = keys + r * stride * es;
		char *o = out + r * k * es;
		uint64_t *ix = out_idx ? out_idx + r * k : nullptr;
		const bool in_st = !aligned16(in), o_st = !aligned16(o), ix_st = ix && !aligned16(ix);
		if (in_st) HIPCHK(c, hipMemcpyAsync(c->rows_stage, in, row_len * es, hipMemcpyDeviceToDevice, c->stream));
		char *const so = c->rows_stage + row_b;
		uint64_t *const sx = (uint64_t *)(c->rows_stage + row_b + out_b);
		if (int rc = msd_topk_keys(c, in_st ? c->rows_stage : in, key_type, row_len, k, which, o_st ? so : o, ix_st ? sx : ix)) return rc;
		if (o_st) HIPCHK(c, hipMemcpyAsync(o, so, k * es, hipMemcpyDeviceToDevice, c->stream));
		if (ix_st) HIPCHK(c, hipMemcpyAsync(ix, sx, k * 8, hipMemcpyDeviceToDevice, c->stream));
	}
	return MSD_OK;
}

extern "C" {

int msd_topk_rows_limits(int key_type, int with_idx, uint64_t *max_row_len, uint64_t *max_k)
{
	(void)with_idx; // (the LDS buffers are sized for the widest element: one envelope for all)
	if (!key_type_ok(key_type) || !max_row_len || !max_k) return MSD_EINVAL;
	*max_row_len = kRowsMaxLen;
	*max_k = kRowsMaxK;
	return MSD_OK;
}

int msd_topk_rows(msd_ctx *c, const void *d_keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t row_stride, uint64_t k, int which,
		  void *d_out_keys, uint64_t *d_out_idx)
{
	if (!c) return MSD_EINVAL;
	if (int rc = check_key_type(c, key_type)) return rc;
	if (which != MSD_SMALLEST && which != MSD_LARGEST) return fail(c, MSD_EINVAL, "which must be MSD_SMALLEST or MSD_LARGEST");
	if (k > row_len) return fail(c, MSD_EINVAL, "k must not exceed row_len");
	if (row_stride < row_len) return fail(c, MSD_EINVAL, "row_stride must not be smaller than row_len");
	const uint32_t es = (uint32_t)key_type_bytes(key_type);
	const RowsExtents ext = rows_extents(rows, row_len, row_stride, k, es, d_out_idx != nullptr);
	if (ext.overflow) return fail(c, MSD_EINVAL, ext.overflow == kRowsInputOverflows ? "rows * row_stride overflows" : "rows * k overflows");
	if (rows == 0 || k == 0) return MSD_OK;
	if (!d_keys || !d_out_keys) return fail(c, MSD_EINVAL, "null data pointer");
	const Span buf[3] = { { d_keys, ext.in_bytes, es }, { d_out_keys, ext.out_bytes, es }, { d_out_idx, ext.idx_bytes, 8 } };
	if (first_misaligned(buf) >= 0) return fail(c, MSD_EINVAL, "input and output buffers must be aligned to their element size");
	if (d_out_idx && es == 4 && row_len > ((uint64_t)1 << 32))
		return fail(c, MSD_EINVAL, "indices of a 32-bit key type need row_len <= 2^32 (the position travels in 32 bits)");
	if (outputs_overlap(buf, 1)) return fail(c, MSD_EINVAL, "the outputs must not overlap the input or each other");
	const bool inside = rows_in_envelope(row_len, k);
	if (c->opt.topk_rows_mode == 2 && !inside)
		return fail(c, MSD_EINVAL, "topk_rows_mode 2: the row kernel takes row_len <= %llu and k <= %u", (unsigned long long)kRowsMaxLen, kRowsMaxK);
	const bool kernel = inside && (c->opt.topk_rows_mode == 2 || (c->opt.topk_rows_mode == 0 && rows_kernel_wins(rows, row_len)));
	HIPCHK(c, hipSetDevice(c->device));
	int rc;
	if (kernel) {
		c->stat_written = 0;
		rc = with_key_type(key_type, [&](auto k0, auto) { // (the 4-byte / 8-byte choice only: the row kernel decodes every type)
			typedef decltype(k0) K;
			return rows_kernel_path<K>(c, (const K *)d_keys, key_type, rows, row_len, row_stride, k, which, (K *)d_out_keys, d_out_idx);
		});
	} else
		rc = rows_looped_path(c, (const char *)d_keys, key_type, rows, row_len, row_stride, k, which, (char *)d_out_keys, d_out_idx);
	if (rc) return rc;
	set_stat(c, kStatTopkRowsKernelRows, kernel ? rows : 0);
	set_stat(c, kStatTopkRowsLoopedRows, kernel ? 0 : rows);
	return MSD_OK;
}

} // extern "C"

// ---- per-row sort (msd_sort_rows.hpp)

// the envelope: what the 1024-lane shape holds
static uint64_t sort_rows_max_len(int key_bytes, bool idx)
{
	return with_width(key_bytes, [&](auto k0) { return with_flag(idx, [](auto i) { return (uint64_t)sort_rows_cap<decltype(k0), decltype(i)::value, 1024>(); }); });
}

// Mode 0 inside the envelope: does the row kernel beat the segment path?  (profiles/sort_rows_sweep.jsonl; DESIGN.md section
// 10.4, "Dispatch".)  32-bit keys: always, by 1.3 to 40 times.  64-bit keys (measured on random bits, where the row kernel
// needs all eight passes and the segment sort's leaves two): up to 512 keys per row always; with positions not beyond that
// ([8192, 1024]: 0.41 against 0.20 ms), without them below 4096 keys ([65536, 4096]: 4.9 against 4.1 ms; [16384, 16384]: 6.5
// against 3.0 ms).  The segment path has its own rules for the outputs (16-byte aligned): where they do not hold, the kernel.
static bool sort_rows_kernel_wins(uint64_t key_bytes, bool idx, uint64_t row_len, bool segments_possible)
{
	if (key_bytes == 4 || !segments_possible) return true;
	return idx ? row_len <= 512 : row_len < 4096;
}

// Lanes per row: the smallest group that holds the row -- a wave up to 512 keys, 256 lanes up to 4096, 1024 lanes beyond
// (profiles/sort_rows_sweep.jsonl, the `lanes*` columns: at every row length a narrower group that holds the row beats a
// wider one, by 1.4 to 50 times at 64 MiB).  A forced shape holds where the row fits it.
template <typename K, bool IDX> static int sort_rows_lanes(const msd_ctx *c, uint64_t row_len)
{
	constexpr uint64_t cap64 = sort_rows_cap<K, IDX, 64>(), cap256 = sort_rows_cap<K, IDX, 256>();
	const int by_shape = row_len <= cap64 ? 64 : row_len <= cap256 ? 256 : 1024;
	const int forced = c->opt.sort_rows_lanes;
	if (forced == 0 || (forced == 64 && row_len > cap64) || (forced == 256 && row_len > cap256)) return by_shape;
	return forced;
}

template <typename K, bool IDX>
static int sort_rows_kernel_path(msd_ctx *c, const K *keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t stride, int order, K *out, uint64_t *out_idx)
{
	const K flip = order == MSD_DESCENDING ? (K)~(K)0 : (K)0;
	const KeyCodec<K> codec = key_codec<K>(key_type);
	const int lanes = sort_rows_lanes<K, IDX>(c, row_len);
	c->stat_written = 0;
	phase_begin(c);
	const int rc = with_lanes(lanes, [&](auto l) {
		constexpr int LANES = decltype(l)::value;
		typedef SortRowsCfg<K, IDX, LANES> C;
		constexpr uint64_t groups = C::BLOCK / LANES;
		// workgroups a CU holds at once (LDS: 160 KiB; registers: one 1024-thread workgroup); the rest of the rows in a loop
		const uint64_t per_cu = LANES == 1024 ? 1 : LANES == 256 ? 4 : 6;
		const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->sm_count * per_cu, (rows + groups - 1) / groups));
		return LAUNCH_RC(c, (sort_rows_kernel<K, IDX, LANES>), grid, C::BLOCK, (SortRowsLds<K, IDX, LANES>::bytes), keys, rows, row_len, stride, flip, codec, out, out_idx);
	});
	if (rc) return rc;
	phase_mark(c, "sort_rows");
	phase_end(c);
	set_stat(c, kStatSortRowsLanes, (uint64_t)lanes);
	return MSD_OK;
}

// Rows of any length: codes of the rows, contiguous, in the output; the segment sort on them (host-blocking, as
// msd_sort_*_segments); keys again.  32-bit keys with positions are sorted as (code << 32 | position) in the index array.
template <typename K>
static int sort_rows_segments(msd_ctx *c, const K *keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t stride, int order, K *out, uint64_t *out_idx)
{
	const K flip = order == MSD_DESCENDING ? (K)~(K)0 : (K)0;
	const KeyCodec<K> fcodec = key_codec<K>(key_type).flipped(flip);
	const uint64_t total = rows * row_len;
	const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->sm_count * 16, (total + 255) / 256));
	std::vector<uint64_t> off(rows + 1);
	for (uint64_t r = 0; r <= rows; ++r) off[r] = r * row_len;
	constexpr bool PACK = sizeof(K) == 4;
	bool packed = false;
	int rc;
	if (!out_idx) {
		LAUNCH(c, (rows_encode_kernel<K, false>), grid, 256, 0, keys, rows, row_len, stride, fcodec, out, out_idx);
		rc = sort_segments<K, NoVal>(c, out, nullptr, total, off.data(), (uint32_t)rows, (int)sizeof(K) * 8);
	} else if constexpr (PACK) {
		packed = true;
		LAUNCH(c, rows_pack_kernel, grid, 256, 0, keys, rows, row_len, stride, fcodec, out_idx);
		rc = sort_segments<uint64_t, NoVal>(c, out_idx, nullptr, total, off.data(), (uint32_t)rows, 64);
	} else {
		LAUNCH(c, (rows_encode_kernel<K, true>), grid, 256, 0, keys, rows, row_len, stride, fcodec, out, out_idx);
		rc = sort_segments<uint64_t, uint64_t>(c, out, out_idx, total, off.data(), (uint32_t)rows, 64);
	}
	if (rc) return rc; // (the outputs hold codes)
	rc = tail_phase(c, "sort_rows", [&]() -> int {
		if (packed) {
			if constexpr (PACK) LAUNCH(c, rows_unpack_kernel, grid, 256, 0, out_idx, total, fcodec, out);
		} else
			LAUNCH(c, (rows_decode_kernel<K>), grid, 256, 0, out, total, fcodec);
		return MSD_OK;
	});
	if (rc) return rc;
	set_stat(c, kStatSortRowsLanes, 0);
	return MSD_OK;
}

extern "C" {

int msd_sort_rows_limits(int key_type, int with_idx, uint64_t *max_row_len)
{
	if (!key_type_ok(key_type) || !max_row_len) return MSD_EINVAL;
	*max_row_len = sort_rows_max_len(key_type_bytes(key_type), with_idx != 0);
	return MSD_OK;
}

int msd_sort_rows(msd_ctx *c, const void *d_keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t row_stride, int order, void *d_out_keys,
		  uint64_t *d_out_idx)
{
	if (!c) return MSD_EINVAL;
	if (int rc = check_key_type(c, key_type)) return rc;
	if (int rc = check_order(c, order)) return rc;
	if (row_stride < row_len) return fail(c, MSD_EINVAL, "row_stride must not be smaller than row_len");
	const uint32_t es = (uint32_t)key_type_bytes(key_type);
	const RowsExtents ext = rows_extents(rows, row_len, row_stride, row_len, es, d_out_idx != nullptr);
	if (ext.overflow) return fail(c, MSD_EINVAL, ext.overflow == kRowsInputOverflows ? "rows * row_stride overflows" : "rows * row_len overflows");
	if (rows == 0 || row_len == 0) return MSD_OK;
	if (!d_keys || !d_out_keys) return fail(c, MSD_EINVAL, "null data pointer");
	// in place the input IS the output (the same extent): it has no span of its own
	const bool in_place = d_out_keys == d_keys && row_stride == row_len;
	const Span buf[3] = { { in_place ? nullptr : d_keys, in_place ? 0 : ext.in_bytes, es }, { d_out_keys, ext.out_bytes, es }, { d_out_idx, ext.idx_bytes, 8 } };
	if (first_misaligned(buf) >= 0) return fail(c, MSD_EINVAL, "input and output buffers must be aligned to their element size");
	if (outputs_overlap(buf, 1))
		return fail(c, MSD_EINVAL, "the outputs must not overlap the input (but d_out_keys == d_keys with row_stride == row_len) or each other");
	const uint64_t max_len = sort_rows_max_len((int)es, d_out_idx != nullptr);
	const bool inside = row_len <= max_len;
	if (c->opt.sort_rows_mode == 2 && !inside)
		return fail(c, MSD_EINVAL, "sort_rows_mode 2: the row kernel takes row_len <= %llu for this key type", (unsigned long long)max_len);
	// the segment path's own rules for the outputs and the sizes (a null d_out_idx is aligned)
	const bool seg_aligned = aligned16(d_out_keys) && aligned16(d_out_idx), seg_fits = rows < ((uint64_t)1 << 32) && ext.out_elems < kMaxElems;
	const bool kernel = inside && (c->opt.sort_rows_mode == 2 || (c->opt.sort_rows_mode == 0 && sort_rows_kernel_wins(es, d_out_idx != nullptr, row_len, seg_aligned && seg_fits)));
	if (!kernel && !seg_aligned)
		return fail(c, MSD_EINVAL, "rows beyond the row kernel (row_len > %llu, or sort_rows_mode 1) go through the segment sort, whose rule this is: "
					   "d_out_keys and d_out_idx must be 16-byte aligned",
			    (unsigned long long)max_len);
	if (!kernel && !seg_fits) return fail(c, MSD_EINVAL, "the segment sort takes fewer than 2^32 rows and 2^36 elements");
	HIPCHK(c, hipSetDevice(c->device));
	const int rc = with_key_type(key_type, [&](auto k0, auto) { // (the 4-byte / 8-byte choice only: the codec is two run-time words)
		typedef decltype(k0) K;
		const K *in = (const K *)d_keys;
		K *out = (K *)d_out_keys;
		if (!kernel) return sort_rows_segments<K>(c, in, key_type, rows, row_len, row_stride, order, out, d_out_idx);
		return with_flag(d_out_idx != nullptr, [&](auto idx) {
			return sort_rows_kernel_path<K, decltype(idx)::value>(c, in, key_type, rows, row_len, row_stride, order, out, d_out_idx);
		});
	});
	if (rc) return rc;
	set_stat(c, kStatSortRowsKernelRows, kernel ? rows : 0);
	set_stat(c, kStatSortRowsSegmentRows, kernel ? 0 : rows);
	return MSD_OK;
}

} // extern "C"

// ---- run-length encode (msd_runs.hpp)

// What every entry point that counts per tile begins with (msd_run_encode, msd_reduce_runs, msd_compact, msd_set_sorted,
// msd_join_groups; msd_join_pairs with groups in the place of tiles): `count` launches what writes one word per tile to
// s.tile_counts, the words are scanned in place -- a tile's base is tile_out_base(s.tile_counts, s.piece_sums, t) -- and the
// total goes to *d_total.  The scratch -- with_splits one split per tile plus one, one word per tile, one per scan piece,
// then whatever `more` takes from the Bump -- is the slab's, like a sort round's: the next call on the context overwrites
// it, in stream order.  The caller's phase begins here, behind the carve; the caller marks and ends it.  An empty input
// (tiles == 0: s.tiles stays 0) is one launch that writes a total of 0, and starts[0] = 0 where starts is given.
// scan_pieces false: `count` has scanned the pieces itself (join_offsets_kernel) and only the top level is left.
struct RunsScratch { uint64_t tiles = 0, pieces = 0, *splits = nullptr, *tile_counts = nullptr, *piece_sums = nullptr; };
template <typename F> static int runs_scratch_carve(msd_ctx *c, RunsScratch &s, uint64_t tiles, bool with_splits, F &&more)
{
	s.tiles = tiles;
	s.pieces = (tiles + kRunsScanTile - 1) / kRunsScanTile;
	return slab_carve(c, [&](Bump &b) {
		if (with_splits) s.splits = b.take<uint64_t>(s.tiles + 1);
		s.tile_counts = b.take<uint64_t>(s.tiles);
		s.piece_sums = b.take<uint64_t>(s.pieces);
		more(b);
	});
}
static int runs_scan_counts(msd_ctx *c, const RunsScratch &s, uint64_t *d_total, bool scan_pieces)
{
	if (scan_pieces) LAUNCH(c, runs_scan_pieces_kernel, (unsigned)s.pieces, kRunsScanTh, 0, s.tile_counts, s.tiles, s.piece_sums);
	LAUNCH(c, runs_scan_top_kernel, 1, kRunsScanTh, 0, s.piece_sums, s.pieces, d_total);
	return MSD_OK;
}
template <typename CNT, typename F>
static int runs_count_scan(msd_ctx *c, uint64_t tiles, bool with_splits, uint64_t *d_total, uint64_t *starts, CNT &&count, F &&more, RunsScratch &s, bool scan_pieces = true)
{
	if (tiles == 0) {
		phase_begin(c);
		LAUNCH(c, runs_empty_kernel, 1, 64, 0, d_total, starts);
		return MSD_OK;
	}
	if (int rc = runs_scratch_carve(c, s, tiles, with_splits, more)) return rc;
	phase_begin(c);
	if (int rc = count()) return rc;
	return runs_scan_counts(c, s, d_total, scan_pieces);
}
// (the runs of an array: msd_run_encode, msd_reduce_runs)
template <typename E, typename F> static int runs_count_scan(msd_ctx *c, const E *data, uint64_t n, uint64_t *num_runs, uint64_t *starts, F &&more, RunsScratch &s)
{
	return runs_count_scan(c, n ? runs_tiles(data, n) : 0, false, num_runs, starts, // (tiles <= 2^25 + 1)
			       [&] { return LAUNCH_RC(c, (runs_count_kernel<E>), (unsigned)s.tiles, kRunsTh, 0, data, n, s.tile_counts); }, more, s);
}

// The shared body of the *_limits exports: *tile = the TILE of Cfg at this width, then every further (pointer, value)
template <template <typename> class Cfg> static int tile_limits(int key_bytes, uint64_t *tile, std::initializer_list<std::pair<uint64_t *, uint64_t>> more = {})
{
	if ((key_bytes != 4 && key_bytes != 8) || !tile) return MSD_EINVAL;
	for (const auto &p : more)
		if (!p.first) return MSD_EINVAL;
	*tile = with_width(key_bytes, [](auto e) { return (uint64_t)Cfg<decltype(e)>::TILE; });
	for (const auto &p : more) *p.first = p.second;
	return MSD_OK;
}

// Count, scan, write: four launches one behind the other on the stream, nothing read back.
template <typename E>
static int run_encode_impl(msd_ctx *c, const E *data, uint64_t n, uint64_t cap, E *values, uint64_t *starts, const uint64_t *positions, uint64_t *inverse,
			   uint64_t *num_runs)
{
	RunsScratch s;
	if (int rc = runs_count_scan(c, data, n, num_runs, starts, [](Bump &) {}, s)) return rc;
	if (s.tiles && (inverse || values || starts)) {
		// (positions only go with an inverse: there is no <E, false, true> instance)
		const int rc = with_flag(inverse != nullptr, [&](auto inv) {
			return with_flag(inverse && positions, [&](auto pos) {
				constexpr bool INV = decltype(inv)::value, POS = INV && decltype(pos)::value;
				return LAUNCH_RC(c, (runs_write_kernel<E, INV, POS>), (unsigned)s.tiles, kRunsTh, 0, data, n, cap, s.tile_counts, s.piece_sums, values, starts, positions, inverse);
			});
		});
		if (rc) return rc;
	}
	phase_mark(c, "run_encode");
	phase_end(c);
	return MSD_OK;
}

extern "C" {

int msd_run_encode_limits(int elem_bytes, uint64_t *tile, uint64_t *scan_tile) { return tile_limits<RunsCfg>(elem_bytes, tile, { { scan_tile, kRunsScanTile } }); }

int msd_run_encode(msd_ctx *c, const void *d_data, int elem_bytes, uint64_t n, uint64_t cap, void *d_values, uint64_t *d_starts, const uint64_t *d_positions,
		   uint64_t *d_inverse, uint64_t *d_num_runs)
{
	if (!c) return MSD_EINVAL;
	if (elem_bytes != 4 && elem_bytes != 8) return fail(c, MSD_EINVAL, "elem_bytes must be 4 or 8");
	if (!d_num_runs) return fail(c, MSD_EINVAL, "d_num_runs is required");
	if (n && !d_data) return fail(c, MSD_EINVAL, "null data pointer");
	// the extents: inputs first, then the outputs; at most min(cap, n) runs are stored (n at most 2^36 - 1 wherever an extent is looked at)
	const uint32_t es = (uint32_t)elem_bytes;
	const uint64_t stored = std::min({ cap, n, kMaxElems });
	const Span buf[6] = { span_of(d_data, n, es),          span_of(d_positions, n, 8), span_of(d_values, stored, es),
			      span_of(d_starts, stored + 1, 8), span_of(d_inverse, n, 8),   span_of(d_num_runs, 1, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_data, d_values: elem_bytes; the others: 8)");
	if (n >= kMaxElems) return fail(c, MSD_EINVAL, "n too large: fewer than 2^36 elements");
	if (d_positions && !d_inverse) return fail(c, MSD_EINVAL, "d_positions without d_inverse");
	if (outputs_overlap(buf, 2))
		return fail(c, MSD_EINVAL, "the outputs must not overlap the input, d_positions or each other (in-place compaction is not offered)");
	HIPCHK(c, hipSetDevice(c->device));
	return with_width(elem_bytes, [&](auto e) {
		typedef decltype(e) E;
		return run_encode_impl<E>(c, (const E *)d_data, n, cap, (E *)d_values, d_starts, d_positions, d_inverse, d_num_runs);
	});
}

} // extern "C"

// ---- reduce-by-key over runs (msd_reduce.hpp)

// Count, scan, reduce, carry, apply: seven launches one behind the other on the stream, nothing read back.  The scratch --
// per tile the count, the lead and the heads, and the same per scan piece -- is the slab's (runs_count_scan).
template <typename E, typename P>
static int reduce_runs_impl(msd_ctx *c, const E *keys, uint64_t n, const void *vals, const uint64_t *positions, uint64_t cap, void *out, uint64_t *num_runs,
			    KeyCodec<typename P::R::O> cd)
{
	typedef typename P::R R;
	RunsScratch s;
	SegRecord rec{ nullptr, nullptr }, piece{ nullptr, nullptr };
	const auto records = [&](Bump &b) {
		rec.val = b.take<uint64_t>(s.tiles);
		rec.flag = b.take<uint32_t>(s.tiles);
		piece.val = b.take<uint64_t>(s.pieces);
		piece.flag = b.take<uint32_t>(s.pieces);
	};
	if (int rc = runs_count_scan(c, keys, n, num_runs, nullptr, records, s)) return rc;
	if (s.tiles && cap) { // (cap == 0 only counts)
		const int rc = with_flag(positions != nullptr, [&](auto pos) {
			return LAUNCH_RC(c, (reduce_tile_kernel<E, P, decltype(pos)::value>), (unsigned)s.tiles, kRunsTh, 0, keys, n, vals, positions, cap, s.tile_counts, s.piece_sums, cd, out, rec);
		});
		if (rc) return rc;
		LAUNCH(c, (seg_carry_pieces_kernel<R, false>), (unsigned)s.pieces, kRunsScanTh, 0, rec, s.tiles, cd, piece);
		LAUNCH(c, (seg_carry_top_kernel<R, false>), 1, kRunsScanTh, 0, piece, s.pieces, cd);
		LAUNCH(c, (reduce_apply_kernel<R>), (unsigned)((s.tiles + 255) / 256), 256, 0, rec, piece, s.tiles, cap, s.tile_counts, s.piece_sums, cd, out);
	}
	phase_mark(c, "reduce_runs");
	phase_end(c);
	return MSD_OK;
}

// (op, val_type) -> f(the policy of msd_reduce.hpp, the codec of its results).  A maximum is the minimum of the complemented codes.
enum class RedOp { Sum, Min, Max };
template <typename F> static int with_reduction(RedOp op, int val_type, F &&f)
{
	if (op == RedOp::Sum) {
		const KeyCodec<uint64_t> none{ 0, 0 };
		switch (val_type) {
		case kKeyU32: return f(SumU32(), none);
		case kKeyI32: return f(SumI32(), none);
		case kKeyF32: return f(SumF32(), none);
		case kKeyF64: return f(SumF64(), none);
		default: return f(SumX64(), none); // (U64, I64: the same sum modulo 2^64)
		}
	}
	const bool mx = op == RedOp::Max;
	if (key_type_bytes(val_type) == 4) return f(MinOf<uint32_t>(), key_codec<uint32_t>(val_type).flipped(mx ? ~0u : 0u));
	return f(MinOf<uint64_t>(), key_codec<uint64_t>(val_type).flipped(mx ? ~0ull : 0ull));
}

template <typename E>
static int reduce_runs_typed(msd_ctx *c, const E *keys, uint64_t n, const void *vals, int val_type, const uint64_t *positions, int op, uint64_t cap, void *out,
			     uint64_t *num_runs)
{
	const RedOp r = op == MSD_REDUCE_SUM ? RedOp::Sum : op == MSD_REDUCE_MIN ? RedOp::Min : RedOp::Max;
	return with_reduction(r, val_type, [&](auto p, auto cd) { return reduce_runs_impl<E, decltype(p)>(c, keys, n, vals, positions, cap, out, num_runs, cd); });
}

extern "C" {

int msd_reduce_runs_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile) { return msd_run_encode_limits(key_bytes, tile, scan_tile); }

int msd_reduce_runs(msd_ctx *c, const void *d_keys, int key_bytes, uint64_t n, const void *d_vals, int val_type, const uint64_t *d_positions, int op, uint64_t cap,
		    void *d_out, uint64_t *d_num_runs)
{
	if (!c) return MSD_EINVAL;
	if (key_bytes != 4 && key_bytes != 8) return fail(c, MSD_EINVAL, "key_bytes must be 4 or 8");
	if (!key_type_ok(val_type)) return fail(c, MSD_EINVAL, "unknown val_type");
	if (op != MSD_REDUCE_SUM && op != MSD_REDUCE_MIN && op != MSD_REDUCE_MAX) return fail(c, MSD_EINVAL, "unknown op");
	if (!d_num_runs) return fail(c, MSD_EINVAL, "d_num_runs is required");
	if (n && (!d_keys || !d_vals)) return fail(c, MSD_EINVAL, "null keys or values pointer");
	if (n && cap && !d_out) return fail(c, MSD_EINVAL, "null d_out pointer");
	// the extents: inputs first, then the outputs; at most min(cap, n) runs are stored, a sum as 8 bytes
	const uint32_t ks = (uint32_t)key_bytes, vs = (uint32_t)key_type_bytes(val_type), os = op == MSD_REDUCE_SUM ? 8 : vs;
	const Span buf[5] = { span_of(d_keys, n, ks), span_of(d_vals, n, vs), span_of(d_positions, n, 8), span_of(d_out, std::min(cap, n), os), span_of(d_num_runs, 1, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_keys: key_bytes; d_vals: the value's; d_out: 8 for a sum, else the value's; the others: 8)");
	if (n >= kMaxElems) return fail(c, MSD_EINVAL, "n too large: fewer than 2^36 elements");
	if (outputs_overlap(buf, 3)) return fail(c, MSD_EINVAL, "d_out and d_num_runs must not overlap the keys, the values, d_positions or each other");
	HIPCHK(c, hipSetDevice(c->device));
	return with_width(key_bytes, [&](auto k0) {
		return reduce_runs_typed(c, (const decltype(k0) *)d_keys, n, d_vals, val_type, d_positions, op, cap, d_out, d_num_runs);
	});
}

} // extern "C"

// ---- scan-by-key over runs (msd_scan.hpp)

// Tail, carry (pieces, top), tile: four launches one behind the other on the stream, nothing read back.  The scratch -- per
// tile and per scan piece one 8-byte tail and one 4-byte flag -- is the slab's, like a sort round's.
template <typename E, typename P>
static int scan_runs_impl(msd_ctx *c, const E *keys, uint64_t n, const void *vals, int flags, void *out, KeyCodec<typename P::R::O> cd)
{
	typedef typename P::R R;
	const uint64_t tiles = runs_tiles(keys, n), pieces = (tiles + kRunsScanTile - 1) / kRunsScanTile; // (tiles <= 2^25 + 1)
	SegRecord rec{ nullptr, nullptr }, piece{ nullptr, nullptr };
	if (int rc = slab_carve(c, [&](Bump &b) {
		    rec.val = b.take<uint64_t>(tiles);
		    rec.flag = b.take<uint32_t>(tiles);
		    piece.val = b.take<uint64_t>(pieces);
		    piece.flag = b.take<uint32_t>(pieces);
	    }))
		return rc;
	phase_begin(c);
	LAUNCH(c, (scan_tail_kernel<E, P>), (unsigned)tiles, kRunsTh, 0, keys, n, vals, cd, rec);
	LAUNCH(c, (seg_carry_pieces_kernel<R, true>), (unsigned)pieces, kRunsScanTh, 0, rec, tiles, cd, piece);
	LAUNCH(c, (seg_carry_top_kernel<R, true>), 1, kRunsScanTh, 0, piece, pieces, cd);
	LAUNCH(c, (scan_tile_kernel<E, P>), (unsigned)tiles, kRunsTh, 0, keys, n, vals, cd, rec, piece, flags, out);
	phase_mark(c, "scan_runs");
	phase_end(c);
	return MSD_OK;
}

template <typename E>
static int scan_runs_typed(msd_ctx *c, const E *keys, uint64_t n, const void *vals, int val_type, int op, int flags, void *out)
{
	if (op == MSD_SCAN_COUNT) return scan_runs_impl<E, CountOne>(c, keys, n, nullptr, flags, out, KeyCodec<uint64_t>{ 0, 0 });
	const RedOp r = op == MSD_SCAN_SUM ? RedOp::Sum : op == MSD_SCAN_MIN ? RedOp::Min : RedOp::Max;
	return with_reduction(r, val_type, [&](auto p, auto cd) { return scan_runs_impl<E, decltype(p)>(c, keys, n, vals, flags, out, cd); });
}

extern "C" {

int msd_scan_runs_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile) { return msd_run_encode_limits(key_bytes, tile, scan_tile); }

int msd_scan_runs(msd_ctx *c, const void *d_keys, int key_bytes, uint64_t n, const void *d_vals, int val_type, const uint64_t *d_positions, int op, int flags,
		  void *d_out)
{
	if (!c) return MSD_EINVAL;
	if (key_bytes != 4 && key_bytes != 8) return fail(c, MSD_EINVAL, "key_bytes must be 4 or 8");
	if (op != MSD_SCAN_SUM && op != MSD_SCAN_MIN && op != MSD_SCAN_MAX && op != MSD_SCAN_COUNT) return fail(c, MSD_EINVAL, "unknown op");
	const bool count = op == MSD_SCAN_COUNT;
	if (!count && !key_type_ok(val_type)) return fail(c, MSD_EINVAL, "unknown val_type");
	if (flags & ~(MSD_SCAN_EXCLUSIVE | MSD_SCAN_SCATTER)) return fail(c, MSD_EINVAL, "unknown flags");
	if ((flags & MSD_SCAN_SCATTER) && !d_positions) return fail(c, MSD_EINVAL, "MSD_SCAN_SCATTER without d_positions");
	if (d_positions) return fail(c, MSD_EINVAL, "d_positions is not offered yet: it must be null (and with it MSD_SCAN_SCATTER is not offered)");
	if (n && !d_keys) return fail(c, MSD_EINVAL, "null keys pointer");
	if (n && !count && !d_vals) return fail(c, MSD_EINVAL, "null values pointer");
	if (n && !d_out) return fail(c, MSD_EINVAL, "null d_out pointer");
	// the extents: inputs first, then the output; a sum and a count as 8 bytes, a count reads no values
	const uint32_t ks = (uint32_t)key_bytes, vs = count ? 1 : (uint32_t)key_type_bytes(val_type), os = op == MSD_SCAN_SUM || count ? 8 : vs;
	const Span buf[3] = { span_of(d_keys, n, ks), span_of(count ? nullptr : d_vals, n, vs), span_of(d_out, n, os) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_keys: key_bytes; d_vals: the value's; d_out: 8 for a sum or a count, else the value's)");
	if (n >= kMaxElems) return fail(c, MSD_EINVAL, "n too large: fewer than 2^36 elements");
	if (outputs_overlap(buf, 2)) return fail(c, MSD_EINVAL, "d_out must not overlap the keys or the values (in place is not offered)");
	if (n == 0) return MSD_OK;
	HIPCHK(c, hipSetDevice(c->device));
	return with_width(key_bytes, [&](auto k0) {
		return scan_runs_typed(c, (const decltype(k0) *)d_keys, n, count ? nullptr : d_vals, val_type, op, flags, d_out);
	});
}

} // extern "C"

// ---- stream compaction and stable partition (msd_compact.hpp)

// Count, scan, write: four launches one behind the other on the stream, nothing read back.  The scratch -- one word per
// tile and one per scan piece -- is the slab's, like msd_run_encode's.  in.keys is what the write pass reads (null where it
// needs no keys); the count reads keys for the range test only.  n == 0 is one launch that writes a count of 0.
template <typename E, bool RANGE, bool MASK, int VB, bool REST>
static int compact_impl(msd_ctx *c, const CompactIn<E> &in, const void *vals, uint64_t cap, E *out_keys, void *out_vals, uint64_t *out_idx, uint64_t *count)
{
	CompactIn<E> cin = in;
	if (!RANGE) cin.keys = nullptr;
	RunsScratch s;
	const uint64_t tiles = in.n ? (in.m + in.n + RunsCfg<E>::TILE - 1) / RunsCfg<E>::TILE : 0; // (<= 2^25 + 1)
	if (int rc = runs_count_scan(c, tiles, false, count, nullptr,
				     [&] { return LAUNCH_RC(c, (compact_count_kernel<E, RANGE, MASK>), (unsigned)s.tiles, kRunsTh, 0, cin, s.tile_counts); }, [](Bump &) {}, s))
		return rc;
	if (s.tiles && (out_keys || out_vals || out_idx)) // (none: the call only counts)
		LAUNCH(c, (compact_write_kernel<E, RANGE, MASK, VB, REST>), (unsigned)s.tiles, kRunsTh, 0, in, vals, cap, s.tile_counts, s.piece_sums, count, out_keys, out_vals, out_idx);
	phase_mark(c, "compact");
	phase_end(c);
	return MSD_OK;
}

// the values' width -> f(std::integral_constant<int, 0 | 4 | 8>())
template <typename F> static int with_val_bytes(int vb, F &&f)
{
	if (vb == 4) return f(std::integral_constant<int, 4>());
	if (vb == 8) return f(std::integral_constant<int, 8>());
	return f(std::integral_constant<int, 0>());
}

template <typename E>
static int compact_typed(msd_ctx *c, const CompactIn<E> &in, bool range, bool rest, const void *vals, int vb, uint64_t cap, void *out_keys, void *out_vals,
			 uint64_t *out_idx, uint64_t *count)
{
	return with_flag(range, [&](auto rg) {
		return with_flag(in.mask != nullptr, [&](auto mk) {
			return with_flag(rest, [&](auto rs) {
				return with_val_bytes(vb, [&](auto v) {
					return compact_impl<E, decltype(rg)::value, decltype(mk)::value, decltype(v)::value, decltype(rs)::value>(c, in, vals, cap, (E *)out_keys, out_vals, out_idx,
																		     count);
				});
			});
		});
	});
}

extern "C" {

int msd_compact_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile) { return msd_run_encode_limits(key_bytes, tile, scan_tile); }

int msd_compact(msd_ctx *c, const void *d_keys, int key_type, uint64_t n, const uint8_t *d_mask, uint64_t lo_bits, uint64_t hi_bits, int flags, const void *d_vals,
		int val_bytes, uint64_t cap, void *d_out_keys, void *d_out_vals, uint64_t *d_out_idx, uint64_t *d_count)
{
	if (!c) return MSD_EINVAL;
	if (d_keys && !key_type_ok(key_type)) return fail(c, MSD_EINVAL, "unknown key_type");
	if (flags & ~(MSD_COMPACT_RANGE | MSD_COMPACT_INVERT | MSD_COMPACT_REST)) return fail(c, MSD_EINVAL, "unknown flags");
	if (!d_count) return fail(c, MSD_EINVAL, "d_count is required");
	const bool range = (flags & MSD_COMPACT_RANGE) != 0, rest = (flags & MSD_COMPACT_REST) != 0;
	if ((range || d_out_keys) && !d_keys) return fail(c, MSD_EINVAL, "MSD_COMPACT_RANGE or d_out_keys without d_keys");
	// without keys the grid is the mask's, with the 4-byte geometry (key_type is not looked at)
	const uint32_t es = d_keys ? (uint32_t)key_type_bytes(key_type) : 4u;
	if (range && es == 4 && ((lo_bits | hi_bits) >> 32)) return fail(c, MSD_EINVAL, "a bound of a 32-bit key type has bits above 2^32");
	if ((d_vals != nullptr) != (d_out_vals != nullptr)) return fail(c, MSD_EINVAL, "d_vals and d_out_vals go together");
	if (d_vals && val_bytes != 4 && val_bytes != 8) return fail(c, MSD_EINVAL, "val_bytes must be 4 or 8");
	if (n && !d_keys && !d_mask && (d_out_keys || d_out_vals)) return fail(c, MSD_EINVAL, "neither d_keys nor d_mask: there is nothing to take elements from");
	// the extents: inputs first, then the outputs; at most min(cap, n) elements are stored (REST: cap >= n), n at most 2^36 - 1 wherever an extent is looked at
	const uint32_t vs = d_vals ? (uint32_t)val_bytes : 0u;
	const uint64_t stored = std::min({ cap, n, kMaxElems });
	const Span buf[7] = { span_of(d_keys, n, es),          span_of(d_mask, n, 1),           span_of(d_vals, n, vs ? vs : 1), span_of(d_out_keys, stored, es),
			      span_of(d_out_vals, stored, vs ? vs : 1), span_of(d_out_idx, stored, 8), span_of(d_count, 1, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_keys, d_out_keys: the key's; d_vals, d_out_vals: val_bytes; d_out_idx, d_count: 8)");
	if (n >= kMaxElems) return fail(c, MSD_EINVAL, "n too large: fewer than 2^36 elements");
	if (rest && cap < n) return fail(c, MSD_EINVAL, "MSD_COMPACT_REST needs cap >= n");
	if (outputs_overlap(buf, 3)) return fail(c, MSD_EINVAL, "the outputs must not overlap d_keys, d_mask, d_vals or each other (in-place operation is not offered)");
	HIPCHK(c, hipSetDevice(c->device));
	const bool read_keys = range || d_out_keys; // (the write pass; the count reads them for the range test only)
	return with_width(read_keys ? (int)es : 4, [&](auto k0) {
		typedef decltype(k0) E;
		const KeyCodec<E> cd = range ? key_codec<E>(key_type) : KeyCodec<E>{ 0, 0 };
		const void *grid = read_keys ? d_keys : d_mask ? (const void *)d_mask : nullptr; // whose 16-byte grid the tiles lie on
		const uint32_t m = read_keys ? runs_misalign((const E *)d_keys) : (uint32_t)((uintptr_t)grid & 15u);
		const CompactIn<E> in{ read_keys ? (const E *)d_keys : nullptr, d_mask, n, m, (flags & MSD_COMPACT_INVERT) ? 1u : 0u, cd,
				       range ? cd.enc((E)lo_bits) : (E)0, range ? cd.enc((E)hi_bits) : (E)0 };
		return compact_typed<E>(c, in, range, rest, d_vals, (int)vs, cap, d_out_keys, d_out_vals, d_out_idx, d_count);
	});
}

} // extern "C"

// ---- sorted search (msd_search.hpp)

// Direct: one launch.  Merge: the splits, then the tiles, one behind the other on the stream; the scratch -- one split per
// tile plus one -- is the slab's, as for msd_run_encode.  Nothing is read back.
template <typename K, bool POS> // (POS: through positions)
static int search_sorted_impl(msd_ctx *c, const K *keys, int key_type, uint64_t n, const K *needles, uint64_t m, bool merge, uint32_t right,
			      const uint64_t *positions, uint64_t *out)
{
	const KeyCodec<K> cd = key_codec<K>(key_type);
	if (!merge) {
		const unsigned grid = (unsigned)((m + kSearchDirectTile - 1) / kSearchDirectTile); // (m < 2^36: at most 2^26)
		phase_begin(c);
		LAUNCH(c, (search_direct_kernel<K, POS>), grid, kSearchTh, 0, keys, n, needles, m, right, cd, positions, out);
		phase_mark(c, "search_sorted");
		phase_end(c);
		return MSD_OK;
	}
	const uint64_t tiles = (n + m + SearchCfg<K>::TILE - 1) / SearchCfg<K>::TILE; // (n + m < 2^37: at most 2^26)
	uint64_t *splits = nullptr;
	if (int rc = slab_carve(c, [&](Bump &b) { splits = b.take<uint64_t>(tiles + 1); })) return rc;
	phase_begin(c);
	LAUNCH(c, (search_split_kernel<K, SearchCfg<K>::TILE>), (unsigned)((tiles + 1 + kSearchTh - 1) / kSearchTh), kSearchTh, 0, keys, n, needles, m, right, cd, tiles, splits);
	LAUNCH(c, (search_tile_kernel<K, POS>), (unsigned)tiles, kSearchTh, 0, keys, n, needles, m, right, cd, splits, positions, out);
	phase_mark(c, "search_sorted");
	phase_end(c);
	return MSD_OK;
}

extern "C" {

int msd_search_sorted_limits(int key_bytes, uint64_t *tile, uint64_t *direct_tile) { return tile_limits<SearchCfg>(key_bytes, tile, { { direct_tile, kSearchDirectTile } }); }

int msd_search_sorted(msd_ctx *c, const void *d_sorted, int key_type, uint64_t n, const void *d_needles, uint64_t m, int needles_sorted, int side,
		      const uint64_t *d_positions, uint64_t *d_out)
{
	if (!c) return MSD_EINVAL;
	if (!key_type_ok(key_type)) return fail(c, MSD_EINVAL, "unknown key_type");
	if (side != MSD_SEARCH_LEFT && side != MSD_SEARCH_RIGHT) return fail(c, MSD_EINVAL, "side must be MSD_SEARCH_LEFT or MSD_SEARCH_RIGHT");
	if (needles_sorted != 0 && needles_sorted != 1) return fail(c, MSD_EINVAL, "needles_sorted must be 0 or 1");
	if (m && !d_out) return fail(c, MSD_EINVAL, "null d_out pointer");
	if (m && !d_needles) return fail(c, MSD_EINVAL, "null d_needles pointer");
	if (m && n && !d_sorted) return fail(c, MSD_EINVAL, "null d_sorted pointer");
	// the extents: the inputs, then d_out (a null d_sorted is empty)
	const uint32_t es = (uint32_t)key_type_bytes(key_type);
	const Span buf[4] = { span_of(d_sorted, n, es), span_of(d_needles, m, es), span_of(d_positions, m, 8), span_of(d_out, m, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_sorted, d_needles: the key's width; d_positions, d_out: 8)");
	if (n >= kMaxElems || m >= kMaxElems) return fail(c, MSD_EINVAL, "n or m too large: fewer than 2^36 elements each");
	if (m && outputs_overlap(buf, 3)) return fail(c, MSD_EINVAL, "d_out must not overlap d_sorted, d_needles or d_positions");
	if (m == 0) return MSD_OK; // nothing to write
	const bool merge = needles_sorted && c->opt.search_mode != 1 && (c->opt.search_mode == 2 || n / c->opt.search_merge_ratio <= m);
	HIPCHK(c, hipSetDevice(c->device));
	return with_width((int)es, [&](auto k0) {
		return with_flag(d_positions != nullptr, [&](auto pos) {
			typedef decltype(k0) K;
			return search_sorted_impl<K, decltype(pos)::value>(c, (const K *)d_sorted, key_type, n, (const K *)d_needles, m, merge, (uint32_t)side, d_positions, d_out);
		});
	});
}

} // extern "C"

// ---- merge of two sorted arrays (msd_merge2.hpp)

// The merge path's cut of [a; b] into tiles of MergeCfg: the split kernel of the sorted search with the RIGHT rule
template <typename K> static int merge_split(msd_ctx *c, const K *a, uint64_t n, const K *b, uint64_t m, KeyCodec<K> cd, uint64_t tiles, uint64_t *splits)
{
	return LAUNCH_RC(c, (search_split_kernel<K, MergeCfg<K>::TILE>), (unsigned)((tiles + 1 + kMergeTh - 1) / kMergeTh), kMergeTh, 0, a, n, b, m, (uint32_t)MSD_SEARCH_RIGHT, cd, tiles,
			 splits);
}

// The splits, then the tiles, one behind the other on the stream; the scratch -- one split per tile plus one -- is the
// slab's, as for msd_search_sorted.  Nothing is read back.
template <typename K, bool VALS, bool ORIGIN>
static int merge_sorted_impl(msd_ctx *c, const K *a, uint64_t n, const K *b, uint64_t m, int key_type, const uint64_t *vals_a, const uint64_t *vals_b, K *out,
			     uint64_t *out_vals, uint64_t *out_origin)
{
	const KeyCodec<K> cd = key_codec<K>(key_type);
	const uint64_t tiles = (n + m + MergeCfg<K>::TILE - 1) / MergeCfg<K>::TILE; // (n + m < 2^37: at most 2^26)
	uint64_t *splits = nullptr;
	if (int rc = slab_carve(c, [&](Bump &bump) { splits = bump.take<uint64_t>(tiles + 1); })) return rc;
	phase_begin(c);
	if (int rc = merge_split(c, a, n, b, m, cd, tiles, splits)) return rc;
	LAUNCH(c, (merge_tile_kernel<K, VALS, ORIGIN>), (unsigned)tiles, kMergeTh, 0, a, n, b, m, cd, splits, vals_a, vals_b, out, out_vals, out_origin);
	phase_mark(c, "merge_sorted");
	phase_end(c);
	return MSD_OK;
}

extern "C" {

int msd_merge_sorted_limits(int key_bytes, uint64_t *tile) { return tile_limits<MergeCfg>(key_bytes, tile); }

int msd_merge_sorted(msd_ctx *c, const void *d_a, uint64_t n, const void *d_b, uint64_t m, int key_type, const uint64_t *d_vals_a, const uint64_t *d_vals_b,
		     void *d_out, uint64_t *d_out_vals, uint64_t *d_out_origin)
{
	if (!c) return MSD_EINVAL;
	if (!key_type_ok(key_type)) return fail(c, MSD_EINVAL, "unknown key_type");
	if ((n || m) && !d_out) return fail(c, MSD_EINVAL, "null d_out pointer");
	if (n && !d_a) return fail(c, MSD_EINVAL, "null d_a pointer");
	if (m && !d_b) return fail(c, MSD_EINVAL, "null d_b pointer");
	if (d_out_vals && ((n && !d_vals_a) || (m && !d_vals_b))) return fail(c, MSD_EINVAL, "d_out_vals without d_vals_a or d_vals_b");
	if (!d_out_vals && (d_vals_a || d_vals_b)) return fail(c, MSD_EINVAL, "d_vals_a or d_vals_b without d_out_vals");
	// the extents: the inputs, then the outputs (a count beyond 2^36 is refused behind the alignment rule; until then n + m saturates)
	const uint32_t es = (uint32_t)key_type_bytes(key_type);
	uint64_t total = 0;
	if (__builtin_add_overflow(n, m, &total)) total = UINT64_MAX;
	const Span buf[7] = { span_of(d_a, n, es),      span_of(d_b, m, es),          span_of(d_vals_a, n, 8),        span_of(d_vals_b, m, 8),
			      span_of(d_out, total, es), span_of(d_out_vals, total, 8), span_of(d_out_origin, total, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_a, d_b, d_out: the key's width; the others: 8)");
	if (n >= kMaxElems || m >= kMaxElems) return fail(c, MSD_EINVAL, "n or m too large: fewer than 2^36 elements each");
	if (total && outputs_overlap(buf, 4)) return fail(c, MSD_EINVAL, "d_out, d_out_vals and d_out_origin must not overlap an input or each other (the merge is not in place)");
	if (total == 0) return MSD_OK; // nothing to write
	HIPCHK(c, hipSetDevice(c->device));
	return with_width((int)es, [&](auto k0) {
		return with_flag(d_out_vals != nullptr, [&](auto vals) {
			return with_flag(d_out_origin != nullptr, [&](auto origin) {
				typedef decltype(k0) K;
				return merge_sorted_impl<K, decltype(vals)::value, decltype(origin)::value>(c, (const K *)d_a, n, (const K *)d_b, m, key_type, d_vals_a, d_vals_b,
													 (K *)d_out, d_out_vals, d_out_origin);
			});
		});
	});
}

} // extern "C"

// ---- set operations on two sorted arrays (msd_setops.hpp)

// What msd_set_sorted and msd_join_groups begin with: the splits, the count per tile of the elements that `keep` keeps, the
// scan of the counts -- four launches one behind the other on the stream; the scratch -- one split per tile plus one, one
// count per tile, one sum per scan piece -- is the slab's (runs_count_scan).  n + m == 0 is one launch that writes a total
// of 0 (s.tiles stays 0).  The caller launches its write kernel and marks and ends the phase.
template <typename K>
static int set_count_scan(msd_ctx *c, const K *a, uint64_t n, const K *b, uint64_t m, KeyCodec<K> cd, uint32_t keep, uint64_t *d_total, RunsScratch &s)
{
	const uint64_t tiles = (n + m + MergeCfg<K>::TILE - 1) / MergeCfg<K>::TILE; // (n + m < 2^37: at most 2^26)
	const auto count = [&] {
		if (int rc = merge_split(c, a, n, b, m, cd, s.tiles, s.splits)) return rc;
		return LAUNCH_RC(c, (set_count_kernel<K>), (unsigned)s.tiles, kMergeTh, 0, a, n, b, m, cd, keep, s.splits, s.tile_counts);
	};
	return runs_count_scan(c, tiles, true, d_total, nullptr, count, [](Bump &) {}, s);
}

// Front, write: five launches, nothing read back.
template <typename K>
static int set_sorted_impl(msd_ctx *c, int op, const K *a, uint64_t n, const K *b, uint64_t m, int key_type, uint64_t cap, K *out, uint64_t *out_origin,
			   uint64_t *num_out)
{
	const KeyCodec<K> cd = key_codec<K>(key_type);
	const uint32_t keep = set_keep_mask(op);
	RunsScratch s;
	if (int rc = set_count_scan(c, a, n, b, m, cd, keep, num_out, s)) return rc;
	if (s.tiles && cap && (out || out_origin)) // (cap == 0, or no output: the count alone)
		LAUNCH(c, (set_write_kernel<K>), (unsigned)s.tiles, kMergeTh, 0, a, n, b, m, cd, keep, s.splits, s.tile_counts, s.piece_sums, num_out, cap, out, out_origin);
	phase_mark(c, "set_sorted");
	phase_end(c);
	return MSD_OK;
}

extern "C" {

int msd_set_sorted_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile) { return tile_limits<MergeCfg>(key_bytes, tile, { { scan_tile, kRunsScanTile } }); }

int msd_set_sorted(msd_ctx *c, int op, const void *d_a, uint64_t n, const void *d_b, uint64_t m, int key_type, uint64_t cap, void *d_out, uint64_t *d_out_origin,
		   uint64_t *d_num_out)
{
	if (!c) return MSD_EINVAL;
	if (!key_type_ok(key_type)) return fail(c, MSD_EINVAL, "unknown key_type");
	if (op != MSD_SET_INTERSECTION && op != MSD_SET_UNION && op != MSD_SET_DIFFERENCE && op != MSD_SET_SYMMETRIC_DIFFERENCE) return fail(c, MSD_EINVAL, "unknown op");
	if (!d_num_out) return fail(c, MSD_EINVAL, "d_num_out is required");
	if (n && !d_a) return fail(c, MSD_EINVAL, "null d_a pointer");
	if (m && !d_b) return fail(c, MSD_EINVAL, "null d_b pointer");
	// the extents: the inputs, then the outputs; at most min(cap, bound) results are stored (a count beyond 2^36 is refused behind the alignment rule; until then n + m saturates)
	const uint32_t es = (uint32_t)key_type_bytes(key_type);
	uint64_t total = 0;
	if (__builtin_add_overflow(n, m, &total)) total = UINT64_MAX;
	const uint64_t bound = op == MSD_SET_INTERSECTION ? std::min(n, m) : op == MSD_SET_DIFFERENCE ? n : total;
	const uint64_t stored = std::min(cap, bound);
	const Span buf[5] = { span_of(d_a, n, es), span_of(d_b, m, es), span_of(d_out, stored, es), span_of(d_out_origin, stored, 8), span_of(d_num_out, 1, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_a, d_b, d_out: the key's width; the others: 8)");
	if (n >= kMaxElems || m >= kMaxElems) return fail(c, MSD_EINVAL, "n or m too large: fewer than 2^36 elements each");
	if (outputs_overlap(buf, 2)) return fail(c, MSD_EINVAL, "d_out, d_out_origin and d_num_out must not overlap an input or each other (the operation is not in place)");
	HIPCHK(c, hipSetDevice(c->device));
	return with_width((int)es, [&](auto k0) {
		typedef decltype(k0) K;
		return set_sorted_impl<K>(c, op, (const K *)d_a, n, (const K *)d_b, m, key_type, cap, (K *)d_out, d_out_origin, d_num_out);
	});
}

} // extern "C"

// ---- sort-merge join of two sorted arrays (msd_join.hpp)

// The groups: the front of msd_set_sorted (set_count_scan) with the intersection's mask, and the join's own write kernel.
template <typename K>
static int join_groups_impl(msd_ctx *c, const K *a, uint64_t n, const K *b, uint64_t m, int key_type, uint64_t cap, K *keys, uint64_t *a_first, uint64_t *a_count,
			    uint64_t *b_first, uint64_t *b_count, uint64_t *num_groups)
{
	const KeyCodec<K> cd = key_codec<K>(key_type);
	RunsScratch s;
	if (int rc = set_count_scan(c, a, n, b, m, cd, kSetKeepMatchedA, num_groups, s)) return rc;
	if (s.tiles && cap && (keys || a_first || a_count || b_first || b_count)) // (cap == 0, or no output: the count alone)
		LAUNCH(c, (join_write_kernel<K>), (unsigned)s.tiles, kMergeTh, 0, a, n, b, m, cd, s.splits, s.tile_counts, s.piece_sums, num_groups, cap, keys, a_first, a_count, b_first,
		       b_count);
	phase_mark(c, "join_groups");
	phase_end(c);
	return MSD_OK;
}

// The pairs: the scan of the products, the expansion; the scratch -- one 8-byte offset per group of groups_cap, one 8-byte
// sum per scan piece -- is the slab's.  Nothing is read back: the grid of the expansion is that of min(cap, n * m) ranks.
static int join_pairs_impl(msd_ctx *c, uint64_t groups_cap, const uint64_t *num_groups, const uint64_t *a_first, const uint64_t *a_count, const uint64_t *b_first,
			   const uint64_t *b_count, uint64_t n, uint64_t m, const uint64_t *pos_a, const uint64_t *pos_b, uint64_t stored, uint64_t cap, uint64_t *out_a,
			   uint64_t *out_b, uint64_t *num_pairs)
{
	// (runs_count_scan with a word per group in the place of the tile counts: the offsets; join_offsets_kernel scans the pieces itself)
	RunsScratch s;
	if (int rc = runs_count_scan(c, groups_cap, false, num_pairs, nullptr,
				     [&] { return LAUNCH_RC(c, join_offsets_kernel, (unsigned)s.pieces, kRunsScanTh, 0, groups_cap, num_groups, a_count, b_count, s.tile_counts, s.piece_sums); },
				     [](Bump &) {}, s, false))
		return rc;
	uint64_t *const offs = s.tile_counts, *const piece_sums = s.piece_sums;
	const uint64_t grid = s.tiles ? (stored + kJoinPairTile - 1) / kJoinPairTile : 0; // (stored < 2^40: at most 2^29)
	if (grid && (out_a || out_b)) { // (cap == 0, an empty side or no output: the count alone)
		int rc = with_flag(pos_a != nullptr, [&](auto pa) {
			return with_flag(pos_b != nullptr, [&](auto pb) {
				LAUNCH(c, (join_expand_kernel<decltype(pa)::value, decltype(pb)::value>), (unsigned)grid, kJoinPairTh, 0, groups_cap, num_groups, offs, piece_sums, num_pairs, a_first,
				       b_first, b_count, n, m, pos_a, pos_b, cap, out_a, out_b);
				return (int)MSD_OK;
			});
		});
		if (rc) return rc;
	}
	phase_mark(c, "join_pairs");
	phase_end(c);
	return MSD_OK;
}

extern "C" {

int msd_join_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile, uint64_t *pair_tile)
{
	return tile_limits<MergeCfg>(key_bytes, tile, { { scan_tile, kRunsScanTile }, { pair_tile, kJoinPairTile } });
}

int msd_join_groups(msd_ctx *c, const void *d_a, uint64_t n, const void *d_b, uint64_t m, int key_type, uint64_t cap, void *d_keys, uint64_t *d_a_first,
		    uint64_t *d_a_count, uint64_t *d_b_first, uint64_t *d_b_count, uint64_t *d_num_groups)
{
	if (!c) return MSD_EINVAL;
	if (!key_type_ok(key_type)) return fail(c, MSD_EINVAL, "unknown key_type");
	if (!d_num_groups) return fail(c, MSD_EINVAL, "d_num_groups is required");
	if (n && !d_a) return fail(c, MSD_EINVAL, "null d_a pointer");
	if (m && !d_b) return fail(c, MSD_EINVAL, "null d_b pointer");
	// the extents: the inputs, then the outputs; at most min(cap, n, m) groups are stored
	const uint32_t es = (uint32_t)key_type_bytes(key_type);
	const uint64_t stored = std::min(cap, std::min(n, m));
	const Span buf[8] = { span_of(d_a, n, es),           span_of(d_b, m, es),           span_of(d_keys, stored, es),    span_of(d_a_first, stored, 8),
			      span_of(d_a_count, stored, 8), span_of(d_b_first, stored, 8), span_of(d_b_count, stored, 8), span_of(d_num_groups, 1, 8) };
	if (first_misaligned(buf) >= 0)
		return fail(c, MSD_EINVAL, "every buffer must be aligned to its element size (d_a, d_b, d_keys: the key's width; the others: 8)");
	if (n >= kJoinMaxElems || m >= kJoinMaxElems) return fail(c, MSD_EINVAL, "n or m too large: fewer than 2^32 elements each");
	if (outputs_overlap(buf, 2)) return fail(c, MSD_EINVAL, "the outputs and d_num_groups must not overlap an input or each other");
	HIPCHK(c, hipSetDevice(c->device));
	return with_width((int)es, [&](auto k0) {
		typedef decltype(k0) K;
		return join_groups_impl<K>(c, (const K *)d_a, n, (const K *)d_b, m, key_type, cap, (K *)d_keys, d_a_first, d_a_count, d_b_first, d_b_count, d_num_groups);
	});
}

int msd_join_pairs(msd_ctx *c, uint64_t groups_cap, const uint64_t *d_num_groups, const uint64_t *d_a_first, const uint64_t *d_a_count, const uint64_t *d_b_first,
		   const uint64_t *d_b_count, uint64_t n, uint64_t m, const uint64_t *d_pos_a, const uint64_t *d_pos_b, uint64_t cap, uint64_t *d_out_a, uint64_t *d_out_b,
		   uint64_t *d_num_pairs)
{
	if (!c) return MSD_EINVAL;
	if (!d_num_pairs) return fail(c, MSD_EINVAL, "d_num_pairs is required");
	if (groups_cap && !d_num_groups) return fail(c, MSD_EINVAL, "null d_num_groups pointer");
	if (groups_cap && (!d_a_first || !d_a_count || !d_b_first || !d_b_count)) return fail(c, MSD_EINVAL, "null group array (d_a_first, d_a_count, d_b_first, d_b_count)");
	// the extents: the inputs, then the outputs; at most min(cap, n * m) pairs are stored (n * m saturates until n and m are checked)
	uint64_t all = 0;
	if (__builtin_mul_overflow(n, m, &all)) all = UINT64_MAX;
	const uint64_t stored = std::min(cap, all);
	const Span buf[10] = { span_of(d_num_groups, 1, 8),        span_of(d_a_first, groups_cap, 8), span_of(d_a_count, groups_cap, 8), span_of(d_b_first, groups_cap, 8),
			       span_of(d_b_count, groups_cap, 8), span_of(d_pos_a, n, 8),            span_of(d_pos_b, m, 8),            span_of(d_out_a, stored, 8),
			       span_of(d_out_b, stored, 8),        span_of(d_num_pairs, 1, 8) };
	if (first_misaligned(buf) >= 0) return fail(c, MSD_EINVAL, "every buffer must be aligned to 8 bytes");
	if (n >= kJoinMaxElems || m >= kJoinMaxElems) return fail(c, MSD_EINVAL, "n or m too large: fewer than 2^32 elements each");
	if (groups_cap >= kJoinMaxElems) return fail(c, MSD_EINVAL, "groups_cap too large: fewer than 2^32 groups");
	if ((d_out_a || d_out_b) && stored >= kJoinMaxStored) return fail(c, MSD_EINVAL, "cap too large: fewer than 2^40 pairs are stored by one call");
	if (outputs_overlap(buf, 7)) return fail(c, MSD_EINVAL, "d_out_a, d_out_b and d_num_pairs must not overlap an input or each other");
	HIPCHK(c, hipSetDevice(c->device));
	return join_pairs_impl(c, groups_cap, d_num_groups, d_a_first, d_a_count, d_b_first, d_b_count, n, m, d_pos_a, d_pos_b, stored, cap, d_out_a, d_out_b, d_num_pairs);
}

} // extern "C"

template <typename K>
static int check_impl(msd_ctx *c, const K *k, const uint64_t *r, uint64_t n, uint64_t *viol, uint64_t *sum, uint64_t *xr)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	CheckResult *res = nullptr;
	int rc = slab_carve(c, [&](Bump &b) { res = b.take<CheckResult>(1); });
	if (!rc) rc = pinned_reserve(c, 4096);
	if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(res, 0, sizeof *res, c->stream));
	if (n) {
		const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 8, (n + 255) / 256);
		LAUNCH(c, (check_kernel<K>), grid, 256, 0, k, r, n, res);
	}
	CheckResult h;
	if ((rc = read_back(c, res, &h))) return rc;
	if (viol) *viol = h.violations;
	if (sum) *sum = h.sum;
	if (xr) *xr = h.xr;
	return MSD_OK;
}
extern "C" {

int msd_check_u32(msd_ctx *c, const uint32_t *k, uint64_t n, uint64_t *v, uint64_t *s, uint64_t *x) { return check_impl<uint32_t>(c, k, nullptr, n, v, s, x); }
int msd_check_u64(msd_ctx *c, const uint64_t *k, const uint64_t *r, uint64_t n, uint64_t *v, uint64_t *s, uint64_t *x) { return check_impl<uint64_t>(c, k, r, n, v, s, x); }

static unsigned gen_grid(const msd_ctx *c, uint64_t n) { return (unsigned)std::min<uint64_t>((uint64_t)c->sm_count * 16, (n + 255) / 256 + 1); }

int msd_gen_uniform_u32(msd_ctx *c, uint32_t *k, uint64_t n, uint64_t seed, uint64_t first)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, gen_uniform_u32_kernel, gen_grid(c, n), 256, 0, k, n, seed + first);
	return MSD_OK;
}
int msd_gen_uniform_u64(msd_ctx *c, uint64_t *k, uint64_t n, uint64_t seed, uint64_t first, int shr)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, gen_uniform_u64_kernel, gen_grid(c, n), 256, 0, k, n, seed + first, shr);
	return MSD_OK;
}
int msd_gen_zipf_u32(msd_ctx *c, uint32_t *k, uint64_t n, uint64_t seed, uint64_t first)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, gen_zipf_u32_kernel, gen_grid(c, n), 256, 0, k, n, seed + first);
	return MSD_OK;
}
int msd_gen_dup_u32(msd_ctx *c, uint32_t *k, uint64_t n, uint64_t seed, uint64_t first, uint64_t distinct)
{
	if (!c) return MSD_EINVAL;
	if (distinct == 0) return fail(c, MSD_EINVAL, "gen_dup: distinct must be positive");
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, gen_dup_u32_kernel, gen_grid(c, n), 256, 0, k, n, seed + first, distinct);
	return MSD_OK;
}
int msd_gen_mt19937_64(msd_ctx *c, uint64_t *k, uint64_t n, uint64_t seed, int shr)
{
	if (!c) return MSD_EINVAL;
	if (shr < 0 || shr > 63) return fail(c, MSD_EINVAL, "gen_mt19937_64: shift_right must be 0..63");
	HIPCHK(c, hipSetDevice(c->device));
	if (n == 0) return MSD_OK;
	LAUNCH(c, gen_mt19937_64_kernel, 1, 320, 0, k, n, seed, shr);
	return MSD_OK;
}
int msd_gen_iota_u64(msd_ctx *c, uint64_t *v, uint64_t n, uint64_t first)
{
	if (!c) return MSD_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	LAUNCH(c, gen_iota_u64_kernel, gen_grid(c, n), 256, 0, v, n, first);
	return MSD_OK;
}

} // extern "C"

template <typename K, typename V>
static int plan_describe(uint64_t n, int end_bit, int cus, msd_plan *out)
{
	using C = Cfg<K, V>;
	constexpr bool HV = has_val<V>::value;
	const uint64_t small_max = (uint64_t)C::SORT_TH * C::SORT_KPT;
	const uint32_t count_bits = HV ? (uint32_t)kLeafCountBits : (uint32_t)kCountMaxBits;
	memset(out, 0, sizeof *out);
	out->block_elems = C::B;
	out->tile_elems = C::T;
	out->leaf_capacity = small_max;
	out->leaf_count_bits = count_bits;
	if (n <= small_max || end_bit <= 0) return MSD_OK; // a single LDS leaf
	std::vector<Segment> segs(1);
	segs[0] = { 0, n, (uint32_t)end_bit, 0 };
	RoundPlan rp;
	plan_round<K, V>(segs, small_max, cus, rp, count_bits);
	out->digit_width = rp.parents[0].width;
	out->digit_shift = rp.parents[0].shift;
	out->stripes = rp.stripes.size();
	out->stripe_elems = rp.stripes[0].end - rp.stripes[0].begin;
	// uniform keys: every round divides the segment size by 2^width
	uint64_t sz = n;
	uint32_t bits = (uint32_t)end_bit, rounds = 0;
	while (sz > small_max && bits > 0) {
		const uint32_t w = pick_width(sz, bits, small_max, count_bits);
		sz >>= w;
		bits -= w;
		++rounds;
	}
	out->expected_rounds = rounds;
	out->workspace_bytes = round_bytes_estimate<K, V>(n, cus) + keep_bytes_for<K, V>(n) + 4 * leaf_list_guess<K, V>(n) * sizeof(Segment);
	return MSD_OK;
}

extern "C" {

int msd_plan_first_round(uint64_t n, int key_bytes, int val_bytes, int end_bit, int cus, msd_plan *out)
{
	if (!out || cus <= 0 || end_bit < 0 || end_bit > key_bytes * 8) return MSD_EINVAL;
	const int rc = with_layout(key_bytes, val_bytes, [&](auto k, auto v) { return plan_describe<decltype(k), decltype(v)>(n, end_bit, cus, out); });
	return rc != kNoLayout ? rc : MSD_EINVAL;
}

int msd_set_option(msd_ctx *c, const char *name, int64_t value)
{
	if (!c || !name) return MSD_EINVAL;
	const char *refusal = nullptr;
	if (options_set(c->opt, name, value, &refusal)) return MSD_OK;
	return refusal ? fail(c, MSD_EINVAL, "%s", refusal) : fail(c, MSD_EINVAL, "unknown option %s", name);
}

#ifdef MSD_STAMPS
// diagnostic build only: per-section shader cycles of classify_direct_kernel, [wave 0 | last wave][section]; resets them
int msd_debug_stamps(uint64_t *out)
{
	unsigned long long h[2][16];
	if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stamps), sizeof h) != hipSuccess) return MSD_EHIP;
	memcpy(out, h, sizeof h);
	memset(h, 0, sizeof h);
	if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), h, sizeof h) != hipSuccess) return MSD_EHIP;
	return MSD_OK;
}
#endif

int msd_set_profiling(msd_ctx *c, int on)
{
	if (!c) return MSD_EINVAL;
	c->profiling = on != 0;
	return MSD_OK;
}
int msd_phase_count(const msd_ctx *c) { return c ? (int)c->phase_us.size() : 0; }
const char *msd_phase_name(const msd_ctx *c, int i) { return (c && i >= 0 && i < (int)c->phase_us.size()) ? c->phase_us[i].first.c_str() : ""; }
double msd_phase_us(const msd_ctx *c, int i) { return (c && i >= 0 && i < (int)c->phase_us.size()) ? c->phase_us[i].second : 0.0; }
int msd_stat(const msd_ctx *c, const char *name, uint64_t *v)
{
	if (!c || !name || !v) return MSD_EINVAL;
	// the typed sort's two counters live in device words: these two names wait for the context's stream
	const int slot = stat_by_name(name);
	const int fix_word = slot == kStatSortKeysSplit ? kFixSplit : slot == kStatSortKeysReversed ? kFixReversed : -1;
	if (fix_word >= 0) {
		if (c->fix_stats == 0) return MSD_EINVAL;
		*v = fix_word == kFixSplit ? c->fix_split : 0;
		if (c->fix_stats == 1) return MSD_OK;
		if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
		    hipMemcpy(v, c->fix_plan + fix_word, sizeof *v, hipMemcpyDeviceToHost) != hipSuccess)
			return MSD_EHIP;
		return MSD_OK;
	}
	if (slot == kStatCount || !(c->stat_written >> slot & 1)) return MSD_EINVAL;
	*v = c->stat[slot];
	return MSD_OK;
}

} // extern "C"

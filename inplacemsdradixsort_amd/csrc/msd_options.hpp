// msd_options.hpp -- the tables of the context of msd_radix.hip: the options of msd_set_option and the counters of
// msd_stat, each stated once.  Host only, like msd_args.hpp: plain C++17 without a HIP header and
// without msd_ctx, so that a host compiler takes it alone (tests/options_main.cpp prints both tables and tries every rule).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace msd {

// ---- the rules an option's value is held to, and what a refusal says behind the option's name
enum OptionRule { kRule_mode3, kRule_positive, kRule_boolean, kRule_lanes, kRule_cap28, kRule_at_least_1 };
#define MSD_SAYS_mode3 "must be 0, 1 or 2"
#define MSD_SAYS_positive "must be positive"
#define MSD_SAYS_boolean "is 0 or not" // (never said: every value is taken, as value != 0)
#define MSD_SAYS_lanes "must be 0, 64, 256 or 1024"
#define MSD_SAYS_cap28 "must be 1 .. 2^28 elements"
#define MSD_SAYS_at_least_1 "must be at least 1"

inline bool option_rule_holds(OptionRule rule, int64_t v)
{
	switch (rule) {
	case kRule_mode3: return v >= 0 && v <= 2;
	case kRule_positive: return v >= 1;
	case kRule_boolean: return true;
	case kRule_lanes: return v == 0 || v == 64 || v == 256 || v == 1024;
	case kRule_cap28: return v >= 1 && v <= ((int64_t)1 << 28);
	case kRule_at_least_1: return v >= 1;
	}
	return false;
}

// ---- the options: X(name, type, default, rule, environment variable read by msd_create or nullptr)
//   direct_mode         direct block placement in the first round: 0 off, 1 when the sampled children are
//                       about equally big, 2 whenever the geometry allows (tests)
//   direct_min          smallest round (elements) it is tried on (tools/size_sweep.py: from 2^22 on it is never slower by more
//                       than 7 %, and up to 47 % faster)
//   direct_min_parent   rounds after the first: smallest parent
//   regpart             u64 keys / tuples: rounds of small parents as one register-resident pass (0: A/B comparisons)
//   count16             u32 keys: count_place16_kernel in front of count_place_kernel (0: A/B comparisons)
//   leaf17              u64 keys and tuples: segments of <= 17408 elements are finished by leaf17_kernel (0: tuples: register
//                       partition + small leaves, keys: leaf_count_sort_kernel; A/B comparisons)
//   mid_leaf            u32 keys: merge_count_kernel (list mode) in front of count_walk_kernel (0: A/B comparisons)
//   early_leaves        keys only: the counting leaves go behind a last round without waiting for its end (0: A/B comparisons)
//   early_plan          a round that is not the last: the next round is planned and enqueued while its fix-up runs (0: A/B
//                       comparisons)
//   front_count         u32 keys, two direct 8-bit rounds: the top 16 bits are counted once up front and both rounds placed
//                       from that (msd_front16.hpp; 0: A/B comparisons)
//   front_min           smallest sort the front pass is tried on (tools/size_sweep.py: 0.7 % slower at 2^28 keys, 1 % faster at
//                       2^29, 1.5 % at 2^30)
//   merge_leaf          msd_merge_buckets_u32: 0 = by bucket size, 1 = merge_place16_kernel, 2 = merge_count_kernel (tests)
//   select_cap          msd_topk_* / msd_select_*: candidate capacity (elements): the search stops once the pivot bucket fits
//   topk_rows_mode      msd_topk_rows: 0 = the library chooses, 1 = always the loop over msd_topk_keys, 2 = always the row kernel
//   topk_rows_lanes     the row kernel's lanes per row: 0 = by row length, 64 / 256 / 1024 = forced where the row fits (A/B
//                       comparisons)
//   sort_rows_mode      msd_sort_rows: 0 = the library chooses, 1 = always the segment path, 2 = always the row kernel
//   sort_rows_lanes     the row kernel's lanes per row: 0 = by row length, 64 / 256 / 1024 = forced where the row fits (A/B
//                       comparisons)
//   search_mode         msd_search_sorted with sorted needles: 0 = the library chooses, 1 = always direct, 2 = always merge
//   search_merge_ratio  R: the library chooses merge when m >= n / R (the measured crossover lies near n / 37 for 4-byte and
//                       n / 24 for 8-byte keys: DESIGN.md section 10.7)
#define MSD_OPTIONS(X)                                                     \
	X(direct_mode, int, 1, mode3, "MSD_DIRECT")                        \
	X(direct_min, uint64_t, 1ull << 22, positive, nullptr)             \
	X(direct_min_parent, uint64_t, 1ull << 17, positive, nullptr)      \
	X(regpart, int, 1, boolean, "MSD_REGPART")                         \
	X(count16, int, 1, mode3, "MSD_COUNT16")                           \
	X(leaf17, int, 1, boolean, nullptr)                                \
	X(mid_leaf, int, 1, boolean, nullptr)                              \
	X(early_leaves, int, 1, boolean, nullptr)                          \
	X(early_plan, int, 1, boolean, nullptr)                            \
	X(front_count, int, 1, boolean, nullptr)                           \
	X(front_min, uint64_t, 1ull << 29, positive, nullptr)              \
	X(merge_leaf, int, 0, mode3, nullptr)                              \
	X(select_cap, uint64_t, 1ull << 20, cap28, nullptr)                \
	X(topk_rows_mode, int, 0, mode3, nullptr)                          \
	X(topk_rows_lanes, int, 0, lanes, nullptr)                         \
	X(sort_rows_mode, int, 0, mode3, nullptr)                          \
	X(sort_rows_lanes, int, 0, lanes, nullptr)                         \
	X(search_mode, int, 0, mode3, nullptr)                             \
	X(search_merge_ratio, uint64_t, 32, at_least_1, nullptr)

struct Options {
#define X(name, type, dflt, rule, env) type name = dflt;
	MSD_OPTIONS(X)
#undef X
};

struct OptionEntry {
	const char *name;
	uint64_t dflt;
	OptionRule rule;
	const char *refusal; // what msd_last_error says of a value the rule does not hold for
	const char *env;     // msd_create sets the option from this variable (nullptr: from none)
	void (*put)(Options &, int64_t);
};

inline constexpr OptionEntry kOptions[] = {
#define X(name, type, dflt, rule, env) { #name, dflt, kRule_##rule, #name " " MSD_SAYS_##rule, env, [](Options &o, int64_t v) { o.name = (type)v; } },
	MSD_OPTIONS(X)
#undef X
};

// Sets the named option.  True: done.  False: nothing has changed, and *message is the entry's refusal, or nullptr for a
// name that the table does not have.
inline bool options_set(Options &o, const char *name, int64_t value, const char **message)
{
	*message = nullptr;
	for (const OptionEntry &e : kOptions) {
		if (strcmp(name, e.name)) continue;
		if (!option_rule_holds(e.rule, value)) {
			*message = e.refusal;
			return false;
		}
		e.put(o, e.rule == kRule_boolean ? value != 0 : value);
		return true;
	}
	return false;
}

// ---- the counters of msd_stat: X(enumerator suffix, name).  A call clears them all and writes the ones it has something to
// say about; msd_stat knows a name only once it has been written.  (The last two are not slots of the context: the typed
// sort leaves them in device words, and msd_stat fetches them from there.)
#define MSD_STATS(X)                                                      \
	X(Rounds, "rounds")                                               \
	X(Parents, "parents")                                             \
	X(Stripes, "stripes")                                             \
	X(Children, "children")                                           \
	X(Slots, "slots")                                                 \
	X(Holes, "holes")                                                 \
	X(ChainSteps, "chain_steps")                                      \
	X(SmallSegments, "small_segments")                                \
	X(CountSegments, "count_segments")                                \
	X(BigCountSegments, "big_count_segments")                         \
	X(DirectRounds, "direct_rounds")                                  \
	X(RegpartRounds, "regpart_rounds")                                \
	X(SkippedBits, "skipped_bits")                                    \
	X(BitSkipRestarts, "bit_skip_restarts")                           \
	X(BitSkipCheckedByHistogram, "bit_skip_checked_by_histogram")     \
	X(LeavesBehindRound, "leaves_behind_round")                       \
	X(RoundsPlannedEarly, "rounds_planned_early")                     \
	X(FrontCountSorts, "front_count_sorts")                           \
	X(FrontCountDeclined, "front_count_declined")                     \
	X(ExcessBlocks, "excess_blocks")                                  \
	X(ChildScanSplitRounds, "child_scan_split_rounds")                \
	X(Count16Rejected, "count16_rejected")                            \
	X(CountSlowSegments, "count_slow_segments")                       \
	X(MergeRejected, "merge_rejected")                                \
	X(Leaf17Segments, "leaf17_segments")                              \
	X(Leaf17Rejected, "leaf17_rejected")                              \
	X(Leaf17SlowSegments, "leaf17_slow_segments")                     \
	X(Leaf17Launches, "leaf17_launches")                              \
	X(WorkspaceBytes, "workspace_bytes")                              \
	X(SelectHistPasses, "select_hist_passes")                         \
	X(SelectSkippedBits, "select_skipped_bits")                       \
	X(SelectCandidates, "select_candidates")                          \
	X(SelectBelow, "select_below")                                    \
	X(TopkRowsKernelRows, "topk_rows_kernel_rows")                    \
	X(TopkRowsLoopedRows, "topk_rows_looped_rows")                    \
	X(SortRowsKernelRows, "sort_rows_kernel_rows")                    \
	X(SortRowsSegmentRows, "sort_rows_segment_rows")                  \
	X(SortRowsLanes, "sort_rows_lanes")                               \
	X(SortKeysSplit, "sort_keys_split")                               \
	X(SortKeysReversed, "sort_keys_reversed")

enum Stat {
#define X(id, name) kStat##id,
	MSD_STATS(X)
#undef X
	kStatCount
};

inline constexpr const char *kStatNames[kStatCount] = {
#define X(id, name) name,
	MSD_STATS(X)
#undef X
};
static_assert(kStatCount <= 64, "the context marks the written slots in one 64-bit word");

// the slot of a name, or kStatCount
inline int stat_by_name(const char *name)
{
	for (int i = 0; i < kStatCount; ++i)
		if (!strcmp(name, kStatNames[i])) return i;
	return kStatCount;
}

} // namespace msd

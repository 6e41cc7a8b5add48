// The tables of csrc/msd_options.hpp on a host compiler, without a GPU: tests/test_option_defaults.py builds and runs this.
// Every option meets every probe value; what is taken, what is stored and what a refusal says are written out below, not
// computed from the table.  Prints "option <name> <default>" per option and "stat <name>" per counter.  Exit status 0:
// everything holds; otherwise the failed lines are printed.
#include "../inplacemsdradixsort_amd/csrc/msd_options.hpp"

#include <cstdio>

using namespace msd;

static int failures = 0;
#define CHECK(cond)                                                          \
	do {                                                                 \
		if (!(cond)) {                                               \
			printf("line %d: %s\n", __LINE__, #cond);            \
			++failures;                                          \
		}                                                            \
	} while (0)

static const int64_t kProbes[13] = { -1, 0, 1, 2, 3, 63, 64, 65, 256, 1024, (int64_t)1 << 28, ((int64_t)1 << 28) + 1, (int64_t)1 << 40 };
// which of the probes a rule takes, in the order above
#define TAKES_0_1_2 "0111000000000"
#define TAKES_FROM_1 "0011111111111"
#define TAKES_ALL "1111111111111"
#define TAKES_LANES "0100001011000"
#define TAKES_1_TO_2_28 "0011111111100"

struct Expect {
	const char *name;
	const char *takes;
	bool boolean; // stored as value != 0
	const char *refusal;
	uint64_t (*get)(const Options &);
};
#define GET(member) [](const Options &o) -> uint64_t { return (uint64_t)o.member; }
static const Expect kExpect[] = {
	{ "direct_mode", TAKES_0_1_2, false, "direct_mode must be 0, 1 or 2", GET(direct_mode) },
	{ "direct_min", TAKES_FROM_1, false, "direct_min must be positive", GET(direct_min) },
	{ "direct_min_parent", TAKES_FROM_1, false, "direct_min_parent must be positive", GET(direct_min_parent) },
	{ "regpart", TAKES_ALL, true, nullptr, GET(regpart) },
	{ "count16", TAKES_0_1_2, false, "count16 must be 0, 1 or 2", GET(count16) },
	{ "leaf17", TAKES_ALL, true, nullptr, GET(leaf17) },
	{ "mid_leaf", TAKES_ALL, true, nullptr, GET(mid_leaf) },
	{ "early_leaves", TAKES_ALL, true, nullptr, GET(early_leaves) },
	{ "early_plan", TAKES_ALL, true, nullptr, GET(early_plan) },
	{ "front_count", TAKES_ALL, true, nullptr, GET(front_count) },
	{ "front_min", TAKES_FROM_1, false, "front_min must be positive", GET(front_min) },
	{ "merge_leaf", TAKES_0_1_2, false, "merge_leaf must be 0, 1 or 2", GET(merge_leaf) },
	{ "select_cap", TAKES_1_TO_2_28, false, "select_cap must be 1 .. 2^28 elements", GET(select_cap) },
	{ "topk_rows_mode", TAKES_0_1_2, false, "topk_rows_mode must be 0, 1 or 2", GET(topk_rows_mode) },
	{ "topk_rows_lanes", TAKES_LANES, false, "topk_rows_lanes must be 0, 64, 256 or 1024", GET(topk_rows_lanes) },
	{ "sort_rows_mode", TAKES_0_1_2, false, "sort_rows_mode must be 0, 1 or 2", GET(sort_rows_mode) },
	{ "sort_rows_lanes", TAKES_LANES, false, "sort_rows_lanes must be 0, 64, 256 or 1024", GET(sort_rows_lanes) },
	{ "search_mode", TAKES_0_1_2, false, "search_mode must be 0, 1 or 2", GET(search_mode) },
	{ "search_merge_ratio", TAKES_FROM_1, false, "search_merge_ratio must be at least 1", GET(search_merge_ratio) },
};

static void every_option_meets_every_probe()
{
	CHECK(sizeof kExpect / sizeof kExpect[0] == sizeof kOptions / sizeof kOptions[0]); // (nothing in the table goes untried)
	for (const Expect &e : kExpect) {
		Options o;
		for (int i = 0; i < 13; ++i) {
			const uint64_t before = e.get(o);
			const char *message = "untouched";
			const bool taken = options_set(o, e.name, kProbes[i], &message);
			const bool as_expected = taken == (e.takes[i] == '1') &&
						 (taken ? message == nullptr && e.get(o) == (e.boolean ? (uint64_t)(kProbes[i] != 0) : (uint64_t)kProbes[i])
							: message && e.refusal && !strcmp(message, e.refusal) && e.get(o) == before);
			if (!as_expected) {
				printf("%s = %lld: taken %d, message %s, now %llu\n", e.name, (long long)kProbes[i], (int)taken, message ? message : "(none)",
				       (unsigned long long)e.get(o));
				++failures;
			}
		}
	}
}

static void an_unknown_name_has_no_message_and_changes_nothing()
{
	Options o;
	const char *message = "untouched";
	CHECK(!options_set(o, "no_such_option", 1, &message) && message == nullptr);
	CHECK(!options_set(o, "", 1, &message) && message == nullptr);
	CHECK(!options_set(o, "direct_mod", 1, &message) && message == nullptr); // (a prefix of a name is no name)
	for (const Expect &e : kExpect) CHECK(e.get(o) == e.get(Options()));
}

static void the_environment_sets_three_options()
{
	int with_env = 0;
	for (const OptionEntry &e : kOptions) {
		if (!e.env) continue;
		++with_env;
		CHECK((!strcmp(e.name, "direct_mode") && !strcmp(e.env, "MSD_DIRECT")) || (!strcmp(e.name, "regpart") && !strcmp(e.env, "MSD_REGPART")) ||
		      (!strcmp(e.name, "count16") && !strcmp(e.env, "MSD_COUNT16")));
	}
	CHECK(with_env == 3);
}

static void stats_are_found_by_name()
{
	for (int i = 0; i < kStatCount; ++i) CHECK(stat_by_name(kStatNames[i]) == i);
	CHECK(stat_by_name("round") == kStatCount && stat_by_name("roundss") == kStatCount && stat_by_name("") == kStatCount);
	CHECK(stat_by_name("rounds") == kStatRounds && stat_by_name("sort_keys_reversed") == kStatSortKeysReversed);
}

int main()
{
	every_option_meets_every_probe();
	an_unknown_name_has_no_message_and_changes_nothing();
	the_environment_sets_three_options();
	stats_are_found_by_name();
	const Options defaults;
	for (const OptionEntry &e : kOptions) {
		printf("option %s %llu\n", e.name, (unsigned long long)e.dflt);
		for (const Expect &x : kExpect) // (the struct's initialiser and the entry's default are one token of the table: so they agree)
			if (!strcmp(x.name, e.name)) CHECK(x.get(defaults) == e.dflt);
	}
	for (const char *name : kStatNames) printf("stat %s\n", name);
	return failures ? 1 : 0;
}

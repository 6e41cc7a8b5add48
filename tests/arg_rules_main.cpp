// The argument rules of csrc/msd_args.hpp on a host compiler, without a GPU: tests/test_arg_rules.py builds and runs this.
// Addresses are numbers that are never dereferenced.  Exit status 0: every rule holds; otherwise the failed lines are printed.
#include "../inplacemsdradixsort_amd/csrc/msd_args.hpp"

#include <cstdio>
#include <initializer_list>

using namespace msd;

static int failures = 0;
#define CHECK(cond)                                                          \
	do {                                                                 \
		if (!(cond)) {                                               \
			printf("line %d: %s\n", __LINE__, #cond);            \
			++failures;                                          \
		}                                                            \
	} while (0)

static const void *at(uint64_t address) { return (const void *)(uintptr_t)address; }

static void overlap_of_two_ranges()
{
	CHECK(ranges_overlap(at(1000), 100, at(1099), 50));  // one byte shared
	CHECK(ranges_overlap(at(1099), 50, at(1000), 100));
	CHECK(!ranges_overlap(at(1000), 100, at(1100), 50)); // exactly adjacent, on either side
	CHECK(!ranges_overlap(at(1100), 50, at(1000), 100));
	CHECK(!ranges_overlap(at(1000), 100, at(900), 100));
	CHECK(ranges_overlap(at(1000), 100, at(1050), 0));   // an empty range strictly inside
	CHECK(ranges_overlap(at(1050), 0, at(1000), 100));
	CHECK(!ranges_overlap(at(1000), 100, at(1000), 0));  // an empty range at either end
	CHECK(!ranges_overlap(at(1000), 100, at(1100), 0));
	CHECK(!ranges_overlap(at(1000), 0, at(1000), 100));
	CHECK(!ranges_overlap(at(1100), 0, at(1000), 100));
	CHECK(!ranges_overlap(nullptr, 0, at(1000), 100));   // null with 0 bytes against anything
	CHECK(!ranges_overlap(at(1000), 100, nullptr, 0));
	CHECK(!ranges_overlap(nullptr, 0, at(0), 100));
	CHECK(!ranges_overlap(nullptr, 0, at(0), UINT64_MAX));
	CHECK(!ranges_overlap(nullptr, 0, nullptr, 0));
}

// the table of msd_run_encode: data, positions | values, starts, inverse, num_runs
struct RunEncode {
	uint64_t data, positions, values, starts, inverse, num;
	bool refused(uint64_t n, uint32_t es) const
	{
		const Span buf[6] = { span_of(at(data), n, es),         span_of(at(positions), n, 8), span_of(at(values), n, es),
				      span_of(at(starts), n + 1, 8),    span_of(at(inverse), n, 8),   span_of(at(num), 1, 8) };
		return outputs_overlap(buf, 2);
	}
};

static void outputs_against_spans()
{
	const uint64_t n = 1000;
	for (const uint32_t es : { 4u, 8u }) {
		const uint64_t w = 8 / es; // elements of the input per word
		const RunEncode good = { 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000 };
		CHECK(!good.refused(n, es));
		RunEncode k;
		// every output against the input, the positions and the other outputs (tests/test_gpu_runs.py, test_refusals_touch_nothing)
#define REFUSED(field, value)             \
	do {                              \
		k = good;                 \
		k.field = (value);        \
		CHECK(k.refused(n, es));  \
	} while (0)
		REFUSED(values, good.data);
		REFUSED(values, good.data + (n - 1) * es);
		REFUSED(starts, good.data + 8 * (n / 2 / w));
		REFUSED(inverse, good.data + 8 * (n / w - 1));
		REFUSED(num, good.data);
		REFUSED(num, good.data + (n * es - 8));
		REFUSED(values, good.positions);
		REFUSED(starts, good.positions + 8 * (n - 1));
		REFUSED(inverse, good.positions);
		REFUSED(num, good.positions + 8);
		REFUSED(values, good.starts + 8 * n); // the last word of the starts
		REFUSED(values, good.inverse);
		REFUSED(starts, good.inverse + 8 * (n - 1));
		REFUSED(num, good.values);
		REFUSED(num, good.starts + 8 * n);
		REFUSED(num, good.inverse + 8 * 5);
		k = good, k.inverse = good.starts, k.positions = 0;
		CHECK(k.refused(n, es));
#undef REFUSED
		// buffers that touch without sharing a byte
		k = good, k.values = good.data + n * es;
		CHECK(!k.refused(n, es));
		k = good, k.num = good.starts + 8 * (n + 1);
		CHECK(!k.refused(n, es));
		// two inputs that overlap each other are not the rule's business
		k = good, k.positions = good.data;
		CHECK(!k.refused(n, es));
		// an absent optional buffer never is, wherever the others lie
		k = good, k.positions = 0, k.values = 0, k.starts = 0, k.inverse = 0;
		CHECK(!k.refused(n, es));
		k = good, k.data = 0, k.positions = 0; // (data at address 0 .. n * es: a null input is empty, too)
		CHECK(!k.refused(n, es));
	}
	const Span absent = span_of(nullptr, 1000, 8);
	CHECK(absent.bytes == 0 && absent.align == 8);
	CHECK(span_of(at(64), 3, 4).bytes == 12 && span_of(at(64), 3, 4, 16).align == 16);
	CHECK(span_of(at(64), UINT64_MAX, 8).bytes == UINT64_MAX); // (saturates: no byte count wraps)
}

static void alignment()
{
	CHECK(aligned16(nullptr) && aligned16(at(4096)) && !aligned16(at(4096 + 8)) && !aligned16(at(4097)));
	const uint64_t a = 0x1000, b = 0x2000, c = 0x3000;
	for (const uint64_t d : { 1, 2, 3 }) {
		const Span s[3] = { span_of(at(a), 10, 4), span_of(at(b + d), 10, 4), span_of(at(c), 10, 8) };
		CHECK(first_misaligned(s) == 1);
	}
	for (const uint64_t d : { 1, 2, 4, 7 }) {
		const Span s[3] = { span_of(at(a), 10, 4), span_of(at(b), 10, 4), span_of(at(c + d), 10, 8) };
		CHECK(first_misaligned(s) == 2);
	}
	const Span fine[3] = { span_of(at(a + 4), 10, 4), span_of(nullptr, 10, 8), span_of(at(c + 8), 10, 8) };
	CHECK(first_misaligned(fine) == -1); // null is aligned
	const Span two[3] = { span_of(at(a), 10, 4), span_of(at(b + 2), 10, 4), span_of(at(c + 4), 10, 8) };
	CHECK(first_misaligned(two) == 1);   // the first one is the one returned
	const Span strict[2] = { span_of(at(a + 8), 10, 8, 16), span_of(at(b), 10, 8, 16) };
	CHECK(first_misaligned(strict) == 0);
}

static void rows_geometry()
{
	RowsExtents e = rows_extents(3, 65, 80, 5, 4, true);
	CHECK(e.overflow == kRowsFit && e.in_bytes == (2 * 80 + 65) * 4 && e.out_elems == 15 && e.out_bytes == 60 && e.idx_bytes == 120);
	e = rows_extents(3, 65, 80, 5, 8, false);
	CHECK(e.overflow == kRowsFit && e.in_bytes == (2 * 80 + 65) * 8 && e.out_bytes == 120 && e.idx_bytes == 0);
	e = rows_extents(0, 65, 80, 5, 4, true);
	CHECK(e.overflow == kRowsFit && e.in_bytes == 0 && e.out_bytes == 0 && e.idx_bytes == 0);
	e = rows_extents((uint64_t)1 << 33, 65, (uint64_t)1 << 31, 5, 8, true); // rows * row_stride fits, its bytes do not
	CHECK(e.overflow == kRowsInputOverflows);
	e = rows_extents((uint64_t)1 << 40, 65, (uint64_t)1 << 40, 5, 4, true);
	CHECK(e.overflow == kRowsInputOverflows);
	e = rows_extents((uint64_t)1 << 40, (uint64_t)1 << 21, (uint64_t)1 << 21, (uint64_t)1 << 22, 4, true); // 2^62 outputs: times 8 overflows
	CHECK(e.overflow == kRowsOutputOverflows);
	e = rows_extents((uint64_t)1 << 40, (uint64_t)1 << 21, (uint64_t)1 << 21, (uint64_t)1 << 22, 4, false); // ... with or without positions
	CHECK(e.overflow == kRowsOutputOverflows);
}

static void dispatch()
{
	size_t size = 0;
	int calls = 0;
	const auto width = [&](auto k0) { return ++calls, size = sizeof k0, 0; };
	CHECK(with_width(4, width) == 0 && size == 4 && calls == 1);
	CHECK(with_width(8, width) == 0 && size == 8 && calls == 2);
	for (const int bad : { 0, 2, 16, -4 }) CHECK(with_width(bad, width) == kNoWidth);
	CHECK(calls == 2);
	CHECK(with_flag(true, [](auto f) { return decltype(f)::value ? 10 : 20; }) == 10);
	CHECK(with_flag(false, [](auto f) { return decltype(f)::value ? 10 : 20; }) == 20);
	const auto lanes = [](auto l) { return (int)decltype(l)::value; };
	CHECK(with_lanes(64, lanes) == 64 && with_lanes(256, lanes) == 256 && with_lanes(1024, lanes) == 1024);
	CHECK(kMaxElems == (uint64_t)1 << 36);
}

int main()
{
	overlap_of_two_ranges();
	outputs_against_spans();
	alignment();
	rows_geometry();
	dispatch();
	if (failures) printf("%d rule(s) broken\n", failures);
	return failures ? 1 : 0;
}

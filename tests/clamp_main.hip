// The clamps of the merge path's index functions on the host, without a GPU: tests/test_clamps_host.py builds this with the
// host's address and undefined-behaviour sanitizers and runs it.  The functions are the kernels' own (__host__ __device__ in
// csrc/msd_search.hpp and csrc/msd_join.hpp); nothing is launched.  Every array is a heap block of exactly its length, so a
// probe outside it is a sanitizer report.  The inputs are NOT ascending: what is checked is that every extent and every result
// stays inside its array whatever they hold, and that for ascending inputs the clamps change nothing.
// Exit status 0: every check holds; otherwise the first failed lines are printed.
#include "../inplacemsdradixsort_amd/csrc/msd_join.hpp"
#include "../inplacemsdradixsort_amd/csrc/msd_search.hpp"

#include <cstdio>
#include <memory>
#include <vector>

using namespace msd;

static long failures = 0, checks = 0;
#define CHECK(cond)                                                                        \
	do {                                                                               \
		++checks;                                                                  \
		if (!(cond)) {                                                             \
			if (failures < 20) printf("line %d: %s\n", __LINE__, #cond);       \
			++failures;                                                        \
		}                                                                          \
	} while (0)

static uint64_t min64(uint64_t x, uint64_t y) { return x < y ? x : y; }

// a heap block of exactly `len` elements (len == 0: one byte nobody may read as an element)
template <typename T> static std::unique_ptr<T[]> block(const std::vector<T> &x)
{
	std::unique_ptr<T[]> p(new T[x.size()]);
	for (size_t i = 0; i < x.size(); ++i) p[i] = x[i];
	return p;
}

// ---- merge_tile_extent: every split vector the split kernel can write for n and m, ascending or not
template <uint32_t TILE> static void extents_of(uint64_t n, uint64_t m)
{
	const uint64_t total = n + m, tiles = (total + TILE - 1) / TILE;
	std::vector<uint64_t> lo(tiles + 1), hi(tiles + 1), s(tiles + 1);
	for (uint64_t i = 0; i <= tiles; ++i) {
		const uint64_t d = min64(i * TILE, total);
		lo[i] = d - min64(d, m); // the range of search_split_kernel's result
		hi[i] = min64(d, n);
		s[i] = lo[i];
	}
	for (;;) {
		const std::unique_ptr<uint64_t[]> splits = block(s);
		bool ascending = true;
		for (uint64_t i = 0; i < tiles; ++i) {
			const uint64_t d0 = min64(i * TILE, total), d1 = min64((i + 1) * TILE, total);
			ascending = ascending && s[i] <= s[i + 1] && d0 - s[i] <= d1 - s[i + 1];
		}
		for (uint64_t i = 0; i < tiles; ++i) {
			const MergeTileExtent t = merge_tile_extent<TILE>(i, n, m, splits.get());
			CHECK(t.d0 == min64(i * TILE, total) && t.d1 == min64((i + 1) * TILE, total));
			CHECK(t.a0 == s[i] && t.b0 == t.d0 - s[i]);
			CHECK(t.a0 + t.na <= n);
			CHECK(t.b0 + t.nb <= m);
			CHECK((uint64_t)t.na + t.nb <= TILE);
			const uint64_t sum = (uint64_t)t.na + t.nb, slice = t.d1 - t.d0;
			const uint64_t cnt = sum < slice ? sum : slice; // merge_tile_kernel's cnt
			CHECK(t.d0 + cnt <= total);
			const uint64_t a1 = s[i + 1], b1 = t.d1 - a1;
			const bool nb_clipped = b1 > t.b0 && b1 - t.b0 > TILE - t.na; // the clip of nb by TILE - na binds ...
			if (nb_clipped) CHECK(t.na == 0);                      // ... only where the a side descends or stands still
			CHECK(cnt == slice);                                   // a descending side makes the other over-long: never less than the slice
			if (cnt > 0) CHECK((int64_t)sum - 1 >= 0);             // last, of merge_tile_kernel and set_write_kernel
			if (t.nb > 0) CHECK(t.b0 + t.nb - 1 < m);              // search_tile_kernel's last store
			if (t.na > 0) CHECK(t.a0 + t.na - 1 < n);              // join_write_kernel's e <= na - 1
			if (ascending) CHECK(sum == slice && t.a0 + t.na == s[i + 1] && t.b0 + t.nb == t.d1 - s[i + 1]);
		}
		uint64_t k = 0; // the next vector
		while (k <= tiles && s[k] == hi[k]) {
			s[k] = lo[k];
			++k;
		}
		if (k > tiles) break;
		++s[k];
	}
}

// ---- lds_count and join_global_upper: every array over {0, 1, 2} of length 0 .. 6
template <typename K> static void counts_and_upper_bounds()
{
	const KeyCodec<K> codecs[3] = { key_codec<K>(sizeof(K) == 4 ? kKeyU32 : kKeyU64), key_codec<K>(sizeof(K) == 4 ? kKeyI32 : kKeyI64),
					key_codec<K>(sizeof(K) == 4 ? kKeyF32 : kKeyF64) };
	for (uint32_t len = 0; len <= 6; ++len) {
		uint32_t arrays = 1;
		for (uint32_t i = 0; i < len; ++i) arrays *= 3;
		for (uint32_t code = 0; code < arrays; ++code) {
			std::vector<K> x(len);
			bool ascending = true;
			for (uint32_t i = 0, c = code; i < len; ++i, c /= 3) {
				x[i] = (K)(c % 3);
				ascending = ascending && (i == 0 || x[i - 1] <= x[i]);
			}
			const std::unique_ptr<K[]> p = block(x);
			for (K v = 0; v < 3; ++v) {
				for (int right = 0; right < 2; ++right) {
					const uint32_t got = lds_count<K>(p.get(), len, v, right != 0);
					CHECK(got <= len);
					if (ascending) {
						uint32_t want = 0;
						for (uint32_t i = 0; i < len; ++i) want += search_counts<K>(x[i], v, right != 0) ? 1u : 0u;
						CHECK(got == want);
					}
				}
				for (const KeyCodec<K> &cd : codecs) {
					bool codes_ascending = true;
					for (uint32_t i = 1; i < len; ++i) codes_ascending = codes_ascending && cd.enc(x[i - 1]) <= cd.enc(x[i]);
					const K cv = cd.enc(v);
					for (uint64_t lo = 0; lo <= len; ++lo) {
						for (uint64_t hi = lo; hi <= len; ++hi) {
							const uint64_t got = join_global_upper<K>(p.get(), lo, hi, cv, cd);
							CHECK(lo <= got && got <= hi);
							if (codes_ascending) {
								uint64_t want = lo;
								for (uint64_t i = lo; i < hi; ++i) want += cd.enc(x[i]) <= cv ? 1u : 0u;
								CHECK(got == want);
							}
						}
					}
				}
			}
		}
	}
}

int main()
{
	for (uint64_t n = 0; n <= 6; ++n) {
		for (uint64_t m = 0; m <= 6; ++m) {
			extents_of<1>(n, m);
			extents_of<3>(n, m);
			extents_of<8>(n, m);
		}
	}
	counts_and_upper_bounds<uint32_t>();
	counts_and_upper_bounds<uint64_t>();
	printf("%ld checks, %ld failed\n", checks, failures);
	return failures ? 1 : 0;
}

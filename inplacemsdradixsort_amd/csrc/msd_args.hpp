// msd_args.hpp -- the argument rules of the entry points of msd_radix.hip and their run-time -> compile-time choices, each
// stated once.  Host only: plain C++17 without a HIP header and without msd_ctx, so that a host
// compiler takes it alone and the rules are tested without a GPU (tests/arg_rules_main.cpp).  Messages stay with the callers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace msd {

inline bool aligned_to(const void *p, uint32_t align) { return (uintptr_t)p % align == 0; } // (a null pointer is aligned)
inline bool aligned16(const void *p) { return aligned_to(p, 16); }

// an array of this many elements or more is refused (block slots are 32 bits wide)
constexpr uint64_t kMaxElems = (uint64_t)1 << 36;

// Do the byte ranges [a, a + abytes) and [b, b + bbytes) share an address?  An empty range strictly inside the other one
// counts as sharing (a pointer into the other buffer was handed in); a null pointer with 0 bytes -- an absent optional
// buffer, the only empty range the select entry points pass -- shares nothing with any range.
inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	return x < y + bbytes && y < x + abytes;
}

// ---- a call's buffers as one table: the inputs first, then the outputs
struct Span { const void *p; uint64_t bytes; uint32_t align; }; // (the pointer must be a multiple of `align`)

// `count` elements of `elem` bytes that must be aligned to `align` (0: to `elem`); an absent buffer (null) is empty.  A byte
// count beyond 64 bits saturates: the callers refuse such a count before they look at an extent, but behind the alignment rule.
inline Span span_of(const void *p, uint64_t count, uint32_t elem, uint32_t align = 0)
{
	uint64_t bytes = 0;
	if (p && __builtin_mul_overflow(count, (uint64_t)elem, &bytes)) bytes = UINT64_MAX;
	return { p, bytes, align ? align : elem };
}

// the first span whose pointer is not a multiple of its `align`, or -1 (a null pointer is aligned)
template <size_t N> inline int first_misaligned(const Span (&s)[N])
{
	for (size_t i = 0; i < N; ++i)
		if (!aligned_to(s[i].p, s[i].align)) return (int)i;
	return -1;
}

// Does any span from index `first_output` on overlap any span in front of it?  (Inputs may share memory with each other.)
template <size_t N> inline bool outputs_overlap(const Span (&s)[N], size_t first_output)
{
	for (size_t o = first_output; o < N; ++o)
		for (size_t i = 0; i < o; ++i)
			if (ranges_overlap(s[o].p, (size_t)s[o].bytes, s[i].p, (size_t)s[i].bytes)) return true;
	return false;
}

// ---- rows of a matrix: `rows` rows of `row_len` keys of `es` bytes, `row_stride` keys apart, `out_len` outputs per row
enum RowsOverflow { kRowsFit = 0, kRowsInputOverflows, kRowsOutputOverflows };
struct RowsExtents {
	RowsOverflow overflow; // rows * row_stride (* es), or rows * out_len (* 8), does not fit 64 bits: the rest is zero
	uint64_t out_elems;    // rows * out_len
	uint64_t in_bytes;     // the input's extent: the padding behind the last row is not part of it
	uint64_t out_bytes;    // out_elems keys
	uint64_t idx_bytes;    // out_elems 64-bit positions, 0 without them
};
inline RowsExtents rows_extents(uint64_t rows, uint64_t row_len, uint64_t row_stride, uint64_t out_len, uint64_t es, bool with_idx)
{
	RowsExtents e = { kRowsFit, 0, 0, 0, 0 };
	uint64_t in_elems = 0, in_all = 0, idx_all = 0;
	if (__builtin_mul_overflow(rows, row_stride, &in_elems) || __builtin_mul_overflow(in_elems, es, &in_all))
		e.overflow = kRowsInputOverflows;
	else if (__builtin_mul_overflow(rows, out_len, &e.out_elems) || __builtin_mul_overflow(e.out_elems, (uint64_t)8, &idx_all))
		e.overflow = kRowsOutputOverflows;
	if (e.overflow || rows == 0) return RowsExtents{ e.overflow, 0, 0, 0, 0 };
	e.in_bytes = ((rows - 1) * row_stride + row_len) * es;
	e.out_bytes = e.out_elems * es;
	e.idx_bytes = with_idx ? idx_all : 0;
	return e;
}

// ---- a run-time value picks a template argument: f gets a value of the type that carries it, like with_key_type

// element width in bytes -> f(uint32_t()) or f(uint64_t()); kNoWidth (not an MSD_ code), as f's result type, for any other width
constexpr int kNoWidth = 1;
template <typename F> inline auto with_width(int bytes, F &&f) -> decltype(f(uint32_t()))
{
	if (bytes == 4) return f(uint32_t());
	if (bytes == 8) return f(uint64_t());
	return static_cast<decltype(f(uint32_t()))>(kNoWidth);
}

// f(std::true_type()) or f(std::false_type()): both arms are instantiated
template <typename F> inline auto with_flag(bool flag, F &&f) { return flag ? f(std::true_type()) : f(std::false_type()); }

// lanes per row of the row kernels: f(std::integral_constant<int, 64 | 256 | 1024>()), the widest for any other value
template <typename F> inline auto with_lanes(int lanes, F &&f)
{
	if (lanes == 64) return f(std::integral_constant<int, 64>());
	if (lanes == 256) return f(std::integral_constant<int, 256>());
	return f(std::integral_constant<int, 1024>());
}

} // namespace msd

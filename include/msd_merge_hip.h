/*
 * msd_merge_hip.h -- merge of two sorted arrays: two arrays that are each ascending in the library's order become
 * one (libinpmsdradix_hip.so; contexts, error codes and MSD_KEY_* come from msd_radix_hip.h).  This is how a
 * sorted table is kept sorted as sorted batches arrive, how the sorted ranges of two ranks are joined, and how
 * sorted runs are united in front of msd_run_encode / msd_reduce_runs -- without sorting the concatenation again:
 * each input is read once and the output written once.  (msd_merge_buckets_* of msd_radix_hip.h is something else:
 * the counting leaf of the multi-GPU sort.)
 *
 * THE ORDER is that of msd_sort_keys: unsigned order of the keys' codes (csrc/msd_keycodec.hpp), which for floats
 * is IEEE-754 totalOrder on the bit patterns: -0.0 lies below +0.0 and the two stay apart; a NaN is an ordinary
 * key, a +NaN above +inf, a -NaN (sign bit set) below -inf, NaNs of one sign ordered by payload.  An array sorted
 * by torch.sort is in this order only if it holds no -NaN and no zeros of both signs.
 *
 * How: the merged sequence is cut into tiles along the merge path (one binary search per tile); one workgroup per
 * tile loads its piece of both arrays into the LDS, ranks every element among the tile's elements of the other
 * array, and stores its slice of the output coalesced.  No workgroup waits for another one and there are no
 * atomics: stream order is the only barrier.
 */
#ifndef MSD_MERGE_HIP_H_
#define MSD_MERGE_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_a holds n keys and d_b holds m keys of key_type (MSD_KEY_U32 .. MSD_KEY_F64), both ascending in the order
 * above -- what msd_sort_keys produces; both TRUSTED, not checked.
 *
 *   d_out receives the n + m keys in ascending order, bit-exact: every output is the bit pattern of an input
 *       (-0.0 and +0.0 stay apart, NaN payloads survive).
 *   The merge is stable: among keys with equal codes all of d_a's come before all of d_b's, and within one side
 *       equal keys keep their order.  The result is exactly the stable sort of the concatenation [A; B] by code.
 *   d_out_vals (optional, n + m words): the 8-byte values d_vals_a (n words) and d_vals_b (m words) travel with
 *       their keys.  d_out_vals requires d_vals_a when n > 0 and d_vals_b when m > 0; a value input without
 *       d_out_vals is refused.
 *   d_out_origin (optional, n + m words): d_out_origin[p] = the index in the concatenation [A; B] of the element
 *       at position p: i for d_a[i], n + i for d_b[i].  It is the argsort of the concatenation.
 *
 * n == 0 or m == 0 copies the other side.  n + m == 0 writes nothing and launches nothing.  Exactly n + m
 * elements of every given output are written and nothing else.  Inputs that are NOT ascending give unspecified
 * values in the outputs -- but every extent in the kernels is clamped: every load stays inside the input arrays
 * and every store inside [0, n + m) of its output.
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not wait.
 * Scratch: one 8-byte split per tile plus one, in the context's workspace like the sort's (msd_workspace_bytes
 * shows it).  Phase: "merge_sorted".
 *
 * Pointers need only the alignment of their element type; the arrays may sit anywhere on the 16-byte grid.
 * d_out is NOT in place: no output may overlap an input or another output.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; an unknown
 * key_type; a null d_out with n + m > 0; a null d_a with n > 0 or a null d_b with m > 0; the value rules
 * (d_out_vals without d_vals_a when n > 0 or without d_vals_b when m > 0; d_vals_a or d_vals_b without
 * d_out_vals); a pointer that is not aligned to its element size (d_a, d_b, d_out: the key's width; the others:
 * 8); n or m >= 2^36; any of d_out, d_out_vals, d_out_origin overlapping any input or each other. */
int msd_merge_sorted(msd_ctx *ctx, const void *d_a, uint64_t n, const void *d_b, uint64_t m, int key_type,
                     const uint64_t *d_vals_a, const uint64_t *d_vals_b,
                     void *d_out, uint64_t *d_out_vals, uint64_t *d_out_origin);

/* The geometry: *tile = the elements (of A and B together) one workgroup takes for that key width.  Host only,
 * no context.  Returns -1 for a key_bytes other than 4 or 8 or a null pointer, and leaves *tile untouched. */
int msd_merge_sorted_limits(int key_bytes, uint64_t *tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_MERGE_HIP_H_ */

/*
 * msd_setops_hip.h -- set operations on two sorted arrays: the intersection, union, difference or symmetric
 * difference of two arrays that are each ascending in the library's order, as a set: every value at most once,
 * ascending (libinpmsdradix_hip.so; contexts, error codes and MSD_KEY_* come from msd_radix_hip.h).  These are
 * numpy's intersect1d, union1d, setdiff1d and setxor1d on arrays that are already sorted.  A union is what the merge
 * of msd_merge_hip.h followed by the run-length encode of msd_runs_hip.h gives, and the other three what two
 * sorted searches and a mask give -- here each input is read twice and the result written once, and nothing as
 * long as the inputs lies in between.
 *
 * THE ORDER is that of msd_sort_keys: unsigned order of the keys' codes (csrc/msd_keycodec.hpp), which for floats
 * is IEEE-754 totalOrder on the bit patterns: -0.0 lies below +0.0; a NaN is an ordinary key, a +NaN above +inf, a
 * -NaN (sign bit set) below -inf, NaNs of one sign ordered by payload.  An array sorted by torch.sort is in this
 * order only if it holds no -NaN and no zeros of both signs.
 *
 * EQUALITY is equality of codes, which is equality of BITS: -0.0 and +0.0 are two values (with -0.0 only in B and
 * +0.0 only in A both are in the union and neither is in the intersection); NaNs with equal bits are one value and
 * intersect, NaNs of different sign or payload do not.  numpy and torch compare floats by value instead.
 *
 * How: the merged sequence of the two arrays is cut into tiles along the merge path (one binary search per tile);
 * one workgroup per tile loads its piece of both arrays into the LDS and decides for every element whether it is
 * the first of its value and whether the other side holds the value too.  The tiles' counts are scanned, and a
 * second pass over the tiles stores the kept elements at their places, coalesced.  No workgroup waits for another
 * one and there are no atomics: stream order is the only barrier.
 */
#ifndef MSD_SETOPS_HIP_H_
#define MSD_SETOPS_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* op */
#define MSD_SET_INTERSECTION 0         /* the values present in both */
#define MSD_SET_UNION 1                /* the values present in either */
#define MSD_SET_DIFFERENCE 2           /* the values of A absent from B */
#define MSD_SET_SYMMETRIC_DIFFERENCE 3 /* the values present in exactly one */

/* d_a holds n keys and d_b holds m keys of key_type (MSD_KEY_U32 .. MSD_KEY_F64), both ascending in the order
 * above -- what msd_sort_keys produces; both TRUSTED, not checked, and not modified.  Duplicates inside either
 * input are allowed.
 *
 *   The result is a set: each value at most once, ascending, bit-exact (every result is the bit pattern of an
 *       input): np.intersect1d / union1d / setdiff1d / setxor1d on the codes.
 *   *d_num_out (required, one device word) always receives the TRUE number of results, also when that exceeds
 *       cap -- as *d_num_runs of msd_runs_hip.h does.
 *   d_out (optional, cap keys): the results j < min(count, cap) are written and nothing beyond them.
 *   d_out_origin (optional, cap words; may be given without d_out): for result j the index in the concatenation
 *       [A; B] of the first occurrence of that value: i for a value taken from d_a[i], n + i for one taken from
 *       d_b[i].  A value that both sides hold is taken from A, so intersection and difference only ever name A.
 *       It is the rule of np.unique(return_index=True) on the concatenation, and of the origin of msd_merge_hip.h.
 *
 * n == 0 or m == 0 is legal and gives the empty result or the distinct values of the other side.  n + m == 0
 * writes *d_num_out = 0 (one small launch).  cap == 0 is legal and only counts, as do a null d_out together with
 * a null d_out_origin.  A count can be at most min(n, m) for an intersection, n for a difference and n + m for a
 * union or a symmetric difference: a cap of that bound holds every result.
 *
 * Inputs that are NOT ascending give unspecified values and counts -- but every extent in the kernels is clamped:
 * every load stays inside its input array and every store inside [0, min(count, cap)) of its output.
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not wait.  No
 * atomics, and no workgroup waits for another one.  Scratch, in the context's workspace like the sort's
 * (msd_workspace_bytes shows it): one 8-byte split per tile plus one, one 8-byte count per tile, one 8-byte sum
 * per scan piece.  Phase: "set_sorted".
 *
 * Pointers need only the alignment of their element type; the arrays may sit anywhere on the 16-byte grid.
 * Nothing is in place: no output may overlap an input or another output.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; an unknown
 * key_type; an unknown op; a null d_num_out; a null d_a with n > 0; a null d_b with m > 0; a pointer that is not
 * aligned to its element size (d_a, d_b, d_out: the key's width; the others: 8); n or m >= 2^36; any of d_out,
 * d_out_origin, d_num_out overlapping an input or each other, where d_out and d_out_origin are taken as
 * min(cap, bound) elements long -- the most that can be written -- with the bound of the operation above. */
int msd_set_sorted(msd_ctx *ctx, int op, const void *d_a, uint64_t n, const void *d_b, uint64_t m, int key_type,
                   uint64_t cap, void *d_out, uint64_t *d_out_origin, uint64_t *d_num_out);

/* The geometry: *tile = the elements (of A and B together) one workgroup takes for that key width, *scan_tile =
 * the tile counts one workgroup of the scan takes.  Host only, no context.  Returns -1 for a key_bytes other than
 * 4 or 8 or a null pointer, and leaves both untouched. */
int msd_set_sorted_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_SETOPS_HIP_H_ */

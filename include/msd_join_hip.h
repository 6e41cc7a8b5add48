/*
 * msd_join_hip.h -- sort-merge join of two sorted arrays: for two arrays that are each ascending in the library's
 * order, every pair of indices (i, j) with A[i] equal to B[j] (libinpmsdradix_hip.so; contexts, error codes and
 * MSD_KEY_* come from msd_radix_hip.h).  It is the inner equi-join of two sorted key columns; the index pairs
 * feed a gather of whatever columns travel with the keys.
 *
 * The join comes in two calls, because what lies between them is small, useful alone and owned by the caller:
 * the MATCHED GROUPS.  For every value that both arrays hold, ascending: the key, the index of its first occurrence
 * in A and the length of its run in A, and the same two numbers for B.  There are at most min(distinct A,
 * distinct B) of them.  They are the join in CSR form, and they are all that count(*) and an aggregate over the
 * join need: group g stands for a_count[g] * b_count[g] pairs.  msd_join_pairs expands them into index pairs.
 * Because the caller owns the groups, the library needs no scratch as long as an input.
 *
 * THE ORDER is that of msd_sort_keys_hip.h: unsigned order of the keys' codes (csrc/msd_keycodec.hpp), which for
 * floats is IEEE-754 totalOrder on the bit patterns: -0.0 lies below +0.0; a NaN is an ordinary key, a +NaN above
 * +inf, a -NaN (sign bit set) below -inf, NaNs of one sign ordered by payload.
 *
 * EQUALITY is equality of codes, which is equality of BITS, as in msd_setops_hip.h: -0.0 and +0.0 are two values
 * and do not join; NaNs with equal bits are one value and join, NaNs of different sign or payload do not.  SQL,
 * numpy and torch compare floats by value instead.
 *
 * How: the groups are found like the intersection of msd_setops_hip.h -- the merged sequence cut into tiles
 * along the merge path, one workgroup per tile, the tiles' counts scanned, a second pass that writes -- and the
 * second pass also finds where the two runs end: inside the tile, or, for at most one value per tile and side
 * whose run leaves the tile, by one binary search behind it.  The pairs are expanded by OUTPUT rank: the groups'
 * products are scanned, and every workgroup takes a fixed range of pair ranks, finds the groups that overlap it
 * and stores coalesced -- one group of a billion pairs and a million groups of one pair are the same work per
 * workgroup.  No workgroup waits for another one and there are no atomics: stream order is the only barrier.
 */
#ifndef MSD_JOIN_HIP_H_
#define MSD_JOIN_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The matched groups.  d_a holds n keys and d_b holds m keys of key_type (MSD_KEY_U32 .. MSD_KEY_F64), both
 * ascending in the order above -- what msd_sort_keys_hip.h produces; both TRUSTED, not checked, and not modified.
 * Duplicates inside either input are allowed; they are what makes a group larger than one pair.
 *
 *   *d_num_groups (required, one device word) always receives the TRUE number of groups, also when that exceeds
 *       cap.  It is at most min(n, m): a cap of that bound holds every group.
 *   For group g < min(count, cap), in ascending order of the value (nothing beyond them is written):
 *   d_keys[g]     (optional, cap keys): the value, bit-exact (the bit pattern of A's first occurrence).
 *   d_a_first[g]  (optional, cap words): the index in A of the first occurrence of the value.
 *   d_a_count[g]  (optional, cap words): the length of its run in A (>= 1).
 *   d_b_first[g], d_b_count[g] (optional, cap words each): the same for B.
 *
 * d_keys and d_a_first are exactly d_out and d_out_origin of MSD_SET_INTERSECTION (msd_setops_hip.h) on the same
 * inputs, and *d_num_groups is that call's count.
 *
 * n == 0 or m == 0 is legal and gives no group.  n + m == 0 writes *d_num_groups = 0 (one small launch).
 * cap == 0 is legal and only counts, as does a call with none of the five arrays.
 *
 * Inputs that are NOT ascending give unspecified values and counts -- but every extent in the kernels is clamped:
 * every load stays inside its input array and every store inside [0, min(count, cap)) of its output, and every
 * stored group lies inside the arrays: a_count >= 1, a_first + a_count <= n and b_first + b_count <= m.
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not wait.  No
 * atomics, and no workgroup waits for another one.  Scratch, in the context's workspace like the sort's
 * (msd_workspace_bytes shows it): one 8-byte split per tile plus one, one 8-byte count per tile, one 8-byte sum
 * per scan piece.  Phase: "join_groups".
 *
 * Pointers need only the alignment of their element type; the arrays may sit anywhere on the 16-byte grid.
 * Nothing is in place: no output may overlap an input or another output.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; an unknown
 * key_type; a null d_num_groups; a null d_a with n > 0; a null d_b with m > 0; a pointer that is not aligned to
 * its element size (d_a, d_b, d_keys: the key's width; the others: 8); n or m >= 2^32 -- so that every product
 * a_count * b_count and the number of pairs, at most n * m, fit 64 bits; any of the five arrays or d_num_groups
 * overlapping an input or each other, where the arrays are taken as min(cap, n, m) elements long -- the most
 * that can be written. */
int msd_join_groups(msd_ctx *ctx, const void *d_a, uint64_t n, const void *d_b, uint64_t m, int key_type,
                    uint64_t cap, void *d_keys, uint64_t *d_a_first, uint64_t *d_a_count,
                    uint64_t *d_b_first, uint64_t *d_b_count, uint64_t *d_num_groups);

/* The index pairs of the groups.  d_num_groups (one device word) and the four arrays of groups_cap words each
 * are what msd_join_groups wrote with cap = groups_cap: the call uses G = min(*d_num_groups, groups_cap) groups.
 * If the groups call was TRUNCATED by its cap (*d_num_groups > groups_cap), the pairs and their count are those
 * of the stored groups only.  n and m are the lengths of A and B.  The groups are TRUSTED: first + count within
 * the array, counts >= 1.
 *
 * Pair number r is defined in lexicographic order of (index in A, index in B): the groups in order, and within
 * group g of sizes p x q the local rank t = r - (the pairs of the groups in front) gives
 *       ia = a_first[g] + t / q,   ib = b_first[g] + t % q.
 *
 *   *d_num_pairs (required, one device word) always receives the TRUE total, the sum of p * q over the G groups,
 *       also when that exceeds cap.
 *   d_out_a, d_out_b (each optional, cap words): ia and ib of the pairs r < min(total, cap); nothing beyond.
 *   d_pos_a (optional, n words), d_pos_b (optional, m words): with it the stored value is d_pos_a[ia] instead of
 *       ia (d_pos_b[ib] instead of ib): the positions a sort of an unsorted table delivered, as the
 *       sorted search and the reduce-by-key of this library take them, so that a join of unsorted tables needs
 *       no gather of its own.
 *
 * cap == 0 is legal and only counts, as does a call with neither output.  groups_cap == 0 writes
 * *d_num_pairs = 0.  The total is at most n * m: a cap of that bound holds every pair.
 *
 * Groups that are not what msd_join_groups writes give unspecified values and counts -- but every group index
 * stays below groups_cap, ia < n and ib < m are clamped before a position is loaded, and every store stays
 * inside [0, min(total, cap)) of its output.
 *
 * Asynchronous as above; nothing is read back: the grid of the expansion is that of min(cap, n * m) ranks, and
 * a workgroup whose ranks lie beyond min(total, cap) leaves before it loads anything else.  Scratch, in the
 * context's workspace: one 8-byte offset per group of groups_cap, one 8-byte sum per scan piece; groups_cap
 * may lie far above the number of groups: what lies behind the last group costs no traffic.
 * Phase: "join_pairs".
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; a null
 * d_num_pairs; with groups_cap > 0 a null d_num_groups, then a null d_a_first, d_a_count, d_b_first or
 * d_b_count; a pointer that is not aligned to 8 bytes; n or m >= 2^32; groups_cap >= 2^32; with an output,
 * min(cap, n * m) >= 2^40 (split such an expansion into several calls over group ranges); any of d_out_a,
 * d_out_b, d_num_pairs overlapping an input or each other, where the outputs are taken as min(cap, n * m)
 * words long. */
int msd_join_pairs(msd_ctx *ctx, uint64_t groups_cap, const uint64_t *d_num_groups,
                   const uint64_t *d_a_first, const uint64_t *d_a_count,
                   const uint64_t *d_b_first, const uint64_t *d_b_count,
                   uint64_t n, uint64_t m, const uint64_t *d_pos_a, const uint64_t *d_pos_b,
                   uint64_t cap, uint64_t *d_out_a, uint64_t *d_out_b, uint64_t *d_num_pairs);

/* The geometry: *tile = the elements (of A and B together) one workgroup of the groups call takes for that key
 * width, *scan_tile = the counts one workgroup of a scan takes, *pair_tile = the pair ranks one workgroup of the
 * expansion takes.  Host only, no context.  Returns -1 for a key_bytes other than 4 or 8 or a null pointer, and
 * leaves all three untouched. */
int msd_join_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile, uint64_t *pair_tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_JOIN_HIP_H_ */

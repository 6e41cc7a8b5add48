/*
 * msd_search_hip.h -- sorted search: where does a value lie in a sorted array?  The lower or the upper bound of
 * every needle in an array that is sorted in the library's order (libinpmsdradix_hip.so; contexts, error codes
 * and MSD_KEY_* come from msd_radix_hip.h).  This is torch.searchsorted / torch.bucketize in the key order of
 * this library: the lookup of a key in the distinct keys of a group-by, the probe side of a sort-merge join
 * (upper - lower = the number of matches), a histogram over arbitrary edges, a rank query.
 *
 * THE ORDER is that of msd_sort_keys: unsigned order of the keys' codes (csrc/msd_keycodec.hpp), which for
 * floats is IEEE-754 totalOrder on the bit patterns.  It DIFFERS from torch.searchsorted:
 *   - -0.0 lies below +0.0: MSD_SEARCH_LEFT of +0.0 points BEHIND the -0.0s of the array, MSD_SEARCH_RIGHT of
 *     -0.0 in front of its +0.0s;
 *   - a NaN is an ordinary key: a +NaN lies above +inf, a -NaN (sign bit set) below -inf, and NaNs of one sign
 *     are ordered by their payload.  A NaN needle finds its place among them;
 *   - an array sorted by torch.sort is in this order only if it holds no -NaN and no zeros of both signs.
 *
 * How: two paths.  DIRECT: every lane runs a branch-free binary search for several needles at once, so that the
 * dependent loads of one needle overlap those of the others.  MERGE, for needles that are themselves ascending:
 * keys and needles are cut into tiles along the merge path (one binary search per tile), and every tile is
 * loaded once, coalesced, and searched in the LDS -- both arrays are read once and nothing is loaded at random.
 * No workgroup waits for another one and there are no atomics: stream order is the only barrier.
 */
#ifndef MSD_SEARCH_HIP_H_
#define MSD_SEARCH_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MSD_SEARCH_LEFT = 0, MSD_SEARCH_RIGHT = 1 };

/* d_sorted holds n keys of key_type (MSD_KEY_U32 .. MSD_KEY_F64), ascending in the order above -- what
 * msd_sort_keys produces; TRUSTED, not checked.  d_needles holds m keys of the same type.
 *
 *   r_j = the number of keys whose code is < (MSD_SEARCH_LEFT: the lower bound) or <= (MSD_SEARCH_RIGHT: the
 *       upper bound) the code of needle j; 0 <= r_j <= n.
 *   d_out[j] = r_j, or with d_positions (optional, m words, TRUSTED to be a permutation of [0, m), as
 *       msd_sort_rows or msd_sort_pairs_keys produce them) d_out[d_positions[j]] = r_j.  Exactly m words of
 *       d_out are written and nothing else.
 *
 * needles_sorted = 0: nothing is assumed about the needles; the direct path runs.
 * needles_sorted = 1: the needles are TRUSTED to be ascending in the same order.  The option "search_mode"
 *   (msd_set_option) then chooses: 0 = the library chooses -- the merge path when m >= n / R, else the direct
 *   path; 1 = always direct; 2 = always merge.  R is the option "search_merge_ratio" (>= 1), 32 by default:
 *   MEASURED on an MI355X with sorted uniform needles: into 2^30 sorted 4-byte keys the direct path wins at
 *   m = n / 64 and the merge path at m = n / 32; into 2^29 sorted 8-byte keys the direct path wins at m = n / 32
 *   and the merge path at m = n / 16.  Interpolated, the two cross near m = n / 37 and m = n / 24; 32 is the
 *   nearest power of two to both.
 *   With needles_sorted = 0 search_mode 2 still runs direct.  Needles that are NOT ascending give unspecified
 *   values in d_out under the merge path -- but every extent in the kernels is clamped: every load stays inside
 *   the two input arrays and every store inside d_out[0, m).
 *
 * n == 0: every result is 0.  m == 0: nothing is written.
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not wait.
 * Scratch: the merge path takes one 8-byte split per tile plus one, in the context's workspace like the sort's
 * (msd_workspace_bytes shows it).  Phase: "search_sorted".
 *
 * Pointers need only the alignment of their element type; the arrays may sit anywhere on the 16-byte grid.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; an unknown
 * key_type; a side other than 0 or 1, or a needles_sorted other than 0 or 1; a null d_out with m > 0; a null
 * d_needles with m > 0; a null d_sorted with n > 0 and m > 0; a pointer that is not aligned to its element size
 * (d_sorted, d_needles: the key's width; d_positions, d_out: 8); n or m >= 2^36; d_out (m words) overlapping
 * d_sorted, d_needles or d_positions. */
int msd_search_sorted(msd_ctx *ctx, const void *d_sorted, int key_type, uint64_t n,
                      const void *d_needles, uint64_t m, int needles_sorted, int side,
                      const uint64_t *d_positions, uint64_t *d_out);

/* The geometry: *tile = the elements (keys plus needles together) one workgroup of the merge path takes for that
 * key width, *direct_tile = the needles one workgroup of the direct path takes.  Host only, no context.  Returns
 * -1 for a key_bytes other than 4 or 8 or a null pointer, and leaves the outputs untouched. */
int msd_search_sorted_limits(int key_bytes, uint64_t *tile, uint64_t *direct_tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_SEARCH_HIP_H_ */

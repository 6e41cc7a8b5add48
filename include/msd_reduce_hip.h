/*
 * msd_reduce_hip.h -- reduce-by-key over runs: one number per run of equal keys, the sum, the minimum or
 * the maximum of a value column (libinpmsdradix_hip.so; contexts, error codes and MSD_KEY_* come from
 * msd_radix_hip.h).
 *
 * The RUNS are exactly those of msd_run_encode (msd_runs_hip.h): maximal stretches of consecutive keys
 * with equal BIT patterns.  Run j of this call is run j of msd_run_encode on the same array, so that
 * d_values[j], d_starts[j] and d_out[j] belong together.  On keys sorted with positions or rids this is
 * the last step of a group-by: the value column stays where it was and is read through the positions.
 *
 * How: the tiles, head ballots, count and scan of msd_run_encode, then (2) every tile reads its keys
 * again and its values once and reduces them by a segmented scan -- every run that starts in the tile
 * stores its part inside the tile, and the tile records the reduction of the elements in front of its
 * first head --, (3) a segmented scan over the tile records, from right to left and two levels deep,
 * hands every tile's last run what the tiles behind it hold of it.  No workgroup waits for another one,
 * and there are no atomics: stream order is the only barrier.
 */
#ifndef MSD_REDUCE_HIP_H_
#define MSD_REDUCE_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MSD_REDUCE_SUM = 0, MSD_REDUCE_MIN = 1, MSD_REDUCE_MAX = 2 };

/* d_keys holds n elements of key_bytes (4 or 8); m is the number of its runs.
 *
 * Values: val_type is one of MSD_KEY_U32 .. MSD_KEY_F64; its width may differ from the keys'.  The value
 * of element i is d_vals[i], or with d_positions (optional, n words, TRUSTED to lie in [0, n), as
 * msd_sort_rows or msd_sort_pairs_keys produce them) d_vals[d_positions[i]].  No gathered copy of the
 * values is made.
 *
 *   *d_num_runs = m.  A device word, required.  Always the true count, also when m > cap: that is how a
 *       caller detects overflow.
 *   d_out[j] for j < min(m, cap) = the reduction of run j.  Nothing at index >= min(m, cap) is written.
 *
 * MSD_REDUCE_SUM: d_out holds 8-byte elements whatever the value type.  U32 and U64 sum into a uint64_t,
 *   I32 and I64 into an int64_t, both exact modulo 2^64.  F32 and F64 sum in and into a double (a float
 *   converts exactly).  A float sum is evaluated in an order that the tile geometry alone fixes -- the
 *   pointers' places on the 16-byte grid and n --, without atomics: the same call on the same buffers
 *   gives the same bits every time.  The order is not that of a sequential loop, so the sum differs from
 *   one by rounding, and a sum that is zero may carry either sign.
 * MSD_REDUCE_MIN / MSD_REDUCE_MAX: d_out holds elements of the value's own type, bit-exact.  The order is
 *   that of the type through the library's key codes (encode, unsigned minimum or maximum, decode); for
 *   floats that is IEEE-754 totalOrder, as everywhere in this library: -0.0 is below +0.0, a +NaN is the
 *   maximum of its run and a -NaN (sign bit set) the minimum.  This DIFFERS from torch.amax / torch.amin,
 *   which propagate any NaN: here a NaN is just the largest or the smallest value.
 *
 * n == 0: m = 0, nothing else is written.  cap == 0 is legal (counting only).
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not
 * wait.  Scratch: per tile one word (the count), one 8-byte lead and one 4-byte head count, and the same
 * per scan piece, in the context's workspace like the sort's (msd_workspace_bytes shows it).  Phase:
 * "reduce_runs".
 *
 * Pointers need only the alignment of their element type; keys and values may sit at different places of
 * the 16-byte grid.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; key_bytes
 * other than 4 or 8; an unknown val_type; an unknown op; a null d_num_runs; a null d_keys or d_vals with
 * n > 0; a null d_out with cap > 0 and n > 0; a pointer that is not aligned to its element size (d_keys:
 * key_bytes; d_vals: the value's width; d_out: 8 for a sum, else the value's width; the others: 8);
 * n >= 2^36; d_out -- taken as min(cap, n) elements, the most that can be written -- or d_num_runs
 * overlapping d_keys, d_vals, d_positions or each other. */
int msd_reduce_runs(msd_ctx *ctx, const void *d_keys, int key_bytes, uint64_t n,
                    const void *d_vals, int val_type, const uint64_t *d_positions,
                    int op, uint64_t cap, void *d_out, uint64_t *d_num_runs);

/* The geometry, the same as msd_run_encode_limits: *tile = the keys one workgroup takes per tile for that
 * key width, *scan_tile = how many tile records one workgroup of the scans takes at once.  Host only, no
 * context.  Returns -1 for a key_bytes other than 4 or 8 or a null pointer, and leaves the outputs
 * untouched. */
int msd_reduce_runs_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_REDUCE_HIP_H_ */

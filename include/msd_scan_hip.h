/*
 * msd_scan_hip.h -- scan-by-key over runs: one number per ELEMENT, the running sum, minimum, maximum or
 * count inside its run of equal keys (libinpmsdradix_hip.so; contexts, error codes and MSD_KEY_* come
 * from msd_radix_hip.h).
 *
 * The RUNS are exactly those of msd_run_encode (msd_runs_hip.h) and msd_reduce_runs (msd_reduce_hip.h):
 * maximal stretches of consecutive keys with equal BIT patterns.  On sorted keys this is a window
 * function, OVER (PARTITION BY key ORDER BY the order of the elements): a running sum, a running extreme
 * or a row number per group.  The value column lies in the order of the keys (sorted along with them, or
 * gathered by the caller): d_positions and MSD_SCAN_SCATTER are part of the signature and NOT OFFERED
 * YET -- a call that passes d_positions is refused.
 *
 * How: the tiles and head ballots of msd_run_encode, then (1) every tile reads its keys and values and
 * records whether it has a head and its tail -- the reduction from its last head to its end --, (2) a
 * segmented scan over the tile records, from left to right and two levels deep, gives every tile what
 * the run that is open at its start holds in front of it, (3) every tile reads its keys and values
 * again, scans them on top of that and stores its results.  The runs are not numbered: the count and
 * scan steps of msd_run_encode are not run.  No workgroup waits for another one, and there are no
 * atomics: stream order is the only barrier.
 */
#ifndef MSD_SCAN_HIP_H_
#define MSD_SCAN_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MSD_SCAN_SUM = 0, MSD_SCAN_MIN = 1, MSD_SCAN_MAX = 2, MSD_SCAN_COUNT = 3 };   /* the first three = MSD_REDUCE_* */
enum { MSD_SCAN_EXCLUSIVE = 1, MSD_SCAN_SCATTER = 2 };                               /* flags, or-ed */

/* d_keys holds n elements of key_bytes (4 or 8).
 *
 * Values: val_type is one of MSD_KEY_U32 .. MSD_KEY_F64; its width may differ from the keys'.  The value
 * v(i) of element i is d_vals[i].  d_positions must be null: reading the values through positions
 * (d_vals[d_positions[i]]) and storing the results through them (MSD_SCAN_SCATTER,
 * d_out[d_positions[i]] = s(i)) are reserved for a later version and refused today.
 *
 * With start(i) = the first element of i's run:
 *   flags == 0 (inclusive):  s(i) = op over v(start(i)) .. v(i).
 *   MSD_SCAN_EXCLUSIVE:      s(i) = op over v(start(i)) .. v(i-1), and the op's IDENTITY at a head.
 *   d_out[i] = s(i).  Exactly n elements of d_out are written, and nothing else of the caller's.
 *
 * MSD_SCAN_SUM: d_out holds 8-byte elements whatever the value type.  U32 and U64 sum into a uint64_t,
 *   I32 and I64 into an int64_t, both exact modulo 2^64.  F32 and F64 sum in and into a double (a float
 *   converts exactly).  Identity: 0 (+0.0).
 *   Every float output is the sum of exactly the elements of its own prefix, combined from disjoint
 *   contiguous partial sums; it is never formed by subtraction -- in particular the exclusive result is
 *   NOT the inclusive one minus v(i), and an infinity or a NaN reaches the later elements of its own run
 *   and no other run.  The order of the additions is fixed by the tile geometry alone -- the keys' place
 *   on the 16-byte grid and n --, without atomics: the same call on the same buffers gives the same bits
 *   every time.  The order is not that of a sequential loop (nor that of torch.cumsum), so a result
 *   differs from one by rounding, and a zero may carry either sign.
 * MSD_SCAN_MIN / MSD_SCAN_MAX: d_out holds elements of the value's own type, bit-exact.  The order is
 *   that of the type through the library's key codes (encode, unsigned minimum or maximum, decode); for
 *   floats that is IEEE-754 totalOrder, as everywhere in this library: -0.0 is below +0.0, a +NaN is the
 *   largest value and a -NaN (sign bit set) the smallest.  This DIFFERS from torch.cummax / torch.cummin,
 *   which propagate any NaN to the rest of the array: here a NaN is just the largest or the smallest
 *   value, and a running maximum takes a -NaN for less than -inf.
 *   Identity of MIN: the decode of the all-ones code -- UINT32_MAX / UINT64_MAX, INT32_MAX / INT64_MAX,
 *   the +NaN with all payload bits set (0x7FFFFFFF, 0x7FFFFFFFFFFFFFFF).  Identity of MAX: the decode of
 *   code 0 -- 0, INT32_MIN / INT64_MIN, the -NaN with all payload bits set (all bits one).
 * MSD_SCAN_COUNT: d_vals and val_type are not looked at (d_vals may be null, val_type anything); every
 *   element counts 1.  d_out holds uint64_t: inclusive the 1-based, exclusive the 0-based row number
 *   inside the run.  Identity: 0.
 *
 * n == 0: MSD_OK, nothing is written and nothing launched.
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not
 * wait.  Scratch: per tile one 8-byte tail and one 4-byte flag, and the same per scan piece, in the
 * context's workspace like the sort's (msd_workspace_bytes shows it).  Phase: "scan_runs".
 *
 * Pointers need only the alignment of their element type; keys, values and output may sit at different
 * places of the 16-byte grid.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; key_bytes
 * other than 4 or 8; an unknown op; an unknown val_type unless the op is MSD_SCAN_COUNT; unknown flag
 * bits; MSD_SCAN_SCATTER without d_positions; a d_positions that is not null (not offered yet: so
 * MSD_SCAN_SCATTER is always refused); a null d_keys with n > 0; a null d_vals with n > 0 unless the op
 * is MSD_SCAN_COUNT; a null d_out with n > 0; a pointer that is not aligned to its element size
 * (d_keys: key_bytes; d_vals: the value's width; d_out: 8 for a sum or a count, else the value's width);
 * n >= 2^36; d_out -- taken as n elements -- overlapping d_keys or d_vals: in place is not offered. */
int msd_scan_runs(msd_ctx *ctx, const void *d_keys, int key_bytes, uint64_t n,
                  const void *d_vals, int val_type, const uint64_t *d_positions,
                  int op, int flags, void *d_out);

/* The geometry, the same as msd_run_encode_limits: *tile = the keys one workgroup takes per tile for that
 * key width, *scan_tile = how many tile records one workgroup of the carry scan takes at once.  Host
 * only, no context.  Returns -1 for a key_bytes other than 4 or 8 or a null pointer, and leaves the
 * outputs untouched. */
int msd_scan_runs_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile);   /* = msd_run_encode_limits */

#ifdef __cplusplus
}
#endif

#endif /* MSD_SCAN_HIP_H_ */

/*
 * msd_compact_hip.h -- stream compaction and stable partition: the filter a query pipeline starts with
 * (libinpmsdradix_hip.so; MSD_KEY_*, contexts and error codes come from msd_radix_hip.h).
 *
 * The elements that a predicate keeps leave in their original order (the call is STABLE): the WHERE
 * clause, x[mask], torch.masked_select, torch.nonzero, thrust's copy_if; with MSD_COMPACT_REST the
 * rejected elements follow the kept ones, in their original order too: thrust's stable_partition.
 * The true count of kept elements goes to a device word and the outputs are capped, so nothing waits
 * on the host, as in the run-length encode of msd_runs_hip.h.
 *
 * The predicate of element i:
 *
 *   keep(i) = [ (d_mask == NULL || d_mask[i] != 0)
 *               && (!(flags & MSD_COMPACT_RANGE) || lo <= code(d_keys[i]) <= hi) ]
 *             XOR (flags & MSD_COMPACT_INVERT)
 *
 * code is msd_key_encode of key_type, and lo / hi are the codes of lo_bits / hi_bits: bit patterns of
 * the key type (a 32-bit type takes the low 32 bits).  Both bounds are inclusive; lo == hi is
 * equality.  A range that is empty in code order (lo > hi) is legal and keeps nothing -- with
 * MSD_COMPACT_INVERT everything.  Any non-zero mask byte keeps: torch.bool, uint8 and int8 all work.
 * With neither a mask nor MSD_COMPACT_RANGE everything is kept (with MSD_COMPACT_INVERT nothing);
 * that is legal.
 *
 * Floats are compared in IEEE-754 totalOrder on their bits, as everywhere in the library:
 * -0.0 is below +0.0, so a lower bound of +0.0 excludes -0.0 and an upper bound of -0.0 excludes +0.0;
 * NaNs are ordinary keys, a +NaN above +inf and a -NaN (sign bit set) below -inf, among NaNs by
 * payload.  This differs from x >= lo in torch, where -0.0 >= +0.0 is true and every comparison with a
 * NaN is false: here the range [-inf, +inf] leaves the NaNs out as torch does, but the full range of
 * codes keeps them, [+0.0, +inf] drops the -0.0s that torch's x >= 0 keeps, and [+inf, +NaN with all
 * payload bits] keeps +inf and every +NaN.  Kept keys come back bit-exact: NaN payloads and the sign
 * of zero survive.
 *
 * How: three stream-ordered steps, no workgroup ever waits for another one and no atomics are used.
 * (1) every tile evaluates keep and counts, one word per tile; (2) the tile counts are scanned in
 * place, scan_tile words per workgroup, the piece totals by one more workgroup, whose last word is
 * the count; (3) every tile is read again, evaluates keep again, and writes: the kept elements are
 * compacted in the workgroup's local memory first, so the stores are coalesced whatever the
 * selectivity.  Keys and mask are therefore read twice, values once.
 */
#ifndef MSD_COMPACT_HIP_H_
#define MSD_COMPACT_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MSD_COMPACT_RANGE = 1, MSD_COMPACT_INVERT = 2, MSD_COMPACT_REST = 4 };   /* flags, or-ed */

/* Inputs.  d_keys: n elements of the width of key_type; may be null when neither MSD_COMPACT_RANGE
 * nor d_out_keys is given -- the mask-only form, torch.nonzero --, and key_type is then not looked
 * at.  d_mask: n bytes, optional.  d_vals: n elements of val_bytes (4 or 8, independent of the key
 * width), present exactly when d_out_vals is.  No input is modified.
 *
 * Outputs without MSD_COMPACT_REST.  With i_0 < i_1 < ... < i_{m-1} the kept indices:
 *
 *   *d_count = m.  A device word, required.  Always the true count, also when m > cap: that is how a
 *       caller detects overflow.
 *   d_out_keys[j] = d_keys[i_j] (bit-exact), d_out_vals[j] = d_vals[i_j], d_out_idx[j] = i_j for
 *       j < min(m, cap).  Each of the three is optional; with none of them the call only counts and
 *       the write pass is not launched.  Nothing beyond index min(m, cap) - 1 of any output is
 *       written.
 *
 * Outputs with MSD_COMPACT_REST (stable partition): the outputs are n elements long and cap must be
 * >= n.  The kept elements come first, as above, then the n - m rejected elements follow in their
 * original order; *d_count = m is the split point.  d_out_idx is then a permutation of [0, n), usable
 * as d_positions of the run-length encode (msd_runs_hip.h) and of the reduce-by-key over runs.
 *
 * n == 0: *d_count = 0 in one small launch, nothing else is written.  cap == 0 is legal (counting).
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not
 * wait.  Scratch: one 8-byte word per tile and one per scan piece, in the context's workspace like
 * the sort's (msd_workspace_bytes shows it; a workspace that has to grow is reallocated behind a
 * stream synchronisation, as for the sort).  Phase: "compact".
 *
 * Pointers need only the alignment of their element type, the mask none: keys, mask, values and
 * outputs may sit at different phases of the 16-byte grid of memory.  d_mask[-1] and d_mask[n] are
 * never read, nor is any key or value outside its array.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context; an
 * unknown key_type, unless d_keys is null; unknown flag bits; a null d_count; MSD_COMPACT_RANGE or
 * d_out_keys without d_keys; for a 32-bit key_type with MSD_COMPACT_RANGE, a bound with bits above
 * 2^32; d_vals without d_out_vals, or the reverse; val_bytes other than 4 or 8 when d_vals is given;
 * n > 0 with neither d_keys nor d_mask when d_out_keys or d_out_vals is asked for (there is nothing to
 * take elements from; d_out_idx alone stands, it needs no input); a pointer that is not aligned to its
 * element size (d_keys, d_out_keys: the key's; d_vals, d_out_vals: val_bytes; d_out_idx, d_count: 8);
 * n >= 2^36; MSD_COMPACT_REST with cap < n; any output (d_out_keys, d_out_vals, d_out_idx, d_count)
 * overlapping d_keys, d_mask, d_vals or another output -- with the outputs taken as min(cap, n)
 * elements long (n with MSD_COMPACT_REST), the most that can be written.  In-place operation is not
 * offered. */
int msd_compact(msd_ctx *ctx, const void *d_keys, int key_type, uint64_t n,
                const uint8_t *d_mask, uint64_t lo_bits, uint64_t hi_bits, int flags,
                const void *d_vals, int val_bytes, uint64_t cap,
                void *d_out_keys, void *d_out_vals, uint64_t *d_out_idx, uint64_t *d_count);

/* The geometry, for callers that size tests and buffers by it: that of the run-length encode
 * (msd_run_encode_limits).  *tile = the elements one workgroup takes per tile for that key width --
 * the mask-only form uses the 4-byte geometry on the mask's own 16-byte grid --, *scan_tile = how many
 * tile counts one workgroup of the tile-count scan takes at once.  Host only, no context.  Returns -1
 * for a key_bytes other than 4 or 8 or a null pointer, and leaves the outputs untouched. */
int msd_compact_limits(int key_bytes, uint64_t *tile, uint64_t *scan_tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_COMPACT_HIP_H_ */

/*
 * msd_runs_hip.h -- run-length encode: distinct keys, where each group starts, and the inverse map
 * (libinpmsdradix_hip.so; contexts and error codes come from msd_radix_hip.h).
 *
 * A RUN is a maximal stretch of consecutive elements with equal bit patterns.  The call works on any
 * array (torch.unique_consecutive); on a sorted array the runs are the groups of equal keys, which is
 * what follows a sort: group-by after msd_sort_pairs_keys, torch.unique after msd_sort_keys.
 *
 * Equality is BITWISE, the library's totalOrder convention: -0.0 and +0.0 are different values, NaNs
 * with equal sign and payload are ONE value, NaNs with different payloads are different values.  This
 * differs from torch.unique and numpy.unique, which keep every NaN apart (NaN != NaN) and merge the two
 * zeros.  Only the element width matters, 4 or 8 bytes: there is no key_type.
 *
 * How: three stream-ordered steps, no workgroup ever waits for another one.  (1) every tile counts its
 * heads -- head(i) = (i == 0) || data[i] != data[i-1] --, one word per tile; (2) the tile counts are
 * scanned in place, scan_tile words per workgroup, the piece totals by one more workgroup, whose last
 * word is the number of runs; (3) every tile is read again, finds its heads again and writes.  The
 * input is therefore read twice.
 */
#ifndef MSD_RUNS_HIP_H_
#define MSD_RUNS_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_data holds n elements of elem_bytes (4 or 8).  With m the number of runs and run(i) the 0-based
 * run that element i lies in:
 *
 *   *d_num_runs = m.  A device word, required.  Always the true count, also when m > cap: that is how
 *       a caller detects overflow.
 *   d_values (optional, cap elements of elem_bytes): d_values[j] = the value of run j, bit-exact, for
 *       j < min(m, cap).
 *   d_starts (optional, cap + 1 words): d_starts[j] = the index of the first element of run j for
 *       j < min(m, cap); d_starts[min(m, cap)] = n if m <= cap, else the start of run cap.  The count
 *       of every stored run is d_starts[j+1] - d_starts[j], the last one included.  Nothing beyond
 *       index min(m, cap) is written, in d_values or d_starts.
 *   d_inverse (optional, n words, not capped): without d_positions d_inverse[i] = run(i); with
 *       d_positions (n words, a permutation of [0, n) as msd_sort_rows or msd_sort_pairs_keys produce
 *       it, TRUSTED to be one) d_inverse[d_positions[i]] = run(i): torch's return_inverse once the
 *       array has been sorted with positions.
 *
 * n == 0: m = 0, d_starts[0] = 0 if d_starts is given, nothing else is written.  cap == 0 is legal
 * (counting only).
 *
 * Asynchronous: the launches go to the context's stream, nothing is read back and the host does not
 * wait.  Scratch: one word per tile and one per scan piece, in the context's workspace like the
 * sort's (msd_workspace_bytes shows it; a workspace that has to grow is reallocated behind a stream
 * synchronisation, as for the sort).  Phase: "run_encode".
 *
 * Pointers need only the alignment of their element type (the rule of msd_reverse and the row
 * kernels): slices of sorted arrays and top-k outputs are welcome.
 *
 * MSD_EINVAL, before any launch and touching nothing, checked in this order: a null context;
 * elem_bytes other than 4 or 8; a null d_num_runs; a null d_data with n > 0; a pointer that is not
 * aligned to its element size (d_data and d_values: elem_bytes; the others: 8); n >= 2^36;
 * d_positions without d_inverse; any output (d_values, d_starts, d_inverse, d_num_runs) overlapping
 * d_data, d_positions or another output -- with d_values and d_starts taken as min(cap, n) and
 * min(cap, n) + 1 elements long, the most that can be written.  In-place compaction is not offered. */
int msd_run_encode(msd_ctx *ctx, const void *d_data, int elem_bytes, uint64_t n, uint64_t cap,
                   void *d_values, uint64_t *d_starts, const uint64_t *d_positions,
                   uint64_t *d_inverse, uint64_t *d_num_runs);

/* The geometry, for callers that size tests and buffers by it: *tile = the elements one workgroup
 * takes per tile for that width (tiles lie on the 16-byte grid of memory: a d_data that is not 16-byte
 * aligned has a shorter first tile), *scan_tile = how many tile counts one workgroup of the tile-count
 * scan takes at once.  Host only, no context.  Returns -1 for an elem_bytes other than 4 or 8 or a
 * null pointer, and leaves the outputs untouched. */
int msd_run_encode_limits(int elem_bytes, uint64_t *tile, uint64_t *scan_tile);

#ifdef __cplusplus
}
#endif

#endif /* MSD_RUNS_HIP_H_ */

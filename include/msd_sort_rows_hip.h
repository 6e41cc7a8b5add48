/*
 * msd_sort_rows_hip.h -- per-row (batched) sort with positions: torch.sort(x, dim=-1) for every key
 * type and both directions (libinpmsdradix_hip.so; contexts, error codes and MSD_KEY_* come from
 * msd_radix_hip.h, MSD_ASCENDING / MSD_DESCENDING from msd_sort_keys_hip.h).
 *
 * Every row of a [rows, row_len] matrix is sorted on its own.  Rows inside the envelope of
 * msd_sort_rows_limits are sorted by ONE launch: a group of 64, 256 or 1024 lanes owns a row, reads it
 * once, orders it on chip and writes it once, together with the positions.  Longer rows go through
 * the segment sort (msd_sort_*_segments) between two elementwise kernels.
 *
 * Order: the one of key_type, floats in totalOrder as everywhere in this library
 *   -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN   (NaNs of one sign by payload).
 * MSD_DESCENDING is the exact reverse of MSD_ASCENDING on the codes.  Every key comes back bit-exact.
 * The order among bit-equal keys, and so among their positions, is unspecified.
 */
#ifndef MSD_SORT_ROWS_HIP_H_
#define MSD_SORT_ROWS_HIP_H_

#include "msd_sort_keys_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Row r is d_keys[r*row_stride .. r*row_stride + row_len), counts in elements, row_stride >= row_len;
 * the elements between two rows are never read.  d_out_keys[r*row_len .. (r+1)*row_len) becomes row r
 * in the order of key_type, `order` = MSD_ASCENDING or MSD_DESCENDING.  d_out_idx may be NULL;
 * otherwise it holds rows*row_len uint64 and d_out_idx[r*row_len + j] becomes a position within row r
 * whose key is bit-equal to d_out_keys[r*row_len + j]; the positions of a row are a permutation of
 * [0, row_len).
 *
 * d_out_keys == d_keys sorts in place and is allowed iff row_stride == row_len.  rows == 0 or
 * row_len == 0 is a successful no-op; rows of one key are copied, their positions are 0.
 *
 * Inside the envelope (row_len <= max_row_len of msd_sort_rows_limits) pointers need only the
 * alignment of their element type, and the row kernel's call enqueues one launch and returns: it
 * reads nothing back, uses no workspace and does not wait on the host.  Beyond it (and, under mode 0,
 * for the longer rows of 64-bit keys: below) the call goes through the segment sort and has that
 * call's host waits and workspace; it allocates no array of rows*row_len elements
 * (32-bit keys with positions are packed with their positions into d_out_idx itself and sorted there).
 *
 * MSD_EINVAL, before any launch and touching nothing: a null context (checked first); an unknown
 * key_type or order; row_stride < row_len; rows*row_stride or rows*row_len overflowing; with work to
 * do: a null d_keys or d_out_keys; a pointer that is not aligned to its element size; d_out_keys
 * overlapping the input's extent (rows-1)*row_stride + row_len in any other way than the in-place
 * case; d_out_idx overlapping the input or d_out_keys; "sort_rows_mode" 2 with row_len beyond the
 * envelope; and, wherever the call takes the segment path (beyond the envelope, or "sort_rows_mode"
 * 1), a d_out_keys or d_out_idx that is not 16-byte aligned or rows >= 2^32 -- the segment sort's own
 * rules; no staging copy is made.
 *
 * If the inner sort of the segment path fails, its error is returned and nothing more is launched:
 * the outputs then hold CODES (d_out_keys: code(key) ^ flip; 32-bit keys with positions: d_out_idx
 * holds (code ^ flip) << 32 | position and d_out_keys is untouched), not keys.
 *
 * msd_set_option: "sort_rows_mode" 0 = the library chooses: beyond the envelope the segment path;
 * inside it the row kernel for 32-bit keys, and for 64-bit keys up to 512 keys per row with
 * positions and below 4096 without -- longer rows of 64-bit keys take the segment path, which was
 * measured faster there, where its rules for the outputs hold (16-byte aligned), and the row kernel
 * where they do not: mode 0 never refuses inside the envelope what the kernel can take; 1 = always
 * the segment path, 2 = always the row kernel; "sort_rows_lanes" 0 = by the
 * shape of the matrix, 64 / 256 / 1024 = that group shape wherever the row fits it.
 * msd_stat afterwards: "sort_rows_kernel_rows" + "sort_rows_segment_rows" = rows of the last call;
 * "sort_rows_lanes" = the group shape the row kernel ran with (0: the segment path).
 * Phase: "sort_rows". */
int msd_sort_rows(msd_ctx *ctx, const void *d_keys, int key_type, uint64_t rows, uint64_t row_len,
                  uint64_t row_stride, int order, void *d_out_keys, uint64_t *d_out_idx);

/* The envelope of the row kernel: the longest row one 1024-lane workgroup holds in its registers
 * (128 per lane, no scratch) and 160 KiB of LDS:
 *   32-bit keys  24576 without positions, 16384 with
 *   64-bit keys  17408 without positions, 12288 with
 * (positions go through the keys' exchange buffer in a turn of their own and take no LDS; they take
 * a register per key).  with_idx: nonzero = d_out_idx will be given.  Host only, no context.
 * Returns -1 for an unknown key_type or a null pointer. */
int msd_sort_rows_limits(int key_type, int with_idx, uint64_t *max_row_len);

#ifdef __cplusplus
}
#endif

#endif /* MSD_SORT_ROWS_HIP_H_ */

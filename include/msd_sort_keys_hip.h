/*
 * msd_sort_keys_hip.h -- the in-place sort for every key type and both directions
 * (libinpmsdradix_hip.so; contexts, error codes and MSD_KEY_* come from msd_radix_hip.h).
 *
 * msd_sort_u32 / _u64 / _pairs_u64 order unsigned bit patterns, ascending.  The calls below order
 * the same arrays as what their key type says they hold, in either direction:
 *   MSD_KEY_U32 / U64   unsigned integers
 *   MSD_KEY_I32 / I64   two's-complement integers
 *   MSD_KEY_F32 / F64   IEEE-754 floats in totalOrder, as msd_topk_keys:
 *                       -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN
 *                       (NaNs of one sign by payload)
 *
 * How: the unsigned sort runs unchanged on the bit patterns.  Afterwards the array is
 * [keys without the sign bit, ascending][keys with it, ascending by pattern]; with P the length of
 * the first block and N = n - P, every typed order is that array with at most three ranges reversed
 * in place (R[a,b) = elements a .. b-1 reversed; a range of fewer than 2 elements is nothing):
 *
 *   key kind   MSD_ASCENDING                                   MSD_DESCENDING
 *   unsigned   nothing                                         R[0,n)
 *   signed     nothing if N == 0 or P == 0;                    R[0,P) and R[P,n)
 *              else R[0,n), then R[0,N) and R[N,n)
 *   float      nothing if N == 0; R[0,n) if P == 0;            R[0,P)
 *              else R[0,n), then R[N,n)
 *
 * No key bit is ever transformed: every key comes back bit-exact, NaN payloads and the sign of
 * zero included, and data whose signs need no reversal (non-negative floats or integers ascending)
 * are not moved again after the sort.
 *
 * Host waits: the ones of the inner sort (msd_radix_hip.h) and no other.  P is found on the device
 * (phase "sort_fixup": one search kernel, then one launch per stage of the table -- two ascending,
 * one descending -- whose workgroups leave at once where the table says "nothing"); the host never
 * reads it.  The calls return when the last kernel has been launched.
 */
#ifndef MSD_SORT_KEYS_HIP_H_
#define MSD_SORT_KEYS_HIP_H_

#include "msd_radix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MSD_ASCENDING = 0, MSD_DESCENDING = 1 };

/* Sorts the n keys at d_keys in place in the order of key_type (MSD_KEY_*), `order` = MSD_ASCENDING
 * or MSD_DESCENDING.  MSD_KEY_U32 / MSD_KEY_U64 ascending IS msd_sort_u32 / msd_sort_u64: nothing
 * else is launched.
 *
 * MSD_EINVAL, before any launch and touching nothing: a null context; an unknown key_type or order;
 * a null d_keys with n > 0; d_keys not 16-byte aligned (the sort's own rule); n >= 2^36.  n == 0 and
 * n == 1 succeed and change nothing.  If the inner sort fails the fix-up is not launched: after
 * MSD_EINTERNAL the array is as msd_radix_hip.h describes it.
 *
 * msd_stat afterwards, besides the inner sort's counters:
 *   "sort_keys_split"     P: how many keys do not have the sign bit (unsigned key types have no
 *                         sign bit: n)
 *   "sort_keys_reversed"  the sum of the lengths of the ranges this call reversed, exactly the table
 *                         above (ranges shorter than 2 elements count 0): 0 where it says "nothing"
 * Both describe the context's last msd_sort_keys / msd_sort_pairs_keys call and are unknown names
 * before the first one.  They live in device words: asking for either of these two names WAITS for
 * the context's stream and copies the word.  The sort call itself does not. */
int msd_sort_keys(msd_ctx *ctx, void *d_keys, int key_type, uint64_t n, int order);

/* The same for (key, rid) tuples in two arrays: d_rids[i] moves with d_keys[i].  64-bit key types
 * only (MSD_KEY_U64 / I64 / F64), as msd_sort_pairs_u64, and like it not stable: tuples with equal
 * keys come out in any order.  The reversal kernel runs on the rid array with the same ranges.
 * MSD_KEY_U64 ascending IS msd_sort_pairs_u64.
 *
 * MSD_EINVAL, in addition to the cases of msd_sort_keys: a 32-bit key type; a null or misaligned
 * d_rids; d_keys and d_rids overlapping. */
int msd_sort_pairs_keys(msd_ctx *ctx, void *d_keys, int key_type, uint64_t *d_rids, uint64_t n, int order);

/* Building block, in the style of msd_histogram_*: reverses the elements [first, first + count) of
 * d_data in place; elem_bytes is 4 or 8.  d_data needs only the alignment of its element type, and
 * neither end of the range needs any: nothing outside the range is read or written.  Asynchronous
 * (one launch on the context's stream, no host wait).
 *
 * MSD_EINVAL, before any launch and touching nothing: a null context; elem_bytes other than 4 or 8;
 * a null d_data with count > 0; d_data not a multiple of elem_bytes; first + count overflowing
 * (as an element count or as a byte offset).  count < 2 succeeds and changes nothing. */
int msd_reverse(msd_ctx *ctx, void *d_data, int elem_bytes, uint64_t first, uint64_t count);

#ifdef __cplusplus
}
#endif

#endif /* MSD_SORT_KEYS_HIP_H_ */

/*
 * msd_radix_hip.h -- typed, device-resident entry points of the MI355X in-place
 * MSD radix sort (libinpmsdradix_hip.so).  Plain C ABI: pointers and sizes only.
 *
 * The reference exposes one host-pointer call (include/msb_64.h:37-39) and leaks
 * its building blocks as accidental global symbols.  The
 * entry points below are the device-side counterparts of those building blocks;
 * each one names the reference function it stands in for (paths relative to
 * /root/reference).
 *
 * All d_* pointers are DEVICE pointers on the context's device.  All kernels run on the
 * context's stream.  msd_sort_* and msd_partition_* plan every round on the host from the
 * previous round's child list: they block the calling thread once per round (one small
 * device-to-host copy; two rounds for 2^30 u32 keys) and once behind the counting leaf, and
 * return when the last kernels have been launched -- the data are final once the stream has
 * drained.  The building blocks (histogram, scan, generators, sample, splitters) are fully
 * asynchronous; msd_check_* are synchronous (they return values).
 * Return value: 0 on success, a negative MSD_E* code otherwise; msd_last_error() gives the
 * message.  After MSD_EINTERNAL (an invariant check failed between two rounds: a bug) the array
 * holds a permutation of its input that is partitioned by the digits processed so far but not
 * sorted; after MSD_EINVAL / MSD_ENOMEM it is untouched.
 */
#ifndef MSD_RADIX_HIP_H_
#define MSD_RADIX_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msd_ctx msd_ctx;

enum {
	MSD_OK = 0,
	MSD_EINVAL = -1,   /* bad argument (null pointer, misaligned buffer, bad bit range) */
	MSD_ENOMEM = -2,   /* workspace allocation failed */
	MSD_EHIP = -3,     /* a HIP runtime call failed */
	MSD_EINTERNAL = -4 /* an internal invariant check failed (bug) */
};

/* ---- context ------------------------------------------------------------ */

/* Create a sorting context on `device`; `stream` is a hipStream_t (NULL = the
 * default stream).  The context owns the auxiliary workspace (block map, block
 * lists, stripe leftovers; about 12 % of the data size at 2^30 u32 keys, grown on
 * demand and reused between calls). */
int msd_create(msd_ctx **ctx, int device, void *stream);
int msd_destroy(msd_ctx *ctx);
int msd_set_stream(msd_ctx *ctx, void *stream);
void *msd_get_stream(const msd_ctx *ctx); /* the hipStream_t the context launches on */
int msd_get_device(const msd_ctx *ctx);
/* Pre-allocate the workspace for sorting n elements of key_bytes (+val_bytes)
 * so that the first timed call does not allocate. */
int msd_reserve(msd_ctx *ctx, uint64_t n, int key_bytes, int val_bytes);
uint64_t msd_workspace_bytes(const msd_ctx *ctx);
const char *msd_last_error(const msd_ctx *ctx);
const char *msd_version(void);

/* ---- the sort (reference: sort() src/msb_64.c:2261, core :2232-2244) ----- */

/* In-place MSD radix sort of n keys in device memory.  Keys must be aligned to
 * 16 bytes (the reference asserts the same, src/msb_64.c:2273-2276). */
int msd_sort_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n);
int msd_sort_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t n);
/* (key,rid) tuples in two arrays, the reference's layout (SoA, 64-bit each).
 * Unstable like the reference: equal keys may appear in any order. */
int msd_sort_pairs_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t *d_rids, uint64_t n);
/* Same, restricted to key bits [0, end_bit): bits at and above end_bit must be
 * equal in all keys (what the reference's `bits` argument of schedule_passes
 * means, src/msb_64.c:1334, :2242 passes 58). */
int msd_sort_u32_bits(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, int end_bit);
int msd_sort_u64_bits(msd_ctx *ctx, uint64_t *d_keys, uint64_t n, int end_bit);
int msd_sort_pairs_u64_bits(msd_ctx *ctx, uint64_t *d_keys, uint64_t *d_rids, uint64_t n, int end_bit);

/* ---- building blocks ----------------------------------------------------- */

/* count[(key >> shift) & (2^radix_bits - 1)]++ over n keys; d_count has
 * 2^radix_bits uint64 entries and is zeroed first; radix_bits <= 12.
 * Reference: histogram() src/msb_64.c:701-738. */
int msd_histogram_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n,
		      unsigned shift, unsigned radix_bits, uint64_t *d_count);
int msd_histogram_u64(msd_ctx *ctx, const uint64_t *d_keys, uint64_t n,
		      unsigned shift, unsigned radix_bits, uint64_t *d_count);

/* Device-wide exclusive prefix sum (single pass, decoupled look-back).
 * Reference: the bucket-offset prefix sums src/msb_64.c:747-750, 799-823 and
 * the cross-thread offset computation 1076-1082.  d_out may equal d_in.  Synchronous: the call
 * waits for the scan and returns MSD_EINTERNAL if a tile's look-back gave up (it polls a bounded
 * number of times so that a lost predecessor cannot hang the device). */
int msd_exclusive_scan_u64(msd_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint64_t n);

/* One in-place digit pass: permute keys so that they are grouped by
 * digit = (key >> shift) & (2^radix_bits - 1), buckets in ascending digit order
 * (unstable).  radix_bits <= 8.  If d_count != NULL it receives the 2^radix_bits
 * bucket sizes (uint64).  Reference: histogram + partition_ip / partition_ip_buf,
 * src/msb_64.c:1023-1027 (740-770, 785-978). */
int msd_partition_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n,
		      unsigned shift, unsigned radix_bits, uint64_t *d_count);
int msd_partition_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t n,
		      unsigned shift, unsigned radix_bits, uint64_t *d_count);
int msd_partition_pairs_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t *d_rids, uint64_t n,
			    unsigned shift, unsigned radix_bits, uint64_t *d_count);

/* ---- segmented sort and run gather: a rank of the multi-GPU sort after its exchange ----
 * The reference's nodes sort their key ranges locally after the blocks have been balanced and swapped
 * (src/msb_64.c:2200-2255: every node's buckets are whole, local_radixsort takes the remaining `bits`, :2242).
 * Here a rank receives, from every source rank, that source's buckets of the rank's key range in order (one
 * all-to-all); msd_gather_runs_* copies all those runs in ONE launch to a second buffer where every bucket is
 * contiguous (run i: `len[i]` elements from d_src + src_off[i] to d_dst + dst_off[i]; the three arrays are HOST
 * arrays; runs must not overlap in d_dst; d_dst and d_src must not overlap), and msd_sort_*_segments sorts
 * nseg independent segments [seg_off[i], seg_off[i+1]) (HOST array of nseg + 1 ascending element offsets,
 * seg_off[nseg] <= n) on their low `end_bit` bits -- all keys of a segment must agree above them -- in one
 * call: the segments are the parents of the first round, so the local sort starts where the top-digit pass
 * before the exchange left off instead of repeating it. */
int msd_sort_u32_segments(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, const uint64_t *seg_off, uint32_t nseg, int end_bit);
int msd_sort_u64_segments(msd_ctx *ctx, uint64_t *d_keys, uint64_t n, const uint64_t *seg_off, uint32_t nseg, int end_bit);
int msd_sort_pairs_u64_segments(msd_ctx *ctx, uint64_t *d_keys, uint64_t *d_rids, uint64_t n,
				const uint64_t *seg_off, uint32_t nseg, int end_bit);
int msd_gather_runs_u32(msd_ctx *ctx, uint32_t *d_dst, const uint32_t *d_src, const uint64_t *src_off,
			const uint64_t *dst_off, const uint64_t *len, uint32_t nruns);
int msd_gather_runs_u64(msd_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const uint64_t *src_off,
			const uint64_t *dst_off, const uint64_t *len, uint32_t nruns);

/* ---- fine-grained sharding: the top digits are sorted BEFORE the exchange, the open bits are counted after it ----
 * A rank of the multi-GPU sort whose keys are evenly spread orders its shard by the top 16 key bits first (two
 * direct-placement rounds -- they run at full speed there, whereas what ARRIVES after an exchange is run-structured),
 * learns the boundaries of its 2^16 buckets, sends every destination rank its range of buckets in ONE all-to-all, and
 * finishes every bucket it received -- nsrc extents, one per source rank -- with one counting pass that reads the
 * extents where they arrived and writes the sorted bucket to its place in a second buffer.  The reference's nodes do
 * the same after their block exchange: whole buckets are sorted locally on the bits that are left
 * (src/msb_64.c:2200-2255, `bits` :2242; range boundaries from the histograms :1546-1564).
 *   msd_sort_*_top: like msd_sort_*_bits, but stops once the keys are ordered by key >> begin_bit (keys that agree
 *     above begin_bit end up adjacent, in any order).  begin_bit = 0 is the full sort.
 *   msd_bucket_bounds_*: d_bounds[b] = first index i with (d_keys[i] >> shift) >= first + b, b = 0 .. nbuckets
 *     (nbuckets + 1 uint64 on the device); the keys must be ordered by key >> shift.  Asynchronous.
 *   msd_merge_buckets_u32: d_counts = nsrc x nbuckets uint64 ON THE DEVICE (row x: the lengths of source x's
 *     extents, bucket by bucket); source x's extents lie back to back in d_src from element src_base[x] on (HOST
 *     array of nsrc offsets: where the all-to-all put source x's keys).  Bucket j holds the keys whose bits above
 *     open_bits equal first_prefix + j; all its keys differ only in their low open_bits <= 16 bits.  The sorted
 *     buckets are written back to back to d_dst (n_expected = the sum of all counts <= dst_cap elements; the call
 *     fails with MSD_EINVAL and writes nothing if the counts do not add up to it).  d_src (src_cap elements) and
 *     d_dst must not overlap.  nsrc <= 8.  Blocks the calling thread until the leaf has run (one small readback:
 *     buckets it did not take -- longer than 17408 keys, more than 255 copies of one key -- are finished by the
 *     general leaves, msd_stat "merge_rejected").
 *   msd_pack_low16_u32 / msd_merge_buckets_u32_low16: once a shard is ordered by its keys' UPPER halves, the upper half of
 *     every key is the number of its bucket, which sender and receiver know from the counts: only the LOW halves need to
 *     cross the links.  msd_pack_low16_u32 writes the low 16 bits of the n keys, in order, to d_out (n uint16; no overlap
 *     with d_keys; asynchronous); msd_merge_buckets_u32_low16 is msd_merge_buckets_u32 with open_bits = 16 for extents of
 *     such low halves (d_src, src_cap and src_base in uint16 elements) and writes whole keys.  Half the exchange volume --
 *     the exchange is what bounds a step at 2 and 4 GPUs (one xGMI link per pair) -- for one more pass over the shard
 *     (6 bytes per key) before it.
 *   msd_hist2_pack_u32 / msd_merge_buckets_u32_hist2: dense buckets (2^14 keys and more per source and bucket: 2^30 keys per
 *     rank) travel as HISTOGRAMS of their low halves instead: per bucket one record of msd_hist2_record_bytes() = 17408
 *     bytes -- 2^16 2-bit counters (0, 1, 2, "3 or more") + up to 255 (value, copies) entries for the values with three or
 *     more copies -- whatever the bucket holds; a quarter of the whole keys' bytes at 2^14 keys per bucket.
 *     msd_hist2_pack_u32 writes the records of buckets 0 .. nbuckets - 1 (d_bounds: nbuckets + 1 boundaries, as from
 *     msd_bucket_bounds_u32 with shift 16) back to back to d_rec and sets *d_overflow (device; cleared first) if a bucket
 *     has more than 65535 keys or more than 255 such values -- the caller must then send the low halves themselves.
 *     Asynchronous.  msd_merge_buckets_u32_hist2: source x's records of this rank's nbuckets buckets lie at
 *     d_rec + x * nbuckets * 17408; d_counts as above (it gives the buckets' places in d_dst); the sum of the
 *     histograms of a bucket IS the sorted bucket. */
int msd_sort_u32_top(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, int end_bit, int begin_bit);
int msd_sort_u64_top(msd_ctx *ctx, uint64_t *d_keys, uint64_t n, int end_bit, int begin_bit);
int msd_sort_pairs_u64_top(msd_ctx *ctx, uint64_t *d_keys, uint64_t *d_rids, uint64_t n, int end_bit, int begin_bit);
int msd_bucket_bounds_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, unsigned shift, uint64_t first, uint32_t nbuckets, uint64_t *d_bounds);
int msd_bucket_bounds_u64(msd_ctx *ctx, const uint64_t *d_keys, uint64_t n, unsigned shift, uint64_t first, uint32_t nbuckets, uint64_t *d_bounds);
int msd_merge_buckets_u32(msd_ctx *ctx, const uint32_t *d_src, uint64_t src_cap, const uint64_t *d_counts, const uint64_t *src_base,
			  uint32_t nsrc, uint32_t nbuckets, int open_bits, uint32_t first_prefix, uint32_t *d_dst, uint64_t dst_cap,
			  uint64_t n_expected);
int msd_pack_low16_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, uint16_t *d_out);
/* msd_sort_u32_top(.., 32, 16) + msd_bucket_bounds_u32 + msd_pack_low16_u32 in one go and two passes less: ONE in-place round
 * on the top 8 bits, exact counts of all 2^16 upper halves (d_counts: 65536 uint64 on the device -- the bucket sizes the
 * exchange needs), and the low halves scattered OUT OF PLACE, bucket after bucket (bucket b from the sum of d_counts[0 .. b)
 * on, in any order inside the bucket), into d_out (n uint16, no overlap with d_keys).  d_keys is left ordered by its top 8
 * bits.  Blocks the calling thread for the in-place round; the rest is asynchronous. */
int msd_order_low16_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, uint16_t *d_out, uint64_t *d_counts);
/* ... in two halves: d_counts is complete (in stream order) after the first, so that the caller can start exchanging the
 * counts with the other ranks while the second -- the scatter, 2 ms per 2^30 keys -- runs.  The scatter must be the
 * context's next call after the counts, on the same keys (MSD_EINVAL otherwise). */
int msd_order_low16_counts_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, uint64_t *d_counts);
int msd_order_low16_scatter_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, uint16_t *d_out);
uint64_t msd_hist2_record_bytes(void);
int msd_hist2_pack_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, const uint64_t *d_bounds, uint32_t nbuckets, void *d_rec,
		       uint64_t rec_bytes, uint32_t *d_overflow);
/* ... from the LOW HALVES msd_order_low16_u32 has written (d_low: n uint16, bucket after bucket; d_bounds from its counts:
 * msd_bounds_from_counts16 writes the 65537 prefix sums of 65536 counts, asynchronously) -- half the bytes to read. */
int msd_hist2_pack_u32_low16(msd_ctx *ctx, const uint16_t *d_low, uint64_t n, const uint64_t *d_bounds, uint32_t nbuckets, void *d_rec,
			     uint64_t rec_bytes, uint32_t *d_overflow);
int msd_bounds_from_counts16(msd_ctx *ctx, const uint64_t *d_counts, uint64_t *d_bounds);
int msd_merge_buckets_u32_hist2(msd_ctx *ctx, const void *d_rec, uint64_t rec_bytes, const uint64_t *d_counts, uint32_t nsrc,
				uint32_t nbuckets, uint32_t first_prefix, uint32_t *d_dst, uint64_t dst_cap, uint64_t n_expected);
int msd_merge_buckets_u32_low16(msd_ctx *ctx, const uint16_t *d_src, uint64_t src_cap, const uint64_t *d_counts, const uint64_t *src_base,
				uint32_t nsrc, uint32_t nbuckets, uint32_t first_prefix, uint32_t *d_dst, uint64_t dst_cap, uint64_t n_expected);

/* ---- splitter service: sample -> sort (msd_sort_u32) -> delimiters -> range partition ----
 * The reference's front end for skewed keys (src/msb_64.c:1511-1564): a random sample of the
 * UNSORTED data (:1511-1521, index = mulhi(rand64, n); here a counter-based generator, seed + i),
 * the sample is sorted, equi-depth delimiters are picked with the duplicate rule of
 * extract_delimiters (:1304-1322), and the data is partitioned by the lower-bound range
 * function: range p = keys in (delim[p-1], delim[p]] (binary_search_64 :188-204, SIMD :239-351).
 * Used by the multi-GPU path on skewed keys (inplacemsdradixsort_amd/dist.py): one range per GPU.
 *   msd_sample_u32: d_sample[i] = d_keys[mulhi(splitmix64(seed + i), n)], i < m.
 *   msd_splitters_u32: d_delims[0 .. parts-2] from a SORTED sample of m keys; parts <= 256.
 *   msd_partition_by_splitters_u32: one in-place pass; afterwards range 0's keys come first, then
 *     range 1's, ... (unsorted inside a range); d_count (may be NULL) receives `parts` range sizes. */
int msd_sample_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, uint64_t m, uint64_t seed, uint32_t *d_sample);
int msd_splitters_u32(msd_ctx *ctx, const uint32_t *d_sorted_sample, uint64_t m, unsigned parts, uint32_t *d_delims);
int msd_partition_by_splitters_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, const uint32_t *d_delims,
				   unsigned parts, uint64_t *d_count);
/* the same for what the reference itself sorts: 64-bit keys, alone or with their rids (its sample, its delimiters and
 * its range function all work on 64-bit keys, src/msb_64.c:1511-1564, :1304-1322, :188-204) */
int msd_sample_u64(msd_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint64_t m, uint64_t seed, uint64_t *d_sample);
int msd_splitters_u64(msd_ctx *ctx, const uint64_t *d_sorted_sample, uint64_t m, unsigned parts, uint64_t *d_delims);
int msd_partition_by_splitters_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t n, const uint64_t *d_delims,
				   unsigned parts, uint64_t *d_count);
int msd_partition_by_splitters_pairs_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t *d_rids, uint64_t n,
					 const uint64_t *d_delims, unsigned parts, uint64_t *d_count);

/* ---- radix select and top-k (no counterpart in the reference): ORDER BY key LIMIT k, the k-th value, a percentile ----
 * With S = the input sorted ascending:
 *   msd_topk_*:   d_out[0 .. k) = S[0 .. k) (MSD_SMALLEST) or S[n-k .. n) (MSD_LARGEST), in ASCENDING order in both cases
 *     (a slice of the sorted array), keys bit-exact.  Tuples: unstable like the sort -- the out keys are that slice, every
 *     (key, rid) written is a tuple of the input, no input position is used twice; which of several tuples with the
 *     boundary key are taken is unspecified.  k == 0 is a successful no-op (n == 0 too).
 *   msd_select_*: *value (HOST memory) = S[k] (MSD_SMALLEST) or S[n-1-k] (MSD_LARGEST), k < n.  Synchronous like msd_check_*.
 * The input is read only (two passes over it for evenly spread keys: a digit histogram and a filter; one more histogram
 * pass per further digit while the bucket that holds rank k is larger than "select_cap") and NOT modified.  The output
 * must not overlap the input; inputs and outputs must be aligned to 16 bytes (the outputs are sorted with the sort).
 * k > n (top-k), k >= n (select), a null pointer, an unknown `which`, overlap or misalignment give MSD_EINVAL and touch nothing.
 * Threading as msd_sort_*: kernels on the context's stream; the call blocks the calling thread for ONE readback of the
 * search state (about 100 bytes) behind the filter pass, then for the readbacks of the internal sorts (of the candidates, if
 * only some of them belong to the answer, and of the k output elements: one per round each, none for what fits one
 * leaf), and msd_select_* for one more of the value; top-k data are final once the stream has drained.
 * Workspace (part of msd_workspace_bytes, grown on demand, reused, independent of n): the search state + one
 * 4096-bin uint64 histogram per possible pass (3 for u32, 6 for u64 keys: 96 / 192 KiB) + the candidate buffer of
 * "select_cap" elements (keys, and rids for tuples: 4 / 8 / 16 MiB at the default), next to what sorting
 * max(candidates, k) elements needs.  msd_stat afterwards: "select_hist_passes" (histogram passes over the input, a
 * first one that only found shared leading bits included), "select_skipped_bits" (leading key bits all keys share: skipped, not counted), "select_candidates"
 * (size of the final pivot bucket), "select_below" (keys written straight to the output). */
enum { MSD_SMALLEST = 0, MSD_LARGEST = 1 };
int msd_topk_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, uint64_t k, int which, uint32_t *d_out);
int msd_topk_u64(msd_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint64_t k, int which, uint64_t *d_out);
int msd_topk_pairs_u64(msd_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_rids, uint64_t n, uint64_t k, int which,
		       uint64_t *d_out_keys, uint64_t *d_out_rids);
int msd_select_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n, uint64_t k, int which, uint32_t *value);
int msd_select_u64(msd_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint64_t k, int which, uint64_t *value);

/* ---- top-k with indices, top-k and select for signed and float keys ----
 * The key type says how the bit patterns are ordered: MSD_KEY_U* as msd_topk_u*, MSD_KEY_I* as two's-complement integers,
 * MSD_KEY_F* as IEEE-754 floats in totalOrder:
 *     -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN      (NaNs of one sign: by payload)
 * Keys are returned BIT-EXACT (NaN payloads, the sign of zero).  torch.topk / torch.sort differ only for NaNs with the sign
 * bit set (torch puts every NaN on top) and in that they do not tell -0 from +0.
 * The search runs on order-preserving unsigned CODES of the keys (msd_key_encode; three more integer operations per key and
 * pass); the filter writes codes, which the library's plain unsigned sort orders, and a finishing pass over the k output
 * elements turns them back into keys (phase "select_finish").  Nothing of the sort itself is typed.
 *   msd_topk_keys: d_out_keys[0 .. k) = the k smallest / largest keys in the key type's order, ASCENDING in both cases (a slice
 *     of the sorted array, as msd_topk_*).  d_out_idx (may be NULL; k uint64): d_out_idx[j] = a position i with d_keys[i]
 *     bit-equal to d_out_keys[j]; no position twice; which of several keys equal to the boundary key are taken is
 *     unspecified.  The positions are generated by the filter pass: no rid array of n elements is read or allocated.
 *     64-bit key types: (code, position) tuples through the tuple path.  32-bit key types: ONE 64-bit element
 *     code << 32 | position per selected key, which needs n <= 2^32; d_out_idx itself is the buffer these elements are
 *     filtered to and sorted in (equal keys therefore come out with ascending positions), so the workspace stays
 *     independent of n and k: as for msd_topk_*, with a candidate buffer of 8 bytes per element for them.
 *   msd_select_key: *value (HOST memory, 4 or 8 bytes by key type) = the key of rank k from the small / large end.
 *   msd_key_encode / msd_key_decode: the codec itself; host only, no context, no device.  32-bit types: bits and code in
 *     the low 32 bits (upper bits of the argument ignored, of the result zero).
 * Arguments as msd_topk_* / msd_select_*: MSD_EINVAL, before any launch and touching nothing, for a null context or pointer,
 * k > n (top-k), k >= n (select), an unknown `which` or `key_type`, buffers not aligned to 16 bytes, overlap of any output with
 * the input or of the two outputs, and n > 2^32 with indices on a 32-bit key type.  k == 0 is a successful no-op.
 * MSD_KEY_U32 / MSD_KEY_U64 without indices ARE msd_topk_u32 / msd_topk_u64 (msd_select_u32 / _u64).  msd_stat and the phases
 * as msd_topk_*. */
enum { MSD_KEY_U32 = 0, MSD_KEY_I32 = 1, MSD_KEY_F32 = 2, MSD_KEY_U64 = 3, MSD_KEY_I64 = 4, MSD_KEY_F64 = 5 };
int msd_topk_keys(msd_ctx *ctx, const void *d_keys, int key_type, uint64_t n, uint64_t k, int which,
		  void *d_out_keys, uint64_t *d_out_idx);
int msd_select_key(msd_ctx *ctx, const void *d_keys, int key_type, uint64_t n, uint64_t k, int which, void *value);
int msd_key_encode(int key_type, uint64_t bits, uint64_t *code);
int msd_key_decode(int key_type, uint64_t code, uint64_t *bits);

/* ---- per-row (batched) top-k: torch.topk(x, k, dim=-1) for a matrix of keys ----
 * Row r is d_keys[r * row_stride .. r * row_stride + row_len) (counts in elements, row_stride >= row_len; the elements
 * between two rows are never read).  key_type and which as msd_topk_keys.
 *   d_out_keys[r * k .. r * k + k) = the k smallest / largest keys of row r, ASCENDING in both cases, bit-exact.
 *   d_out_idx (may be NULL; rows * k uint64): d_out_idx[r * k + j] = a position WITHIN ROW r whose key is bit-equal to
 *     d_out_keys[r * k + j]; no position twice within a row; which of several keys equal to the boundary key are taken is
 *     unspecified.
 * The input is read only.  rows == 0 or k == 0 is a successful no-op.  The three pointers need only the alignment of their
 * element type: rows of real matrices do not start on 16-byte boundaries.
 * Inside the envelope msd_topk_rows_limits reports (row_len <= max_row_len, k <= max_k; host only, no context) ONE kernel
 * launch answers all rows: a workgroup (long rows), or a wave of it (rows of up to 512 keys), owns a row and keeps the
 * state of the search in LDS.  The call enqueues on the context's stream and returns: no readback, no workspace.
 * Outside it, and for fewer than 4 rows of rows * 2^18 keys or more (one workgroup per row leaves the chip idle), the rows go one by one through
 * msd_topk_keys -- host-blocking as that call is; rows or output rows that are not 16-byte aligned are staged through the
 * context's workspace (one row + k output elements, grown on demand).  "topk_rows_mode" (msd_set_option) forces either way.
 * msd_stat afterwards: "topk_rows_kernel_rows" + "topk_rows_looped_rows" = rows: who produced the result.  Phase: "select_rows".
 * MSD_EINVAL, before any launch and touching nothing: null context or pointer (d_out_idx excepted), unknown which / key_type,
 * k > row_len, row_stride < row_len, a pointer not aligned to its element size, rows * row_stride or rows * k overflowing,
 * an output overlapping the input's extent ((rows - 1) * row_stride + row_len elements) or the other output, row_len > 2^32
 * with indices on a 32-bit key type, "topk_rows_mode" 2 outside the envelope.  msd_topk_rows_limits: unknown key type, null pointers. */
int msd_topk_rows(msd_ctx *ctx, const void *d_keys, int key_type, uint64_t rows, uint64_t row_len, uint64_t row_stride,
		  uint64_t k, int which, void *d_out_keys, uint64_t *d_out_idx);
int msd_topk_rows_limits(int key_type, int with_idx, uint64_t *max_row_len, uint64_t *max_k);

/* Verifier, the device form of check() (src/msb_64.c:2432-2505): counts order
 * violations (key[i] < key[i-1]) and, when d_rids != NULL, key != rid
 * mismatches; returns wrap-around sum and xor of the keys.  Synchronous (the
 * three results are written to host memory). */
int msd_check_u32(msd_ctx *ctx, const uint32_t *d_keys, uint64_t n,
		  uint64_t *violations, uint64_t *sum, uint64_t *xr);
int msd_check_u64(msd_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_rids, uint64_t n,
		  uint64_t *violations, uint64_t *sum, uint64_t *xr);

/* Synthetic inputs of SURVEY.md section 8d, generated on the device:
 * key[i] = splitmix64(seed + first + i) >> 32 (u32) or the full word (u64);
 * Zipf(theta=1): key = floor((2^32+1)^u) - 1. */
int msd_gen_uniform_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, uint64_t seed, uint64_t first);
int msd_gen_uniform_u64(msd_ctx *ctx, uint64_t *d_keys, uint64_t n, uint64_t seed, uint64_t first, int shift_right);
int msd_gen_zipf_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, uint64_t seed, uint64_t first);
int msd_gen_iota_u64(msd_ctx *ctx, uint64_t *d_vals, uint64_t n, uint64_t first);
/* duplicates: `distinct` different values with evenly spread digits, each about n / distinct times:
 * key[i] = splitmix64((splitmix64(seed + first + i) mod distinct) ^ 0xD0B1E5) >> 32 */
int msd_gen_dup_u32(msd_ctx *ctx, uint32_t *d_keys, uint64_t n, uint64_t seed, uint64_t first, uint64_t distinct);
/* the reference's own generator, MT19937-64 (src/rand.c:47-86): d_keys[i] = the i-th rand64_next() after
 * rand64_init(seed), shifted right by shift_right -- for cross-checks against a caller that fills its arrays
 * with the reference's RNG.  One workgroup walks the stream (a few GB/s); not a bulk generator. */
int msd_gen_mt19937_64(msd_ctx *ctx, uint64_t *d_keys, uint64_t n, uint64_t seed, int shift_right);

/* ---- pass planner (reference: schedule_passes(), src/msb_64.c:1334-1400) -------------
 * Host-only (no device needed).  The reference plans 1-3 leading passes of <= 9 bits
 * to reach <= 6500-tuple pieces; this planner cuts segments by <= 8-bit digits until they
 * fit the LDS leaf sorters.  Describes the FIRST round for n elements with `end_bit`
 * open key bits; later rounds depend on the data and are planned from the child counts. */
typedef struct msd_plan {
	uint32_t digit_width;      /* bits of the first digit (0: no partition round, LDS leaf only) */
	uint32_t digit_shift;      /* digit = (key >> digit_shift) & (2^digit_width - 1) */
	uint32_t block_elems;      /* elements per 256-byte block */
	uint32_t tile_elems;       /* elements per classify tile */
	uint64_t stripe_elems;     /* elements per stripe (one classify workgroup) */
	uint64_t stripes;          /* stripes of the first round */
	uint64_t leaf_capacity;    /* largest segment the LDS leaf sorter takes */
	uint32_t leaf_count_bits;  /* open bits the one-pass counting leaf can finish (0: not used) */
	uint32_t expected_rounds;  /* rounds for uniformly distributed keys */
	uint64_t workspace_bytes;  /* per-round + per-call auxiliary memory for this shape */
} msd_plan;
int msd_plan_first_round(uint64_t n, int key_bytes, int val_bytes, int end_bit, int compute_units, msd_plan *out);

/* ---- tuning knobs (no counterpart in the reference) --------------------------------
 * "direct_mode": 0 = every round classifies into the workgroup's own stripe and permutes
 *   all blocks afterwards; 1 (default) = the first round of a large input whose sampled
 *   top-digit buckets are about equally big writes its blocks straight into the bucket's
 *   estimated region and permutes only the misplaced ones; 2 = the same without the sample test.
 *   Rounds after the first follow (from exact per-parent digit counts) if the first round did.
 * "direct_min": smallest round (elements) direct placement is tried on (default 2^22).
 * "direct_min_parent": rounds after the first: smallest parent segment (default 2^17).
 * "count16": u32 keys with 16 open bits: 1 (default) = count_place16_kernel for segments of about 2^14
 *   keys, 2 = always, 0 = never (count_place_kernel).
 * "leaf17": u64 keys and tuples: 1 (default) = segments of <= 17408 elements are finished in one pass by leaf17_kernel (read
 *   once, sorted in registers and LDS, written once), 0 = tuples: register partition + the small leaves, u64 keys:
 *   leaf_count_sort_kernel (round 2).
 * "mid_leaf": u32 keys: 1 (default) = counting-leaf segments the register-resident kernels do not take (17 Ki .. 128 Ki
 *   keys, crowded ones) are finished by the 16-bit-counter leaf (merge_count_kernel) instead of count_walk_kernel; 0 = never.
 * "early_leaves": keys without payload: 1 (default) = behind a round that by its plan leaves no parent (every child has at
 *   most 16 open bits) the counting leaves are enqueued while the round's fix-up still runs -- the lists' lengths come
 *   from a copy of the counters taken behind collect_kernel -- and the round's summary travels with the leaves' counters;
 *   0 = every round ends with its own readback (A/B comparisons).  msd_stat "leaves_behind_round" counts such rounds.
 * "early_plan": 1 (default) = behind a round that is not the last the next round is planned from a copy of the counters and
 *   the first next parents taken behind collect_kernel, and enqueued while the round's fix-up still runs; the round's own
 *   summary is parked on the device and travels with the next readback.  The round ends with its own readback instead
 *   if it left no parent or more than travelled, if its next parents stay on the device or take a register-resident
 *   pass, if it carries the check behind a sampled bit skip, or if a buffer of the next round would have to grow;
 *   0 = always (A/B comparisons).  msd_stat "rounds_planned_early" counts the rounds planned this way.
 * "front_count": u32 keys, a whole-array sort whose plan is two direct 8-bit rounds: 1 (default) = the top 16 key bits are
 *   counted once before the first round (csrc/msd_front16.hpp) and ONE readback tells the host what the bit-skip sample,
 *   the first round's sample and the second round's exact count used to tell it in three; both rounds are placed from
 *   exact counts and enqueued without waiting for each other.  The sort takes the usual path, on untouched keys, if a
 *   whole leading digit is constant, if either round's children are uneven or its keys come in runs, if a 16-bit counter
 *   overflowed, or if some child of the second round is no counting leaf; 0 = never (A/B comparisons).  msd_stat
 *   "front_count_sorts" / "front_count_declined" count the sorts that took the path / counted and then declined it.
 * "front_min": smallest sort (elements) the front pass is tried on (default 2^29: at 2^28 keys it loses 0.7 %, the second
 *   round no longer starts behind a read that left a quarter of the array in the memory-side cache; tests lower it).
 * "merge_leaf": msd_merge_buckets_u32: 0 (default) = by bucket size, 1 = the register-resident leaf, 2 = the 16-bit-counter leaf.
 * "regpart": u64 keys / tuples: 1 (default) = segments of <= 17408 elements take the register-resident
 *   partition pass (csrc/msd_regpart.hpp) instead of a general round, 0 = never.
 * "select_cap": msd_topk_* / msd_select_*: capacity of the candidate buffer in elements (default 2^20, 1 .. 2^28): the
 *   search adds histogram passes until the bucket that holds rank k fits.  The 12-bit bucket of 2^30 evenly spread keys
 *   has 2^18 keys: one histogram pass; tests set it low to force the deep path on small inputs.
 * "topk_rows_mode": msd_topk_rows: 0 (default) = the library chooses between the row kernel and the loop over msd_topk_keys,
 *   1 = always the loop, 2 = always the row kernel (MSD_EINVAL outside its envelope).
 * "topk_rows_lanes": the row kernel's lanes per row: 0 (default) = by shape (a wave up to 512 keys; 256 lanes below 8192 keys
 *   and for more rows than 2 per CU of up to 1 MiB; a 1024-thread workgroup otherwise), 64 / 256 / 1024 = that shape wherever
 *   the row fits it (A/B comparisons). */
int msd_set_option(msd_ctx *ctx, const char *name, int64_t value);

/* ---- phase report (reference: description[]/times[], src/msb_64.c:2402-2412) */

/* Enable per-phase hipEvent timing for subsequent sorts on this context
 * (adds synchronisation; off by default). */
int msd_set_profiling(msd_ctx *ctx, int enabled);
/* Number of phases recorded by the last sort; names/us arrays of that length. */
int msd_phase_count(const msd_ctx *ctx);
const char *msd_phase_name(const msd_ctx *ctx, int i);
double msd_phase_us(const msd_ctx *ctx, int i);
/* Counters of the last sort: rounds of in-place partitioning, blocks moved,
 * small segments, ... (for tests and DESIGN.md tables). */
int msd_stat(const msd_ctx *ctx, const char *name, uint64_t *value);

#ifdef __cplusplus
}
#endif

#endif

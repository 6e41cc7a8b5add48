"""Every entry point that takes a context refuses a null one before it looks at anything else -- without a GPU.

Each function is called with a null context and, for every other argument, the zero value of its ctypes ``argtypes``
entry (null pointers, zero counts): a call that went past the context check would dereference one of them or reach for a
device.  The functions that return ``int`` answer MSD_EINVAL; the few getters answer the value listed in ``OTHER``."""
import pytest

MSD_EINVAL = -1

# no context among the arguments (the last four are the symbols of include/msb_64.h)
NO_CONTEXT = ["msd_create", "msd_version", "msd_key_encode", "msd_key_decode", "msd_plan_first_round", "msd_topk_rows_limits",
              "msd_hist2_record_bytes", "sort", "mamalloc", "check", "msb_64_last_error"]

# context-taking getters that do not return a status: what they answer for a null context
OTHER = {"msd_get_stream": None, "msd_get_device": -1, "msd_workspace_bytes": 0, "msd_last_error": b"null context",
         "msd_phase_count": 0, "msd_phase_name": b"", "msd_phase_us": 0.0}

# context-taking functions that return a status
STATUS = [
    "msd_destroy", "msd_set_stream", "msd_reserve",
    "msd_sort_u32", "msd_sort_u64", "msd_sort_pairs_u64", "msd_sort_u32_bits", "msd_sort_u64_bits", "msd_sort_pairs_u64_bits",
    "msd_histogram_u32", "msd_histogram_u64", "msd_exclusive_scan_u64",
    "msd_partition_u32", "msd_partition_u64", "msd_partition_pairs_u64",
    "msd_sample_u32", "msd_splitters_u32", "msd_partition_by_splitters_u32",
    "msd_sample_u64", "msd_splitters_u64", "msd_partition_by_splitters_u64", "msd_partition_by_splitters_pairs_u64",
    "msd_sort_u32_top", "msd_sort_u64_top", "msd_sort_pairs_u64_top", "msd_bucket_bounds_u32", "msd_bucket_bounds_u64",
    "msd_merge_buckets_u32", "msd_pack_low16_u32", "msd_order_low16_u32", "msd_order_low16_counts_u32", "msd_order_low16_scatter_u32",
    "msd_merge_buckets_u32_low16", "msd_hist2_pack_u32", "msd_hist2_pack_u32_low16", "msd_bounds_from_counts16",
    "msd_merge_buckets_u32_hist2",
    "msd_sort_u32_segments", "msd_sort_u64_segments", "msd_sort_pairs_u64_segments", "msd_gather_runs_u32", "msd_gather_runs_u64",
    "msd_topk_u32", "msd_topk_u64", "msd_topk_pairs_u64", "msd_select_u32", "msd_select_u64", "msd_topk_keys", "msd_select_key",
    "msd_topk_rows", "msd_check_u32", "msd_check_u64",
    "msd_gen_uniform_u32", "msd_gen_uniform_u64", "msd_gen_zipf_u32", "msd_gen_iota_u64", "msd_gen_dup_u32", "msd_gen_mt19937_64",
    "msd_set_option", "msd_set_profiling", "msd_stat",
]


def test_every_export_is_classified():
    """A new entry point has to be put into one of the lists above, or this fails."""
    from inplacemsdradixsort_amd import _lib
    lists = NO_CONTEXT + list(OTHER) + STATUS
    assert len(lists) == len(set(lists)), "a name is in two lists"
    assert sorted(lists) == sorted(_lib.EXPORTS), (sorted(set(_lib.EXPORTS) - set(lists)), sorted(set(lists) - set(_lib.EXPORTS)))
    assert len(STATUS) == 61 and len(OTHER) == 7   # (with msd_get_device, 62 of them return int)


@pytest.mark.parametrize("name", STATUS + list(OTHER))
def test_null_context_is_refused(name):
    from inplacemsdradixsort_amd import _lib
    f = getattr(_lib.load(), name)
    assert f.argtypes and f.argtypes[0] is _lib._vp, "the context comes first"
    got = f(*[t() for t in f.argtypes])
    assert got == (OTHER[name] if name in OTHER else MSD_EINVAL), (name, got)

"""The argument rules of the Python wrapper (inplacemsdradixsort_amd/api.py: MsdContext), recorded and compared.

Every case below is one call on a context without a device (``abi_support.bare_ctx()``: no library handle either) with tiny
CPU tensors.  Its outcome is one of

* ``"MsdError: <text>"``: the wrapper refused, with that message;
* ``"library"``: the call raised AttributeError for ``_L`` or ``_h``: it passed every rule of the wrapper and reached for
  the library;
* the repr of what the call returned (pure helpers such as ``_rows_layout``, ``_set_bound``, ``_bound_bits`` with a bound).

tests/golden/api_refusals.json holds the outcome of every case as the wrapper gave it BEFORE its rules were gathered in
inplacemsdradixsort_amd/_args.py; ``python tests/test_api_refusals.py --record`` writes that file and is only ever run on a
checkout of that earlier commit, never on the code under test.  The test asserts that every case still has its recorded
outcome, with one relaxation: where the record says ``library``, the refusal of tensors that are not on the context's GPU is
accepted too (a helper that prepares its pointer arguments before it fetches the export reaches that refusal first).

The cases of the ``*_limits`` wrappers and of ``_bound_bits(None)`` need the exports, not a device: they run on a bare
context that has the loaded library as ``_L`` (``lib=True``).  Cases whose name ends in ``[uint]`` use torch.uint32 /
torch.uint64 and are skipped on a torch without them.

``raise MsdError`` sites of MsdContext that no case reaches, by method, and why:

* ``__init__``: "msd_create ... failed" needs the library to refuse a device; a bare context never runs ``__init__``.
* ``_ok``: the message comes from the library's own error text after a call into it.
* ``_ptr``: "tensor must be contiguous with the expected element size" sits behind ``_on_gpu``, which a CPU tensor never
  passes.

Two sites are reached, but not through every method that leads to them: ``topk_rows`` refuses CPU keys before
``_value_index_outputs`` looks at its outputs, so the three messages of that helper are reached through ``sort_rows`` (dtype,
shape) and ``topk_typed`` (shorter than k; it sits behind an allocation on the keys' device, which a CPU tensor allows); and
in ``compact`` a bad ``lo`` or ``hi`` is only looked at behind the GPU refusal (a known quirk, pinned by the cases
``compact/bad-lo-after-cpu`` and ``bad-hi-after-cpu``), so "the bound ... is not a value of" is reached by calling
``_bound_bits`` itself.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "api_refusals.json")
GPU_REFUSAL = "MsdError: the tensors must live on the context's GPU"

NO_ORDER = ("float16", "int16", "bool", "uint8")          # dtypes without a key order
KEYED = ("float32", "int32", "float64", "int64")          # dtypes with one in every torch
UINTS = ("uint32", "uint64")                              # ... and where torch has them


def z(dt="float32", *shape):
    """zeros of dtype ``dt`` (a name): 5 elements, or ``shape``"""
    import torch
    return torch.zeros(shape or (5,), dtype=getattr(torch, dt))


def strided(dt="float32"):
    """3 elements, every second one of 6: not contiguous"""
    return z(dt, 6)[::2]


def transposed(dt="float32"):
    """3x2, the transpose of a 2x3 matrix: not contiguous"""
    return z(dt, 2, 3).t()


def pos(n=5, dt="int64"):
    return z(dt, n)


def _build_cases():
    cases = {}

    def case(name, fn, lib=False):
        assert name not in cases, name
        cases[name] = (fn, lib)

    def tag(dt):
        return " [uint]" if dt in UINTS else ""

    # ---- the helpers themselves
    case("_on_gpu/cpu", lambda c: c._on_gpu(z()))
    case("_on_gpu/none", lambda c: c._on_gpu(None))
    case("_on_gpu/nothing", lambda c: c._on_gpu())
    case("_on_gpu/none-then-cpu", lambda c: c._on_gpu(None, z("int64")))
    case("_ptr/cpu", lambda c: c._ptr(z("int32"), 4))
    case("_ptr/cpu-wrong-size", lambda c: c._ptr(z("int32"), 8))
    case("_check_positions/none", lambda c: c._check_positions(None, 5))
    case("_check_positions/good", lambda c: c._check_positions(pos(5), 5))
    case("_check_positions/int32", lambda c: c._check_positions(pos(5, "int32"), 5))
    case("_check_positions/2d", lambda c: c._check_positions(z("int64", 1, 5), 5))
    case("_check_positions/short", lambda c: c._check_positions(pos(3), 5))
    case("_check_positions/strided", lambda c: c._check_positions(strided("int64"), 3))
    case("_check_positions/what", lambda c: c._check_positions(pos(3), 5, "needles"))
    for dt in KEYED + UINTS + NO_ORDER:
        case(f"_key_type/{dt}{tag(dt)}", lambda c, dt=dt: c._key_type(z(dt)))
    case("_key_type/bfloat16", lambda c: c._key_type(z("bfloat16")))
    case("_key_type/empty-2d", lambda c: c._key_type(z("int64", 0, 3)))
    case("_set_bound/intersection", lambda c: c._set_bound("intersection", 3, 5))
    case("_set_bound/union", lambda c: c._set_bound("union", 3, 5))
    case("_set_bound/difference", lambda c: c._set_bound("difference", 3, 5))
    case("_set_bound/symmetric_difference", lambda c: c._set_bound("symmetric_difference", 3, 5))
    case("_set_bound/zero", lambda c: c._set_bound("intersection", 0, 5))
    case("_u64arr/list", lambda c: c._u64arr([0, 3, 5])._keep.tolist())

    # ---- _rows_layout
    case("_rows_layout/0-dim", lambda c: c._rows_layout(z("float32", 1).reshape(())))
    case("_rows_layout/1d-5", lambda c: c._rows_layout(z()))
    case("_rows_layout/1d-0", lambda c: c._rows_layout(z("float32", 0)))
    case("_rows_layout/1d-1", lambda c: c._rows_layout(z("float32", 1)))
    case("_rows_layout/2x3", lambda c: c._rows_layout(z("float32", 2, 3)))
    case("_rows_layout/1x3", lambda c: c._rows_layout(z("float32", 1, 3)))
    case("_rows_layout/0x3", lambda c: c._rows_layout(z("float32", 0, 3)))
    case("_rows_layout/2x3x5", lambda c: c._rows_layout(z("float32", 2, 3, 5)))
    case("_rows_layout/padded-rows", lambda c: c._rows_layout(z("float32", 2, 5)[:, :3]))
    case("_rows_layout/strided", lambda c: c._rows_layout(strided()))
    case("_rows_layout/strided-1", lambda c: c._rows_layout(z("float32", 2)[::2]))
    case("_rows_layout/transposed", lambda c: c._rows_layout(transposed()))
    case("_rows_layout/no-one-stride", lambda c: c._rows_layout(z("float32", 2, 3, 5)[:, ::2]))
    case("_rows_layout/overlap", lambda c: c._rows_layout(z("float32", 3).expand(2, 3)))

    # ---- _bound_bits with a bound given (no library needed)
    K = dict(float32=2, int32=1, float64=5, int64=4, uint32=0, uint64=3)
    for dt, bounds in (("float32", (-0.0, 0.0, 1.0, float("inf"), 7)), ("float64", (-0.0, 1, 2.5)), ("int32", (-1, 0, 5, 2.0)), ("int64", (-2, 1 << 40)),
                       ("uint32", (0, (1 << 32) - 1)), ("uint64", ((1 << 64) - 1,))):
        for b in bounds:
            for lowest in (True, False):
                case(f"_bound_bits/{dt}/{b!r}/{lowest}{tag(dt)}", lambda c, dt=dt, b=b, lowest=lowest: c._bound_bits(z(dt, 1), K[dt], b, lowest))
    for dt, bad in (("int32", (1 << 31, -(1 << 31) - 1, 1.5, "x", float("nan"))), ("int64", (1 << 63, 0.5)), ("float32", ("x", [1])), ("float64", ("y",)),
                    ("uint32", (-1, 1 << 32)), ("uint64", (-1, 1 << 64))):
        for b in bad:
            case(f"_bound_bits/{dt}/bad-{b!r}{tag(dt)}", lambda c, dt=dt, b=b: c._bound_bits(z(dt, 1), K[dt], b, True))
    for dt in KEYED:
        case(f"_bound_bits/{dt}/none-lowest", lambda c, dt=dt: c._bound_bits(z(dt, 1), K[dt], None, True), lib=True)
        case(f"_bound_bits/{dt}/none-highest", lambda c, dt=dt: c._bound_bits(z(dt, 1), K[dt], None, False), lib=True)

    # ---- the *_limits wrappers (the exports answer on the host)
    for name in ("run_encode_limits", "reduce_runs_limits", "scan_runs_limits", "compact_limits", "search_sorted_limits", "merge_sorted_limits",
                 "set_sorted_limits", "join_limits"):
        for width in (4, 8, 0, 2, 16, -4, 5):
            case(f"{name}/{width}", lambda c, name=name, width=width: getattr(c, name)(width), lib=True)
        case(f"{name}/bare", lambda c, name=name: getattr(c, name)(4))
    for name in ("topk_rows_limits", "sort_rows_limits"):
        for kt in (0, 1, 2, 3, 4, 5, 6, -1, 99):
            for idx in (False, True):
                case(f"{name}/kt{kt}/{idx}", lambda c, name=name, kt=kt, idx=idx: getattr(c, name)(kt, indices=idx), lib=True)
        for dt in KEYED + UINTS + NO_ORDER:
            case(f"{name}/{dt}{tag(dt)}", lambda c, name=name, dt=dt: getattr(c, name)(z(dt)), lib=True)
        case(f"{name}/bare", lambda c, name=name: getattr(c, name)(z("int32")))
        case(f"{name}/bare-float16", lambda c, name=name: getattr(c, name)(z("float16")))

    # ---- the untyped sort and its building blocks: the key layout (u32, u64, pairs) picks the export
    k4, k8 = (lambda: z("int32")), (lambda: z("int64"))
    case("sort_u32/accept", lambda c: c.sort_u32(k4()))
    case("sort_u64/accept", lambda c: c.sort_u64(k8()))
    case("sort_pairs_u64/accept", lambda c: c.sort_pairs_u64(k8(), k8()))
    case("sort_pairs_u64/lengths", lambda c: c.sort_pairs_u64(k8(), z("int64", 3)))
    case("sort_pairs_u64/lengths-0", lambda c: c.sort_pairs_u64(z("int64", 0), z("int64", 1)))
    layouts = (("u32", k4, None), ("u64", k8, None), ("pairs", k8, k8))
    for lname, kf, rf in layouts:
        r = (lambda rf=rf: rf() if rf else None)
        case(f"sort_top/{lname}", lambda c, kf=kf, r=r: c.sort_top(kf(), 8, rids=r()))
        case(f"sort_top/{lname}/end_bit", lambda c, kf=kf, r=r: c.sort_top(kf(), 8, 24, rids=r()))
        case(f"partition/{lname}", lambda c, kf=kf, r=r: c.partition(kf(), 0, 4, rids=r()))
        case(f"sort_segments/{lname}", lambda c, kf=kf, r=r: c.sort_segments(kf(), [0, 3, 5], 32, rids=r()))
        case(f"sort_segments/{lname}/no-segment", lambda c, kf=kf, r=r: c.sort_segments(kf(), [0], 32, rids=r()))
        case(f"sort_segments/{lname}/empty-list", lambda c, kf=kf, r=r: c.sort_segments(kf(), [], 32, rids=r()))
        case(f"partition_by_splitters/{lname}/one-part", lambda c, kf=kf, r=r: c.partition_by_splitters(kf(), None, 1, rids=r()))
        case(f"partition_by_splitters/{lname}/three-parts", lambda c, kf=kf, r=r: c.partition_by_splitters(kf(), kf()[:2], 3, rids=r()))
        case(f"topk/{lname}", lambda c, kf=kf, r=r: c.topk(kf(), 3, rids=r()))
        case(f"topk/{lname}/largest-k0", lambda c, kf=kf, r=r: c.topk(kf(), 0, largest=True, rids=r()))
        case(f"topk/{lname}/out-short", lambda c, kf=kf, r=r: c.topk(kf(), 3, rids=r(), out=kf()[:2]))
        case(f"topk/{lname}/out-given", lambda c, kf=kf, r=r: c.topk(kf(), 3, rids=r(), out=kf()))
    for lname, kf in (("u32", k4), ("u64", k8)):
        case(f"bucket_bounds/{lname}", lambda c, kf=kf: c.bucket_bounds(kf(), 16, 4))
        case(f"histogram/{lname}", lambda c, kf=kf: c.histogram(kf(), 0, 4))
        case(f"sample/{lname}", lambda c, kf=kf: c.sample(kf(), 3))
        case(f"sample_u32/{lname}", lambda c, kf=kf: c.sample_u32(kf(), 3, seed=1))
        case(f"splitters/{lname}", lambda c, kf=kf: c.splitters(kf(), 3))
        case(f"splitters/{lname}/no-part", lambda c, kf=kf: c.splitters(kf(), 0))
        case(f"splitters_u32/{lname}", lambda c, kf=kf: c.splitters_u32(kf(), 2))
        case(f"select/{lname}", lambda c, kf=kf: c.select(kf(), 2))
        case(f"select/{lname}/largest", lambda c, kf=kf: c.select(kf(), 0, largest=True))
        case(f"check/{lname}", lambda c, kf=kf: c.check(kf()))
        case(f"gather_runs/{lname}", lambda c, kf=kf: c.gather_runs(kf(), kf(), [0], [2], [3]))
        case(f"gather_runs/{lname}/no-run", lambda c, kf=kf: c.gather_runs(kf(), kf(), [], [], []))
    case("check/pairs", lambda c: c.check(k8(), rids=k8()))
    case("check/u32-rids-ignored", lambda c: c.check(k4(), rids=k8()))
    case("exclusive_scan/accept", lambda c: c.exclusive_scan(k8()))
    case("topk/rids-with-u32-keys", lambda c: c.topk(k4(), 3, rids=k8()))
    case("topk/rids-length", lambda c: c.topk(k8(), 3, rids=z("int64", 3)))
    case("topk/rids-with-u32-keys+out-short", lambda c: c.topk(k4(), 3, rids=k8(), out=z("int32", 1)))
    case("topk/rids-length+out_rids-short", lambda c: c.topk(k8(), 3, rids=z("int64", 3), out_rids=z("int64", 1)))
    case("topk/pairs/out_rids-short", lambda c: c.topk(k8(), 3, rids=k8(), out_rids=z("int64", 2)))
    case("topk/pairs/outs-given", lambda c: c.topk(k8(), 3, rids=k8(), out=k8(), out_rids=k8()))
    case("topk/u32/k-beyond-n", lambda c: c.topk(k4(), 9))
    case("topk/u32/k-negative", lambda c: c.topk(k4(), -1))
    case("gather_runs/list-lengths", lambda c: c.gather_runs(k4(), k4(), [0, 1], [2], [3]))
    case("gather_runs/list-lengths-2", lambda c: c.gather_runs(k4(), k4(), [0], [2], [3, 1]))
    case("gather_runs/element-sizes", lambda c: c.gather_runs(k4(), k8(), [0], [2], [3]))
    case("gather_runs/list-lengths+element-sizes", lambda c: c.gather_runs(k8(), k4(), [0], [2, 2], [3]))

    # ---- fine-grained sharding
    cnt = lambda: z("int64", 2, 3)
    case("merge_buckets/accept", lambda c: c.merge_buckets(k4(), cnt(), [0, 3], 16, 0, k4(), 5))
    case("merge_buckets/accept-open-bits", lambda c: c.merge_buckets(k4(), cnt(), [0, 3], 12, 0, k4(), 5))
    case("merge_buckets/accept-low16", lambda c: c.merge_buckets(z("int16"), cnt(), [0, 3], 16, 0, k4(), 5))
    case("merge_buckets/accept-hist2", lambda c: c.merge_buckets(z("uint8"), cnt(), [0, 3], 16, 0, k4(), 5))
    case("merge_buckets/bases", lambda c: c.merge_buckets(k4(), cnt(), [0], 16, 0, k4(), 5))
    case("merge_buckets/low16-open-bits", lambda c: c.merge_buckets(z("int16"), cnt(), [0, 3], 12, 0, k4(), 5))
    case("merge_buckets/hist2-open-bits", lambda c: c.merge_buckets(z("uint8"), cnt(), [0, 3], 12, 0, k4(), 5))
    case("merge_buckets/bases+low16-open-bits", lambda c: c.merge_buckets(z("int16"), cnt(), [0, 3, 4], 12, 0, k4(), 5))
    case("merge_buckets/bases+hist2-open-bits", lambda c: c.merge_buckets(z("uint8"), cnt(), [], 12, 0, k4(), 5))
    rec = lambda n=2 * 17408: z("uint8", n)
    case("hist2_pack/accept", lambda c: c.hist2_pack(k4(), z("int64", 3), rec()))
    case("hist2_pack/accept-low-halves", lambda c: c.hist2_pack(z("int16"), z("int64", 3), rec()))
    case("hist2_pack/keys-8-bytes", lambda c: c.hist2_pack(k8(), z("int64", 3), rec()))
    case("hist2_pack/rec-not-bytes", lambda c: c.hist2_pack(k4(), z("int64", 3), z("int32", 2 * 17408)))
    case("hist2_pack/rec-short", lambda c: c.hist2_pack(k4(), z("int64", 3), rec(2 * 17408 - 1)))
    case("bounds_from_counts16/accept", lambda c: c.bounds_from_counts16(z("int64", 16)))
    for name in ("order_low16", "order_low16_scatter", "pack_low16"):
        case(f"{name}/accept", lambda c, name=name: getattr(c, name)(k4(), z("int16")))
        case(f"{name}/accept-longer", lambda c, name=name: getattr(c, name)(k4(), z("int16", 6)))
        case(f"{name}/keys-8-bytes", lambda c, name=name: getattr(c, name)(k8(), z("int16")))
        case(f"{name}/out-4-bytes", lambda c, name=name: getattr(c, name)(k4(), z("int32")))
        case(f"{name}/out-short", lambda c, name=name: getattr(c, name)(k4(), z("int16", 3)))
        case(f"{name}/keys-8-bytes+out-short", lambda c, name=name: getattr(c, name)(k8(), z("int16", 3)))
    case("order_low16_counts/accept", lambda c: c.order_low16_counts(k4()))

    # ---- sort_typed, reverse
    for dt in KEYED + UINTS:
        case(f"sort_typed/{dt}{tag(dt)}", lambda c, dt=dt: c.sort_typed(z(dt)))
        case(f"sort_typed/{dt}/descending-empty{tag(dt)}", lambda c, dt=dt: c.sort_typed(z(dt, 0), descending=True))
    for dt in NO_ORDER:
        case(f"sort_typed/{dt}", lambda c, dt=dt: c.sort_typed(z(dt)))
    case("sort_typed/keys-2d", lambda c: c.sort_typed(z("float32", 2, 3)))
    case("sort_typed/keys-strided", lambda c: c.sort_typed(strided("float32")))
    case("sort_typed/rids", lambda c: c.sort_typed(z("float64"), rids=pos()))
    case("sort_typed/rids-2d", lambda c: c.sort_typed(z("int64"), rids=z("int64", 1, 5)))
    case("sort_typed/rids-32-bit-keys", lambda c: c.sort_typed(z("float32"), rids=pos()))
    case("sort_typed/rids-int32", lambda c: c.sort_typed(z("int64"), rids=pos(5, "int32")))
    case("sort_typed/rids-length", lambda c: c.sort_typed(z("int64"), rids=pos(3)))
    case("sort_typed/float16+keys-2d", lambda c: c.sort_typed(z("float16", 2, 3)))
    case("sort_typed/keys-2d+rids-32-bit-keys", lambda c: c.sort_typed(z("int32", 2, 3), rids=pos()))
    case("sort_typed/rids-32-bit-keys+rids-int32", lambda c: c.sort_typed(z("int32"), rids=pos(3, "int32")))
    case("sort_typed/rids-2d+rids-length", lambda c: c.sort_typed(z("int64"), rids=z("int64", 2, 3)))
    for dt in KEYED + ("float16", "uint8"):
        case(f"reverse/{dt}", lambda c, dt=dt: c.reverse(z(dt)))
    case("reverse/2d", lambda c: c.reverse(z("float32", 2, 3)))
    case("reverse/range", lambda c: c.reverse(z(), 1, 3))
    case("reverse/range-empty", lambda c: c.reverse(z("float32", 0)))
    case("reverse/first-negative", lambda c: c.reverse(z(), -1, 2))
    case("reverse/count-negative", lambda c: c.reverse(z(), 1, -1))
    case("reverse/past-the-end", lambda c: c.reverse(z(), 3, 3))
    case("reverse/first-past-the-end", lambda c: c.reverse(z(), 6))
    case("reverse/2d+past-the-end", lambda c: c.reverse(z("float32", 2, 3), 0, 9))
    case("reverse/float16+count-negative", lambda c: c.reverse(z("float16"), 0, -1))
    case("reverse/strided", lambda c: c.reverse(strided()))

    # ---- topk_typed, select_typed, topk_rows, sort_rows: the value and index outputs
    for dt in KEYED + UINTS + NO_ORDER:
        case(f"topk_typed/{dt}{tag(dt)}", lambda c, dt=dt: c.topk_typed(z(dt), 3))
        case(f"select_typed/{dt}{tag(dt)}", lambda c, dt=dt: c.select_typed(z(dt), 2))
        case(f"topk_rows/{dt}{tag(dt)}", lambda c, dt=dt: c.topk_rows(z(dt, 2, 3), 2))
        case(f"sort_rows/{dt}{tag(dt)}", lambda c, dt=dt: c.sort_rows(z(dt, 2, 3)))
    case("topk_typed/indices", lambda c: c.topk_typed(z(), 3, indices=True))
    case("topk_typed/outs-given", lambda c: c.topk_typed(z(), 3, out=z(), out_indices=pos()))
    case("topk_typed/out-dtype", lambda c: c.topk_typed(z(), 3, out=z("int32")))
    case("topk_typed/out_indices-dtype", lambda c: c.topk_typed(z(), 3, out_indices=pos(5, "int32")))
    case("topk_typed/out-short", lambda c: c.topk_typed(z(), 3, out=z("float32", 1)))
    case("topk_typed/out_indices-short", lambda c: c.topk_typed(z(), 3, out_indices=pos(1)))
    case("topk_typed/out-dtype+out-short", lambda c: c.topk_typed(z(), 3, out=z("int32", 1)))
    case("topk_typed/float16+out-short", lambda c: c.topk_typed(z("float16"), 3, out=z("float16", 1)))
    case("topk_typed/out-short+cpu", lambda c: c.topk_typed(z("int64"), 5, largest=True, out=z("int64", 3), out_indices=pos(5)))
    case("topk_typed/k-negative", lambda c: c.topk_typed(z(), -2))
    case("topk_typed/keys-2d", lambda c: c.topk_typed(z("float32", 2, 3), 2))
    case("select_typed/largest", lambda c: c.select_typed(z("int64"), 0, largest=True))
    case("topk_rows/1d", lambda c: c.topk_rows(z(), 2, largest=True, indices=True))
    case("topk_rows/0-dim", lambda c: c.topk_rows(z("float32", 1).reshape(()), 1))
    case("topk_rows/strided", lambda c: c.topk_rows(strided(), 1))
    case("topk_rows/transposed", lambda c: c.topk_rows(transposed(), 1))
    case("topk_rows/overlap", lambda c: c.topk_rows(z("float32", 3).expand(2, 3), 1))
    case("topk_rows/no-one-stride", lambda c: c.topk_rows(z("float32", 2, 3, 5)[:, ::2], 1))
    case("topk_rows/float16+transposed", lambda c: c.topk_rows(transposed("float16"), 1))
    case("topk_rows/transposed+out-dtype", lambda c: c.topk_rows(transposed(), 1, out=z("int32", 3, 1)))
    case("topk_rows/cpu+out-dtype", lambda c: c.topk_rows(z("float32", 2, 3), 2, out=z("int32", 2, 2)))
    case("sort_rows/1d-indices", lambda c: c.sort_rows(z(), descending=True, indices=True))
    case("sort_rows/in-place", lambda c: (lambda k: c.sort_rows(k, out=k))(z("float32", 2, 3)))
    case("sort_rows/outs-given", lambda c: c.sort_rows(z("float32", 2, 3), out=z("float32", 2, 3), out_indices=z("int64", 2, 3)))
    case("sort_rows/0-dim", lambda c: c.sort_rows(z("float32", 1).reshape(())))
    case("sort_rows/strided", lambda c: c.sort_rows(strided()))
    case("sort_rows/transposed", lambda c: c.sort_rows(transposed()))
    case("sort_rows/overlap", lambda c: c.sort_rows(z("float32", 3).expand(2, 3)))
    case("sort_rows/no-one-stride", lambda c: c.sort_rows(z("float32", 2, 3, 5)[:, ::2]))
    case("sort_rows/padded-rows", lambda c: c.sort_rows(z("float32", 2, 5)[:, :3]))
    case("sort_rows/out-dtype", lambda c: c.sort_rows(z("float32", 2, 3), out=z("int32", 2, 3)))
    case("sort_rows/out_indices-dtype", lambda c: c.sort_rows(z("float32", 2, 3), out_indices=z("int32", 2, 3)))
    case("sort_rows/out-shape", lambda c: c.sort_rows(z("float32", 2, 3), out=z("float32", 6)))
    case("sort_rows/out_indices-shape", lambda c: c.sort_rows(z("float32", 2, 3), out_indices=z("int64", 3, 2)))
    case("sort_rows/out-transposed", lambda c: c.sort_rows(z("float32", 3, 2), out=transposed()))
    case("sort_rows/out_indices-strided", lambda c: c.sort_rows(z("float32", 3), out_indices=strided("int64")))
    case("sort_rows/float16+strided", lambda c: c.sort_rows(strided("float16")))
    case("sort_rows/transposed+out-dtype", lambda c: c.sort_rows(transposed(), out=z("int32", 3, 2)))
    case("sort_rows/out-dtype+out-shape", lambda c: c.sort_rows(z("float32", 2, 3), out=z("int32", 6)))
    case("sort_rows/out-shape+cpu", lambda c: c.sort_rows(z("float32", 2, 3), indices=True, out=z("float32", 3)))

    # ---- run_encode, unique
    for dt in KEYED + UINTS + NO_ORDER:
        case(f"run_encode/{dt}{tag(dt)}", lambda c, dt=dt: c.run_encode(z(dt)))
        case(f"unique/{dt}{tag(dt)}", lambda c, dt=dt: c.unique(z(dt)))
    case("run_encode/empty", lambda c: c.run_encode(z("int32", 0)))
    case("run_encode/one", lambda c: c.run_encode(z("int32", 1), cap=0, values=False, starts=False))
    case("run_encode/cap", lambda c: c.run_encode(z(), cap=3))
    case("run_encode/inverse-positions", lambda c: c.run_encode(z(), inverse=True, positions=pos()))
    case("run_encode/2d", lambda c: c.run_encode(z("float32", 2, 3)))
    case("run_encode/strided", lambda c: c.run_encode(strided()))
    case("run_encode/transposed", lambda c: c.run_encode(transposed()))
    case("run_encode/positions-int32", lambda c: c.run_encode(z(), inverse=True, positions=pos(5, "int32")))
    case("run_encode/positions-2d", lambda c: c.run_encode(z(), inverse=True, positions=z("int64", 1, 5)))
    case("run_encode/positions-short", lambda c: c.run_encode(z(), inverse=True, positions=pos(3)))
    case("run_encode/positions-strided", lambda c: c.run_encode(z("float32", 3), inverse=True, positions=strided("int64")))
    case("run_encode/positions-without-inverse", lambda c: c.run_encode(z(), positions=pos()))
    case("run_encode/cap-negative", lambda c: c.run_encode(z(), cap=-1))
    case("run_encode/2d+float16", lambda c: c.run_encode(z("float16", 2, 3)))
    case("run_encode/float16+cap-negative", lambda c: c.run_encode(z("float16"), cap=-1))
    case("run_encode/positions-short+positions-without-inverse", lambda c: c.run_encode(z(), positions=pos(3)))
    case("run_encode/positions-without-inverse+cap-negative", lambda c: c.run_encode(z(), positions=pos(), cap=-1))
    case("run_encode/cap-negative+cpu", lambda c: c.run_encode(z("int64"), cap=-3, inverse=True))
    case("unique/inverse-counts", lambda c: c.unique(z("int64"), return_inverse=True, return_counts=True))
    case("unique/2d", lambda c: c.unique(z("float32", 2, 3)))
    case("unique/strided", lambda c: c.unique(strided()))
    case("unique/float16+2d", lambda c: c.unique(z("float16", 2, 3)))
    case("unique/empty", lambda c: c.unique(z("int32", 0)))

    # ---- reduce_runs, group_reduce, scan_runs
    for name in ("reduce_runs", "group_reduce", "scan_runs"):
        f = (lambda c, *a, name=name, **kw: getattr(c, name)(*a, **kw))
        ops = ("sum", "min", "max") + (("count",) if name == "scan_runs" else ())
        for op in ops:
            for dt in KEYED + UINTS:
                case(f"{name}/{op}/vals-{dt}{tag(dt)}", lambda c, f=f, op=op, dt=dt: f(c, z("int32"), z(dt), op=op))
        case(f"{name}/default-op", lambda c, f=f: f(c, z("int64"), z("float64")))
        case(f"{name}/empty", lambda c, f=f: f(c, z("int64", 0), z("float64", 0)))
        for op in ("mean", "count" if name != "scan_runs" else "prod", None, 0):
            case(f"{name}/op-{op!r}", lambda c, f=f, op=op: f(c, z(), z(), op=op))
        case(f"{name}/keys-2d", lambda c, f=f: f(c, z("float32", 2, 3), z()))
        case(f"{name}/vals-2d", lambda c, f=f: f(c, z(), z("float32", 1, 5)))
        case(f"{name}/keys-strided", lambda c, f=f: f(c, strided(), z("float32", 3)))
        case(f"{name}/vals-strided", lambda c, f=f: f(c, z("float32", 3), strided()))
        for dt in NO_ORDER:
            case(f"{name}/keys-{dt}", lambda c, f=f, dt=dt: f(c, z(dt), z()))
            case(f"{name}/vals-{dt}", lambda c, f=f, dt=dt: f(c, z(), z(dt)))
        case(f"{name}/lengths", lambda c, f=f: f(c, z(), z("float32", 3)))
        case(f"{name}/lengths-0", lambda c, f=f: f(c, z("float32", 1), z("float32", 0)))
        case(f"{name}/op+keys-2d", lambda c, f=f: f(c, z("float32", 2, 3), z(), op="mean"))
        case(f"{name}/keys-float16+vals-float16", lambda c, f=f: f(c, z("float16"), z("float16")))
        case(f"{name}/keys-2d+keys-float16", lambda c, f=f: f(c, z("float16", 2, 3), z()))
        case(f"{name}/vals-float16+lengths", lambda c, f=f: f(c, z(), z("float16", 3)))
        case(f"{name}/vals-strided+lengths", lambda c, f=f: f(c, z(), strided()))
    case("reduce_runs/positions", lambda c: c.reduce_runs(z(), z(), positions=pos()))
    case("reduce_runs/cap", lambda c: c.reduce_runs(z(), z(), cap=2))
    case("reduce_runs/positions-int32", lambda c: c.reduce_runs(z(), z(), positions=pos(5, "int32")))
    case("reduce_runs/positions-2d", lambda c: c.reduce_runs(z(), z(), positions=z("int64", 5, 1)))
    case("reduce_runs/positions-short", lambda c: c.reduce_runs(z(), z(), positions=pos(3)))
    case("reduce_runs/positions-strided", lambda c: c.reduce_runs(z("float32", 3), z("float32", 3), positions=strided("int64")))
    case("reduce_runs/cap-negative", lambda c: c.reduce_runs(z(), z(), cap=-1))
    case("reduce_runs/lengths+cap-negative", lambda c: c.reduce_runs(z(), z("float32", 3), cap=-1))
    case("reduce_runs/positions-short+cap-negative", lambda c: c.reduce_runs(z(), z(), positions=pos(3), cap=-1))
    case("reduce_runs/cap-negative+cpu", lambda c: c.reduce_runs(z("int64"), z("int64"), op="max", cap=-2))
    case("scan_runs/count-without-vals", lambda c: c.scan_runs(z(), None, op="count"))
    case("scan_runs/exclusive", lambda c: c.scan_runs(z(), z("int64"), exclusive=True))
    for op in ("sum", "min", "max"):
        case(f"scan_runs/{op}-without-vals", lambda c, op=op: c.scan_runs(z(), None, op=op))
    case("scan_runs/op+without-vals", lambda c: c.scan_runs(z(), None, op="mean"))
    case("scan_runs/without-vals+keys-2d", lambda c: c.scan_runs(z("float32", 2, 3), None))
    case("scan_runs/count-without-vals/keys-2d", lambda c: c.scan_runs(z("float32", 2, 3), None, op="count"))
    case("scan_runs/count-without-vals/keys-float16", lambda c: c.scan_runs(z("float16"), None, op="count"))
    case("scan_runs/count/vals-float16", lambda c: c.scan_runs(z(), z("float16"), op="count"))
    case("scan_runs/positions", lambda c: c.scan_runs(z(), z(), positions=pos()))
    case("scan_runs/positions-scatter", lambda c: c.scan_runs(z(), z(), positions=pos(), scatter=True))
    case("scan_runs/positions-short", lambda c: c.scan_runs(z(), z(), positions=pos(3)))
    case("scan_runs/positions-int32", lambda c: c.scan_runs(z(), z(), positions=pos(5, "int32")))
    case("scan_runs/positions-2d", lambda c: c.scan_runs(z(), z(), positions=z("int64", 1, 5)))
    case("scan_runs/positions-strided", lambda c: c.scan_runs(z("float32", 3), z("float32", 3), positions=strided("int64")))
    case("scan_runs/scatter-without-positions", lambda c: c.scan_runs(z(), z(), scatter=True))
    case("scan_runs/lengths+scatter-without-positions", lambda c: c.scan_runs(z(), z("float32", 3), scatter=True))
    case("scan_runs/positions-short+scatter", lambda c: c.scan_runs(z(), z(), positions=pos(3), scatter=True))

    # ---- compact and its conveniences
    mask = lambda n=5, dt="bool": z(dt, n)
    for dt in KEYED + UINTS + NO_ORDER:
        case(f"compact/keys-{dt}{tag(dt)}", lambda c, dt=dt: c.compact(z(dt)))
        case(f"compact/keys-{dt}/range{tag(dt)}", lambda c, dt=dt: c.compact(z(dt), lo=0, hi=1))
        case(f"masked_select/{dt}{tag(dt)}", lambda c, dt=dt: c.masked_select(z(dt, 2, 3), mask().new_zeros(2, 3)))
        case(f"filter_range/{dt}{tag(dt)}", lambda c, dt=dt: c.filter_range(z(dt), 0, 1))
    case("compact/nothing", lambda c: c.compact())
    case("compact/values-only", lambda c: c.compact(values=z()))
    case("compact/mask-only", lambda c: c.compact(mask=mask()))
    case("compact/mask-only-indices", lambda c: c.compact(mask=mask(5, "uint8"), indices=True))
    case("compact/mask-int8", lambda c: c.compact(z(), mask=mask(5, "int8")))
    case("compact/everything", lambda c: c.compact(z("int64"), mask=mask(), lo=0, hi=None, invert=True, rest=True, values=z("float64"), indices=True,
                                                      cap=5, out=z("int64"), out_values=z("float64", 6), out_indices=pos(7)))
    case("compact/empty", lambda c: c.compact(z("int32", 0), mask=mask(0), values=z("int64", 0)))
    case("compact/cap-0", lambda c: c.compact(z(), cap=0))
    case("compact/keys-2d", lambda c: c.compact(z("float32", 2, 3)))
    case("compact/mask-2d", lambda c: c.compact(z(), mask=z("bool", 1, 5)))
    case("compact/values-2d", lambda c: c.compact(z(), values=z("float32", 5, 1)))
    case("compact/keys-0-dim", lambda c: c.compact(z("float32", 1).reshape(())))
    case("compact/keys-strided", lambda c: c.compact(strided()))
    case("compact/mask-strided", lambda c: c.compact(z("float32", 3), mask=strided("bool")))
    case("compact/values-transposed", lambda c: c.compact(mask=mask(), values=transposed()))
    case("compact/mask-length", lambda c: c.compact(z(), mask=mask(3)))
    case("compact/values-length", lambda c: c.compact(z(), values=z("float32", 0)))
    case("compact/mask-values-length", lambda c: c.compact(mask=mask(), values=z("float32", 1)))
    for dt in ("float32", "int32", "int16", "int64"):
        case(f"compact/mask-{dt}", lambda c, dt=dt: c.compact(z(), mask=mask(5, dt)))
    for dt in ("float16", "int16", "uint8", "bool"):
        case(f"compact/values-{dt}", lambda c, dt=dt: c.compact(z(), values=z(dt)))
    for dt in ("int32", "float64"):
        case(f"compact/values-{dt}-accept", lambda c, dt=dt: c.compact(z(), values=z(dt)))
    case("compact/lo-without-keys", lambda c: c.compact(mask=mask(), lo=3))
    case("compact/hi-without-keys", lambda c: c.compact(mask=mask(), hi=3.5))
    case("compact/out-without-keys", lambda c: c.compact(mask=mask(), out=z()))
    case("compact/out_values-without-values", lambda c: c.compact(z(), out_values=z()))
    case("compact/cap-negative", lambda c: c.compact(z(), cap=-1))
    case("compact/rest-cap", lambda c: c.compact(z(), rest=True, cap=4))
    case("compact/rest-cap-equal", lambda c: c.compact(z(), rest=True, cap=5))
    case("compact/out-dtype", lambda c: c.compact(z("int32"), out=z("float32")))
    case("compact/out-short", lambda c: c.compact(z("int32"), out=z("int32", 3)))
    case("compact/out-2d", lambda c: c.compact(z("int32", 3), out=z("int32", 2, 3)))
    case("compact/out-strided", lambda c: c.compact(z("int32", 3), out=strided("int32")))
    case("compact/out-longer", lambda c: c.compact(z("int32", 3), out=z("int32", 5)))
    case("compact/out-short-but-cap", lambda c: c.compact(z("int32"), out=z("int32", 3), cap=3))
    case("compact/out_values-dtype", lambda c: c.compact(z(), values=z(), out_values=z("float64")))
    case("compact/out_values-short", lambda c: c.compact(mask=mask(), values=z(), out_values=z("float32", 1)))
    case("compact/out_indices-dtype", lambda c: c.compact(z(), out_indices=pos(5, "int32")))
    case("compact/out_indices-short", lambda c: c.compact(z(), out_indices=pos(3)))
    case("compact/out_indices-2d", lambda c: c.compact(z(), out_indices=z("int64", 5, 1)))
    case("compact/out_indices-strided", lambda c: c.compact(z("float32", 3), out_indices=strided("int64")))
    case("compact/bad-lo-after-cpu", lambda c: c.compact(z("int32"), lo="x"))
    case("compact/bad-hi-after-cpu", lambda c: c.compact(z("int32"), hi=1.5))
    case("compact/nothing+cap-negative", lambda c: c.compact(cap=-1))
    case("compact/keys-2d+mask-length", lambda c: c.compact(z("float32", 2, 3), mask=mask(3)))
    case("compact/mask-length+keys-float16", lambda c: c.compact(z("float16"), mask=mask(3)))
    case("compact/keys-float16+mask-int32", lambda c: c.compact(z("float16"), mask=mask(5, "int32")))
    case("compact/mask-int32+values-float16", lambda c: c.compact(z(), mask=mask(5, "int32"), values=z("float16")))
    case("compact/values-float16+lo-without-keys", lambda c: c.compact(mask=mask(), values=z("float16"), lo=1))
    case("compact/lo-without-keys+out-without-keys", lambda c: c.compact(mask=mask(), lo=1, out=z()))
    case("compact/out_values-without-values+cap-negative", lambda c: c.compact(z(), out_values=z(), cap=-1))
    case("compact/cap-negative+rest", lambda c: c.compact(z(), cap=-1, rest=True))
    case("compact/rest-cap+out-short", lambda c: c.compact(z(), rest=True, cap=4, out=z("float32", 1)))
    case("compact/out-short+out_values-dtype", lambda c: c.compact(z(), values=z(), out=z("float32", 1), out_values=z("int32")))
    case("compact/out_values-short+out_indices-dtype", lambda c: c.compact(z(), values=z(), out_values=z("float32", 1), out_indices=pos(5, "int32")))
    case("compact/out_indices-short+cpu", lambda c: c.compact(z(), out_indices=pos(1), lo="x"))
    case("masked_select/shapes", lambda c: c.masked_select(z(), mask(3)))
    case("masked_select/shapes-2d", lambda c: c.masked_select(z("float32", 2, 3), z("bool", 3, 2)))
    case("masked_select/t-transposed", lambda c: c.masked_select(transposed(), z("bool", 3, 2)))
    case("masked_select/mask-strided", lambda c: c.masked_select(z("float32", 3), strided("bool")))
    case("masked_select/mask-int32", lambda c: c.masked_select(z(), mask(5, "int32")))
    case("masked_select/shapes+float16", lambda c: c.masked_select(z("float16"), mask(3)))
    case("nonzero/accept", lambda c: c.nonzero(mask()))
    case("nonzero/uint8", lambda c: c.nonzero(mask(5, "uint8")))
    case("nonzero/int32", lambda c: c.nonzero(mask(5, "int32")))
    case("nonzero/2d", lambda c: c.nonzero(z("bool", 2, 3)))
    case("nonzero/strided", lambda c: c.nonzero(strided("bool")))
    case("filter_range/no-bound", lambda c: c.filter_range(z(), None, None))
    case("filter_range/no-bound+2d", lambda c: c.filter_range(z("float32", 2, 3), None, None))
    case("filter_range/lo-only", lambda c: c.filter_range(z(), 0.5, None))
    case("filter_range/values", lambda c: c.filter_range(z(), None, 1.0, values=z("int64")))
    case("filter_range/values-length", lambda c: c.filter_range(z(), None, 1.0, values=z("int64", 3)))
    case("filter_range/2d", lambda c: c.filter_range(z("float32", 2, 3), 0, 1))

    # ---- searchsorted, bucketize
    for dt in KEYED + UINTS + NO_ORDER:
        case(f"searchsorted/{dt}{tag(dt)}", lambda c, dt=dt: c.searchsorted(z(dt), z(dt, 3)))
        case(f"bucketize/{dt}{tag(dt)}", lambda c, dt=dt: c.bucketize(z(dt, 3), z(dt)))
    case("searchsorted/needles-2d", lambda c: c.searchsorted(z(), z("float32", 2, 3), right=True, needles_sorted=True))
    case("searchsorted/no-needles", lambda c: c.searchsorted(z(), z("float32", 0)))
    case("searchsorted/no-keys", lambda c: c.searchsorted(z("float32", 0), z("float32", 1)))
    case("searchsorted/sort_needles", lambda c: c.searchsorted(z(), z("float32", 3), sort_needles=True))
    case("searchsorted/positions", lambda c: c.searchsorted(z(), z("float32", 3), needles_sorted=True, positions=pos(3)))
    case("searchsorted/out", lambda c: c.searchsorted(z(), z("float32", 2, 3), out=z("int64", 2, 3)))
    case("searchsorted/dtypes", lambda c: c.searchsorted(z("float32"), z("float64", 3)))
    case("searchsorted/dtypes-int", lambda c: c.searchsorted(z("int64"), z("int32", 3)))
    case("searchsorted/keys-2d", lambda c: c.searchsorted(z("float32", 2, 3), z()))
    case("searchsorted/keys-strided", lambda c: c.searchsorted(strided(), z()))
    case("searchsorted/needles-strided", lambda c: c.searchsorted(z(), strided()))
    case("searchsorted/needles-transposed", lambda c: c.searchsorted(z(), transposed()))
    case("searchsorted/positions-short", lambda c: c.searchsorted(z(), z("float32", 3), positions=pos(5)))
    case("searchsorted/positions-int32", lambda c: c.searchsorted(z(), z("float32", 3), positions=pos(3, "int32")))
    case("searchsorted/positions-2d", lambda c: c.searchsorted(z(), z("float32", 3), positions=z("int64", 3, 1)))
    case("searchsorted/positions-strided", lambda c: c.searchsorted(z(), z("float32", 3), positions=strided("int64")))
    case("searchsorted/positions-with-sort_needles", lambda c: c.searchsorted(z(), z("float32", 3), positions=pos(3), sort_needles=True))
    case("searchsorted/out-dtype", lambda c: c.searchsorted(z(), z("float32", 3), out=z("int32", 3)))
    case("searchsorted/out-shape", lambda c: c.searchsorted(z(), z("float32", 2, 3), out=z("int64", 6)))
    case("searchsorted/out-strided", lambda c: c.searchsorted(z(), z("float32", 3), out=strided("int64")))
    case("searchsorted/float16+dtypes", lambda c: c.searchsorted(z("float16"), z("float32", 3)))
    case("searchsorted/dtypes+keys-2d", lambda c: c.searchsorted(z("float32", 2, 3), z("int32", 3)))
    case("searchsorted/keys-2d+needles-strided", lambda c: c.searchsorted(z("float32", 2, 3), strided()))
    case("searchsorted/needles-strided+positions-short", lambda c: c.searchsorted(z(), strided(), positions=pos(5)))
    case("searchsorted/positions-short+with-sort_needles", lambda c: c.searchsorted(z(), z("float32", 3), positions=pos(5), sort_needles=True))
    case("searchsorted/positions-with-sort_needles+out-dtype", lambda c: c.searchsorted(z(), z("float32", 3), positions=pos(3), sort_needles=True, out=z("int32", 3)))
    case("searchsorted/out-shape+cpu", lambda c: c.searchsorted(z("int32"), z("int32", 3), out=z("int64", 5)))
    case("bucketize/dtypes", lambda c: c.bucketize(z("int32", 3), z("int64")))
    case("bucketize/boundaries-2d", lambda c: c.bucketize(z("float32", 3), z("float32", 2, 3)))
    case("bucketize/values-2d", lambda c: c.bucketize(z("float32", 2, 3), z(), right=True))

    # ---- two sorted inputs: merge_sorted, set_sorted, the 1-D conveniences, join_groups, join
    two = {"merge_sorted": lambda c, a, b: c.merge_sorted(a, b),
           "set_sorted": lambda c, a, b: c.set_sorted(a, b, "union"),
           "join_groups": lambda c, a, b: c.join_groups(a, b),
           "join": lambda c, a, b: c.join(a, b)}
    for name in ("intersect1d", "union1d", "setdiff1d", "setxor1d"):
        two[name] = (lambda c, a, b, name=name: getattr(c, name)(a, b))
    for name, f in two.items():
        for dt in KEYED + UINTS + NO_ORDER:
            case(f"{name}/{dt}{tag(dt)}", lambda c, f=f, dt=dt: f(c, z(dt, 3), z(dt)))
        case(f"{name}/b-float16", lambda c, f=f: f(c, z(), z("float16")))
        case(f"{name}/dtypes", lambda c, f=f: f(c, z("float32"), z("float64")))
        case(f"{name}/dtypes-int", lambda c, f=f: f(c, z("int64"), z("int32")))
        case(f"{name}/a-2d", lambda c, f=f: f(c, z("float32", 2, 3), z()))
        case(f"{name}/b-2d", lambda c, f=f: f(c, z(), z("float32", 2, 3)))
        case(f"{name}/a-0-dim", lambda c, f=f: f(c, z("float32", 1).reshape(()), z()))
        case(f"{name}/a-strided", lambda c, f=f: f(c, strided(), z()))
        case(f"{name}/b-strided", lambda c, f=f: f(c, z(), strided()))
        case(f"{name}/b-transposed", lambda c, f=f: f(c, z(), transposed()))
        case(f"{name}/a-empty", lambda c, f=f: f(c, z("float32", 0), z()))
        case(f"{name}/both-empty", lambda c, f=f: f(c, z("int64", 0), z("int64", 0)))
        case(f"{name}/float16+dtypes", lambda c, f=f: f(c, z("float16"), z("float32")))
        case(f"{name}/dtypes+a-2d", lambda c, f=f: f(c, z("float32", 2, 3), z("int32")))
        case(f"{name}/a-2d+b-strided", lambda c, f=f: f(c, z("float32", 2, 3), strided()))
    v8 = lambda n=5, dt="int64": z(dt, n)
    case("merge_sorted/values", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8()))
    case("merge_sorted/values-float64", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3, "float64"), values_b=v8(5, "float64")))
    case("merge_sorted/values-uint64 [uint]", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3, "uint64"), values_b=v8(5, "uint64")))
    case("merge_sorted/origin", lambda c: c.merge_sorted(z("float32", 3), z(), origin=True))
    case("merge_sorted/outs-given", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8(), out=z("float32", 8), out_values=v8(8), out_origin=pos(8)))
    case("merge_sorted/values_a-only", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3)))
    case("merge_sorted/values_b-only", lambda c: c.merge_sorted(z("float32", 3), z(), values_b=v8()))
    case("merge_sorted/values_a-2d", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=z("int64", 3, 1), values_b=v8()))
    case("merge_sorted/values_b-2d", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=z("int64", 1, 5)))
    case("merge_sorted/values-dtypes", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8(5, "float64")))
    case("merge_sorted/values-int32", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3, "int32"), values_b=v8(5, "int32")))
    case("merge_sorted/values-float32", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3, "float32"), values_b=v8(5, "float32")))
    case("merge_sorted/values_a-length", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(5), values_b=v8()))
    case("merge_sorted/values_b-length", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8(3)))
    case("merge_sorted/out_values-without-values", lambda c: c.merge_sorted(z("float32", 3), z(), out_values=v8(8)))
    case("merge_sorted/values_a-strided", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=strided("int64"), values_b=v8()))
    case("merge_sorted/values_b-strided", lambda c: c.merge_sorted(z("float32", 3), z("float32", 3), values_a=v8(3), values_b=strided("int64")))
    case("merge_sorted/out-dtype", lambda c: c.merge_sorted(z("float32", 3), z(), out=z("int32", 8)))
    case("merge_sorted/out-shape", lambda c: c.merge_sorted(z("float32", 3), z(), out=z("float32", 9)))
    case("merge_sorted/out-2d", lambda c: c.merge_sorted(z("float32", 3), z("float32", 3), out=z("float32", 2, 3)))
    case("merge_sorted/out-strided", lambda c: c.merge_sorted(z("float32", 1), z("float32", 2), out=strided()))
    case("merge_sorted/out_values-dtype", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8(), out_values=v8(8, "float64")))
    case("merge_sorted/out_values-shape", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8(), out_values=v8(5)))
    case("merge_sorted/out_origin-dtype", lambda c: c.merge_sorted(z("float32", 3), z(), out_origin=pos(8, "int32")))
    case("merge_sorted/out_origin-shape", lambda c: c.merge_sorted(z("float32", 3), z(), out_origin=pos(3)))
    case("merge_sorted/a-2d+values_a-only", lambda c: c.merge_sorted(z("float32", 2, 3), z(), values_a=v8(3)))
    case("merge_sorted/values_a-only+out_values", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), out_values=v8(8)))
    case("merge_sorted/values_a-2d+values-dtypes", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=z("int64", 3, 1), values_b=v8(5, "float64")))
    case("merge_sorted/values-int32+values_a-length", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(5, "int32"), values_b=v8(5, "int32")))
    case("merge_sorted/values_a-length+a-strided", lambda c: c.merge_sorted(strided(), z(), values_a=v8(5), values_b=v8()))
    case("merge_sorted/out_values-without-values+b-strided", lambda c: c.merge_sorted(z(), strided(), out_values=v8(8)))
    case("merge_sorted/a-strided+out-dtype", lambda c: c.merge_sorted(strided(), z(), out=z("int32", 8)))
    case("merge_sorted/out-shape+out_origin-dtype", lambda c: c.merge_sorted(z("float32", 3), z(), out=z("float32", 9), out_origin=pos(8, "int32")))
    case("merge_sorted/out_values-shape+out_origin-shape", lambda c: c.merge_sorted(z("float32", 3), z(), values_a=v8(3), values_b=v8(), out_values=v8(5), out_origin=pos(3)))
    case("merge_sorted/out_origin-shape+cpu", lambda c: c.merge_sorted(z("int64", 3), z("int64"), origin=True, out_origin=pos(9)))
    for op in ("intersection", "union", "difference", "symmetric_difference"):
        case(f"set_sorted/{op}", lambda c, op=op: c.set_sorted(z("int32", 3), z("int32"), op))
        case(f"set_sorted/{op}/out-of-the-bound", lambda c, op=op: c.set_sorted(z("int32", 3), z("int32"), op, out=z("int32", 3)))
        case(f"set_sorted/{op}/out_origin-of-the-sum", lambda c, op=op: c.set_sorted(z("int32", 3), z("int32"), op, out_origin=pos(8)))
    for op in ("xor", "Union", None, 1):
        case(f"set_sorted/op-{op!r}", lambda c, op=op: c.set_sorted(z("int32", 3), z("int32"), op))
    case("set_sorted/origin-cap", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", origin=True, cap=2))
    case("set_sorted/cap-0-outs-given", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", cap=0, out=z("int32", 0), out_origin=pos(0)))
    case("set_sorted/cap-negative", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", cap=-1))
    case("set_sorted/out-dtype", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", out=z("float32", 8)))
    case("set_sorted/out-shape", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", cap=4, out=z("int32", 8)))
    case("set_sorted/out-strided", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", cap=3, out=strided("int32")))
    case("set_sorted/out_origin-dtype", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", out_origin=pos(8, "int32")))
    case("set_sorted/out_origin-shape", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", out_origin=z("int64", 8, 1)))
    case("set_sorted/b-strided+op", lambda c: c.set_sorted(z("int32", 3), strided("int32"), "xor"))
    case("set_sorted/op+cap-negative", lambda c: c.set_sorted(z("int32", 3), z("int32"), "xor", cap=-1))
    case("set_sorted/cap-negative+out-dtype", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", cap=-1, out=z("float32", 8)))
    case("set_sorted/out-shape+out_origin-dtype", lambda c: c.set_sorted(z("int32", 3), z("int32"), "union", out=z("int32", 3), out_origin=pos(8, "int32")))
    case("set_sorted/out_origin-shape+cpu", lambda c: c.set_sorted(z("int64", 3), z("int64"), "difference", origin=True, out_origin=pos(8)))
    case("_set1d/accept", lambda c: c._set1d(z("int32", 3), z("int32"), "union", "union1d"))
    case("_set1d/name", lambda c: c._set1d(z("int32", 2, 3), z("int32"), "union", "some name"))
    case("join_groups/cap", lambda c: c.join_groups(z("int32", 3), z("int32"), cap=1))
    case("join_groups/no-keys", lambda c: c.join_groups(z("int32", 3), z("int32"), keys=False))
    case("join_groups/cap-negative", lambda c: c.join_groups(z("int32", 3), z("int32"), cap=-1))
    case("join_groups/b-2d+cap-negative", lambda c: c.join_groups(z("int32", 3), z("int32", 2, 3), cap=-1))
    case("join_groups/a-strided+cap-negative", lambda c: c.join_groups(strided("int32"), z("int32"), cap=-1))
    case("join_groups/cap-negative+cpu", lambda c: c.join_groups(z("int64", 3), z("int64", 1), cap=-5, keys=False))

    # ---- join_pairs
    def groups(gcap=3, num=None, dt="int64", bad=None, keys=True):
        four = [z(dt, gcap) for _ in range(4)]
        if bad is not None:
            four[bad[0]] = bad[1]
        return (z("int64", 1) if num is None else num, z("int32", gcap) if keys else None, *four)
    jp = lambda c, g=None, n=3, m=5, cap=4, **kw: c.join_pairs(groups() if g is None else g, n, m, cap, **kw)
    case("join_pairs/accept", lambda c: jp(c))
    case("join_pairs/count-only", lambda c: jp(c, groups(keys=False), cap=0))
    case("join_pairs/no-groups", lambda c: jp(c, groups(0), n=0, m=0, cap=0))
    case("join_pairs/positions", lambda c: jp(c, positions_a=pos(3), positions_b=pos(5)))
    case("join_pairs/outs-given", lambda c: jp(c, out_a=pos(4), out_b=pos(4)))
    case("join_pairs/n-negative", lambda c: jp(c, n=-1))
    case("join_pairs/m-negative", lambda c: jp(c, m=-1))
    case("join_pairs/cap-negative", lambda c: jp(c, cap=-1))
    case("join_pairs/num_groups-int32", lambda c: jp(c, groups(num=z("int32", 1))))
    case("join_pairs/num_groups-two", lambda c: jp(c, groups(num=z("int64", 2))))
    case("join_pairs/num_groups-0-dim", lambda c: jp(c, groups(num=z("int64", 1).reshape(()))))
    case("join_pairs/groups-int32", lambda c: jp(c, groups(dt="int32")))
    case("join_pairs/groups-one-int32", lambda c: jp(c, groups(bad=(2, z("int32", 3)))))
    case("join_pairs/groups-one-2d", lambda c: jp(c, groups(bad=(1, z("int64", 3, 1)))))
    case("join_pairs/groups-one-short", lambda c: jp(c, groups(bad=(3, z("int64", 1)))))
    case("join_pairs/groups-first-longer", lambda c: jp(c, groups(bad=(0, z("int64", 5)))))
    case("join_pairs/groups-one-strided", lambda c: jp(c, groups(bad=(1, strided("int64")))))
    case("join_pairs/positions_a-int32", lambda c: jp(c, positions_a=pos(3, "int32")))
    case("join_pairs/positions_a-length", lambda c: jp(c, positions_a=pos(5)))
    case("join_pairs/positions_a-2d", lambda c: jp(c, positions_a=z("int64", 3, 1)))
    case("join_pairs/positions_a-strided", lambda c: jp(c, positions_a=strided("int64")))
    case("join_pairs/positions_b-int32", lambda c: jp(c, positions_b=pos(5, "int32")))
    case("join_pairs/positions_b-length", lambda c: jp(c, positions_b=pos(3)))
    case("join_pairs/positions_b-2d", lambda c: jp(c, positions_b=z("int64", 1, 5)))
    case("join_pairs/positions_b-strided", lambda c: jp(c, m=3, positions_b=strided("int64")))
    case("join_pairs/out_a-dtype", lambda c: jp(c, out_a=pos(4, "int32")))
    case("join_pairs/out_a-shape", lambda c: jp(c, out_a=pos(5)))
    case("join_pairs/out_a-strided", lambda c: jp(c, cap=3, out_a=strided("int64")))
    case("join_pairs/out_b-dtype", lambda c: jp(c, out_b=pos(4, "float64")))
    case("join_pairs/out_b-shape", lambda c: jp(c, out_b=z("int64", 2, 2)))
    case("join_pairs/cap-negative+num_groups-int32", lambda c: jp(c, groups(num=z("int32", 1)), cap=-1))
    case("join_pairs/num_groups-two+groups-int32", lambda c: jp(c, groups(num=z("int64", 2), dt="int32")))
    case("join_pairs/groups-one-short+positions_a-length", lambda c: jp(c, groups(bad=(3, z("int64", 1))), positions_a=pos(5)))
    case("join_pairs/positions_a-length+positions_b-length", lambda c: jp(c, positions_a=pos(5), positions_b=pos(3)))
    case("join_pairs/positions_b-length+out_a-shape", lambda c: jp(c, positions_b=pos(3), out_a=pos(5)))
    case("join_pairs/out_a-shape+out_b-dtype", lambda c: jp(c, out_a=pos(5), out_b=pos(4, "int32")))
    case("join_pairs/out_b-shape+cpu", lambda c: jp(c, out_b=pos(5)))

    # ---- calls without a rule of their own: they reach for the library
    case("reserve/accept", lambda c: c.reserve(5, 4))
    case("workspace_bytes/accept", lambda c: c.workspace_bytes)
    for name in ("gen_uniform_u32", "gen_zipf_u32"):
        case(f"{name}/accept", lambda c, name=name: getattr(c, name)(k4()))
    for name in ("gen_uniform_u64", "gen_iota_u64"):
        case(f"{name}/accept", lambda c, name=name: getattr(c, name)(k8()))
    case("gen_dup_u32/accept", lambda c: c.gen_dup_u32(k4(), 3))
    case("gen_mt19937_64/accept", lambda c: c.gen_mt19937_64(k8(), 7))
    case("set_option/accept", lambda c: c.set_option("direct_mode", 1))
    case("set_profiling/accept", lambda c: c.set_profiling(True))
    case("phases/accept", lambda c: c.phases())
    case("stats/accept", lambda c: c.stats())
    case("close/accept", lambda c: c.close())
    return cases


CASES = _build_cases()


def outcome(name):
    """the outcome of case ``name`` on a fresh bare context, as the record spells it"""
    import abi_support as A
    from inplacemsdradixsort_amd import MsdError
    fn, lib = CASES[name]
    ctx = A.bare_ctx()
    if lib:
        from inplacemsdradixsort_amd import _lib
        ctx._L = _lib.load()
    try:
        got = fn(ctx)
    except MsdError as e:
        return "MsdError: " + str(e)
    except AttributeError as e:
        if "object has no attribute '_L'" in str(e) or "object has no attribute '_h'" in str(e):
            return "library"
        raise
    return repr(got)


def _skipped(name):
    import torch
    return name.endswith("[uint]") and not hasattr(torch, "uint64")


def _record():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_outcome_is_the_recorded_one(name):
    if _skipped(name):
        pytest.skip("this torch has no uint32 / uint64")
    want = _record()[name]
    got = outcome(name)
    assert got == want or (want == "library" and got == GPU_REFUSAL), (name, got, want)


def test_the_record_has_no_case_that_the_test_lost():
    assert set(_record()) <= set(CASES)
    assert all(name in _record() or name.endswith("[uint]") for name in CASES)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_api_refusals.py --record   (on a checkout of the commit the record is taken from)")
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    record = {name: outcome(name) for name in sorted(CASES) if not _skipped(name)}
    with open(GOLDEN, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(record)} cases into {GOLDEN}")

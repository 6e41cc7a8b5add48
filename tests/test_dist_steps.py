"""The sharded front ends make the same engine calls and the same collectives, in the same order, as the traces
recorded in tests/golden/dist_steps.json (``python tests/golden/make_golden.py dist_steps`` writes that file from the
code as it stands).  One rank, in process: a recording proxy around the numpy stand-in engine and a one-rank
stand-in for ``torch.distributed``; ``_force_exchange`` sends the single rank through the whole exchange.

Where histogram records are wanted the engine's ``hist2_pack`` and ``merge_buckets`` only log (really packing 2^16
records in numpy takes 19 s): those cases assert the trace alone, the records' results are covered by
test_dist_gloo.test_histogram_exchange_over_gloo.  Every other case also checks that the output is the sorted input.

One trace was recorded BEFORE the one-shot adopted the rule "records need room in the receive buffer too" and is
kept under the key ``oneshot/fine/recv_small@before``: there the one-shot packed 2^16 records it could never send
(``order_low16``, ``bounds_from_counts16``, ``hist2_pack``) and then sent low halves.  Now it prepares low halves
only, exactly as with ``FINE_HIST = False`` in the same buffers -- the collectives are the same in both."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dist_gloo import NumpyEngine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dist_steps.json")
BEFORE = "oneshot/fine/recv_small@before"
N = 5000
REC_TOTAL = 65536 * 17408                            # bytes of a shard's 2^16 histogram records
SMALL = N + 8                                        # what arrives plus the leaf's 16-byte vector
NREC = REC_TOTAL // 4                                # int32 elements that hold exactly the records
BOTH = ((2 * N + 255) // 256 * 256 + REC_TOTAL) // 4  # ... the low halves and, behind them at a 256-byte boundary, the records

# name: (module globals to set, work elements, receive elements, "records are wanted": the stub engine, trace only)
CONFIGS = {
    "defaults": ({}, SMALL, SMALL, False),
    "whole_keys": ({"FINE_LOW16": False}, SMALL, SMALL, False),
    "records": ({"FINE_HIST_MIN_KEYS": 0}, BOTH, NREC, True),
    "records_overlap": ({"FINE_HIST_MIN_KEYS": 0}, NREC, NREC, True),
    "records_whole_keys": ({"FINE_HIST_MIN_KEYS": 0, "FINE_LOW16": False}, BOTH, NREC, True),
    "recv_small": ({"FINE_HIST_MIN_KEYS": 0}, BOTH, SMALL, True),
    "recv_small_no_hist": ({"FINE_HIST_MIN_KEYS": 0, "FINE_HIST": False}, BOTH, SMALL, False),
    "no_hist": ({"FINE_HIST_MIN_KEYS": 0, "FINE_HIST": False}, BOTH, NREC, False),
    "pieces": ({"A2A_MAX_BYTES": 4096}, SMALL, SMALL, False),
}


def _desc(x):
    if isinstance(x, torch.Tensor):
        return f"{str(x.dtype).replace('torch.', '')}[{x.numel()}]"
    if isinstance(x, (list, tuple)):
        if len(x) <= 8:
            return [_desc(v) for v in x]
        return f"list[{len(x)}] sum={int(sum(int(v) for v in x))}" if all(isinstance(v, (int, np.integer)) for v in x) else f"list[{len(x)}]"
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, (np.integer,)):
        return int(x)
    return "callable" if callable(x) else type(x).__name__


class Recording:
    """Every engine method called, with each tensor argument's dtype and length and each scalar."""

    def __init__(self, engine, log):
        self._e, self._log = engine, log

    def __getattr__(self, name):
        fn = getattr(self._e, name)      # (AttributeError where the engine has no such method: the product asks with hasattr)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            self._log.append(["engine", name, [_desc(v) for v in a], {k: _desc(kw[k]) for k in sorted(kw)}])
            return fn(*a, **kw)
        return call


class LoggingRecords(NumpyEngine):
    """hist2_pack and merge_buckets are only logged (module docstring)."""

    def hist2_pack(self, keys, bounds, rec):
        return torch.zeros(1, dtype=torch.int32)     # no record overflowed

    def merge_buckets(self, src, counts, src_base, open_bits, first_prefix, dst, n_expected):
        pass


class OneRank:
    """torch.distributed for one rank: every collective is logged with its dtype and split sizes."""

    def __init__(self, log, copy):
        self._log, self._copy = log, copy

    def get_rank(self, group=None):
        return 0

    def all_gather(self, outs, t, group=None):
        self._log.append(["dist", "all_gather", _desc(t), len(outs)])
        outs[0].copy_(t)

    def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None, group=None):
        self._log.append(["dist", "all_to_all_single", _desc(input), _desc(input_split_sizes), _desc(output), _desc(output_split_sizes)])
        if self._copy:
            output[:sum(output_split_sizes)].copy_(input[:sum(input_split_sizes)])

    def all_to_all(self, outs, ins, group=None):
        self._log.append(["dist", "all_to_all", [_desc(x) for x in ins], [_desc(x) for x in outs]])
        for o, i in zip(outs, ins):
            if self._copy:
                o.copy_(i)


class OneRankAsync(OneRank):
    """... whose collectives take ``async_op`` and return a handle, like the real backends'."""

    class _Handle:
        def __init__(self, log, what):
            self._log, self._what = log, what

        def wait(self):
            self._log.append(["dist", "wait", self._what])

    def all_gather(self, outs, t, group=None, async_op=False):
        super().all_gather(outs, t, group)
        self._log[-1].append({"async_op": async_op})
        return self._Handle(self._log, "all_gather") if async_op else None

    def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None, group=None, async_op=False):
        super().all_to_all_single(output, input, output_split_sizes, input_split_sizes, group)
        self._log[-1].append({"async_op": async_op})
        return self._Handle(self._log, "all_to_all_single") if async_op else None

    def all_to_all(self, outs, ins, group=None, async_op=False):
        super().all_to_all(outs, ins, group)
        self._log[-1].append({"async_op": async_op})
        return self._Handle(self._log, "all_to_all") if async_op else None


def _keys(seed, dtype=np.uint32):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, np.iinfo(dtype).max, size=N, dtype=dtype, endpoint=True)
    return k, torch.from_numpy(k.view(np.int32 if dtype == np.uint32 else np.int64).copy())


def _u32_case(front, scheme, config, have_work=True, async_dist=False):
    """The trace of one u32 case; the outputs are checked where the engine is the real stand-in."""
    import inplacemsdradixsort_amd.dist as D
    sets, work_n, recv_n, stub = CONFIGS[config]
    stub = stub and scheme == "fine"
    log = []
    eng = Recording(LoggingRecords() if stub else NumpyEngine(), log)
    dd = (OneRankAsync if async_dist else OneRank)(log, copy=not stub)
    old = {k: getattr(D, k) for k in sets}
    try:
        for k, v in sets.items():
            setattr(D, k, v)
        if front == "oneshot":
            k, t = _keys(1)
            work = torch.empty(work_n, dtype=torch.int32) if have_work else None
            out = D.sort_sharded_u32(eng, t, torch.empty(recv_n, dtype=torch.int32), dd, 1, work=work, scheme=scheme, _force_exchange=True)
            pairs = [(k, out)]
        else:
            recv = [torch.empty(recv_n, dtype=torch.int32) for _ in range(2)]
            work = [torch.empty(work_n, dtype=torch.int32) for _ in range(2)] if have_work else None
            sorter = D.ShardedSorter(eng, dd, 1, recv, work_bufs=work, scheme=scheme, _force_exchange=True)
            shards, pairs = [_keys(10 + s) for s in range(3)], []
            for s in range(3):        # the order bench.py uses: submit shard s, then finish shard s-1
                sorter.submit(shards[s][1])
                log.append(["sorter", "last_format", sorter.last_format])
                if s:
                    pairs.append((shards[s - 1][0], sorter.collect().clone()))
            pairs.append((shards[2][0], sorter.collect().clone()))
            assert sorter.pending() == 0
    finally:
        for k, v in old.items():
            setattr(D, k, v)
    if not stub:
        for k, out in pairs:
            assert (out.numpy().view(np.uint32) == np.sort(k)).all()
    return log


def _wide_case(name):
    """u64 keys, tuples and the sampled variants at one rank: their local shortcut, pinned."""
    import inplacemsdradixsort_amd.dist as D
    log = []
    eng, dd = Recording(NumpyEngine(), log), OneRank(log, copy=True)
    if name.startswith("u32"):
        k, t = _keys(3)
        out = D.sort_sharded_u32_sampled(eng, t, torch.empty(SMALL, dtype=torch.int32), dd, 1)
        assert (out.numpy().view(np.uint32) == np.sort(k)).all()
        return log
    k, t = _keys(4, np.uint64)
    recv = torch.empty(SMALL, dtype=torch.int64)
    if "pairs" in name:
        rids = torch.from_numpy((k ^ np.uint64(0x5A5A5A5A5A5A5A5A)).view(np.int64).copy())
        fn = D.sort_sharded_pairs_u64_sampled if name.endswith("sampled") else D.sort_sharded_pairs_u64
        out, out_r = fn(eng, t, rids, recv, torch.empty(SMALL, dtype=torch.int64), dd, 1)
        assert (out_r.numpy().view(np.uint64) == (out.numpy().view(np.uint64) ^ np.uint64(0x5A5A5A5A5A5A5A5A))).all()
    else:
        out = (D.sort_sharded_u64_sampled if name.endswith("sampled") else D.sort_sharded_u64)(eng, t, recv, dd, 1)
    assert (out.numpy().view(np.uint64) == np.sort(k)).all()
    return log


CASES = {}
for _front in ("oneshot", "sorter"):
    for _scheme in ("fine", "coarse"):
        for _config in CONFIGS:
            CASES[f"{_front}/{_scheme}/{_config}"] = (_u32_case, (_front, _scheme, _config))
        # (collectives that take async_op: the work under the count all-gather, the handles the sorter waits for)
        CASES[f"{_front}/{_scheme}/defaults/async"] = (_u32_case, (_front, _scheme, "defaults", True, True))
    CASES[f"{_front}/coarse/no_work"] = (_u32_case, (_front, "coarse", "defaults", False))
    CASES[f"{_front}/chosen/defaults"] = (_u32_case, (_front, None, "defaults"))       # (use_fine: a small shard goes coarse)
for _name in ("u64", "pairs_u64", "u32_sampled", "u64_sampled", "pairs_u64_sampled"):
    CASES[f"wide/{_name}"] = (_wide_case, (_name,))


def record_all():
    return {name: fn(*args) for name, (fn, args) in CASES.items()}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_same_calls_in_the_same_order(case):
    fn, args = CASES[case]
    got = json.loads(json.dumps(fn(*args)))      # (tuples become lists, as in the file)
    want = _golden()[case]
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)


def test_the_one_intended_difference_is_the_packing():
    """Module docstring: with a receive buffer too small for the records the one-shot no longer packs them."""
    g = _golden()
    before, now = g[BEFORE], g["oneshot/fine/recv_small"]
    names = lambda t: [e[1] for e in t if e[0] == "engine"]           # noqa: E731
    assert {"order_low16", "bounds_from_counts16", "hist2_pack"} <= set(names(before))
    assert not {"bounds_from_counts16", "hist2_pack"} & set(names(now))
    assert [e for e in before if e[0] == "dist"] == [e for e in now if e[0] == "dist"]
    assert now == g["oneshot/fine/recv_small_no_hist"]
    assert names(before)[3:] == names(now)[2:]                        # after the preparation: the same leaf

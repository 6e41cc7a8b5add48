"""Multi-GPU range partition + one all-to-all.

One process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI).  Rank g
holds a shard of keys in HBM.  Like the reference's NUMA phase -- contiguous key
ranges per node (numa_dest, src/msb_64.c:1596-1607), blocks balanced across nodes
(:1952-1997), then purely local sorting (:2200-2255) -- the distributed sort is:

  1. one in-place partition pass on every rank: buckets end up contiguous in
     ascending order, so the slice for destination rank d is already packed for sending.
     Uniform keys: the top digit (``engine.partition``), destination = top log2(G) bits.
     Skewed keys: sampled splitters (``sort_sharded_u32_sampled``), destination = range.
  2. the G x G send matrix is all-gathered (every rank learns every rank's total, so a
     receive buffer that is too small fails on ALL ranks, not on one) and ONE
     all-to-all(v) moves the keys;
  3. each rank sorts what it received; with the radix split all its keys share the top
     log2(G) bits, which are passed on as ``end_bit`` (the reference passes bits=58 after
     its 6-bit split, src/msb_64.c:2242).

Large evenly spread shards (>= 2^27 keys per rank, with a second buffer) take the FINE scheme instead: the shard is
ordered by its top 16 bits BEFORE the exchange (``engine.sort_top`` -- two direct-placement rounds, which run at full
speed on a rank's own uniform keys, whereas what ARRIVES after an exchange is run-structured), the 65536 bucket counts
are all-gathered, the one all-to-all moves every rank's range of buckets, and ``engine.merge_buckets`` finishes every
bucket -- ``world`` extents, one per source -- with one counting pass that reads the extents where they arrived and
writes the sorted bucket to its place in the second buffer: no gather pass, no run-structured round, 7.5-8.5 ms of
local work per 2^30-key step at 8, 4 and 2 ranks instead of 10.9-11.5 (tools/multigpu_local_work.py).

u64 keys and (u64 key, u64 rid) tuples -- what the reference's ``sort()`` takes, one pair of arrays per memory node --
shard the same way (``sort_sharded_u64``, ``sort_sharded_pairs_u64``).
``engine`` is an :class:`inplacemsdradixsort_amd.MsdContext`; the CPU gloo tests pass a
stand-in with the same methods to exercise the exchange logic without a GPU.
The receive buffer needs slack over n/G under skew (the reference's ``fudge``).
"""
from __future__ import annotations


class ReceiveOverflow(RuntimeError):
    """Some rank's receive buffer cannot take its range; raised on EVERY rank (the decision is made
    from the all-gathered send matrix, before the data exchange, so no rank is left in a collective)."""


class HostStagedDist:
    """torch.distributed's collectives for CUDA tensors over a CPU-only backend (gloo): every tensor is staged
    through host memory.  For rehearsing the multi-rank code paths where RCCL cannot run -- several ranks sharing
    one GPU (tests/test_gpu_dist.py, ``bench.py --backend gloo``); the real runs use backend "nccl" directly."""

    def __init__(self, dist):
        self._d = dist

    def get_rank(self, group=None):
        return self._d.get_rank(group) if group is not None else self._d.get_rank()

    def barrier(self, group=None):
        self._d.barrier(group=group)

    def all_gather(self, outs, t, group=None):
        import torch
        tmp = [torch.empty(o.shape, dtype=o.dtype) for o in outs]
        self._d.all_gather(tmp, t.cpu(), group=group)
        for o, x in zip(outs, tmp):
            o.copy_(x)

    def all_reduce(self, t, op=None, group=None):
        h = t.cpu()
        self._d.all_reduce(h, op=op if op is not None else self._d.ReduceOp.SUM, group=group)
        t.copy_(h)

    def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None, group=None):
        import torch
        o = torch.empty(output.shape, dtype=output.dtype)
        self._d.all_to_all_single(o, input.cpu(), output_split_sizes=output_split_sizes,
                                  input_split_sizes=input_split_sizes, group=group)
        output.copy_(o)

    def all_to_all(self, outs, ins, group=None):
        import torch
        o = torch.empty(sum(x.numel() for x in outs), dtype=outs[0].dtype)
        self._d.all_to_all_single(o, torch.cat([x.reshape(-1) for x in ins]).cpu(), output_split_sizes=[x.numel() for x in outs],
                                  input_split_sizes=[x.numel() for x in ins], group=group)
        at = 0
        for x in outs:
            x.copy_(o[at:at + x.numel()])
            at += x.numel()

    def __getattr__(self, name):   # ReduceOp, get_world_size, ...
        return getattr(self._d, name)


# RCCL 2.26 (the build ROCm 7 / torch 2.10 ship) moves only HALF of a single send / receive of >= 2 GiB -- silently: a
# one-rank all_to_all_single of 2^29 int32 comes back with its second GiB untouched (tools/debug/a2a_big.py, measured on
# the GPU box in round 3; the same through ncclSend / ncclRecv directly).  At 2^30 keys per rank a pair's block is 2 GiB at
# 2 ranks, 1 GiB at 4, 512 MiB at 8.  Every exchange therefore goes in pieces of at most this many bytes per pair.
A2A_MAX_BYTES = 1 << 29


class _Splits(list):
    """Split sizes of one rank + the largest block any PAIR of ranks exchanges (every rank must run the same number of
    exchange rounds)."""
    max_block = 0


def all_to_all_v(dist, out, inp, got_l, send_l, group=None, async_op: bool = False):
    """``out`` <- all-to-all(v) of ``inp`` with the given split sizes, in rounds of at most A2A_MAX_BYTES per pair (one
    ``all_to_all_single`` when every block is small).  Returns the list of Work handles (``async_op``) or []."""
    if inp.element_size() == 2:   # (neither RCCL nor gloo moves 16-bit integers: the same bytes as uint8, twice the counts)
        import torch
        send2 = _Splits([2 * int(x) for x in send_l])
        send2.max_block = 2 * getattr(send_l, "max_block", 0)
        return all_to_all_v(dist, out.view(torch.uint8), inp.view(torch.uint8), [2 * int(x) for x in got_l], send2, group, async_op)
    lim = A2A_MAX_BYTES // inp.element_size()
    world = len(send_l)
    big = max(getattr(send_l, "max_block", 0), max(list(send_l) + list(got_l) + [0]))
    if big <= lim:
        if async_op:
            return [dist.all_to_all_single(out, inp, output_split_sizes=list(got_l), input_split_sizes=list(send_l), group=group, async_op=True)]
        dist.all_to_all_single(out, inp, output_split_sizes=list(got_l), input_split_sizes=list(send_l), group=group)
        return []
    soff, goff, a, b = [], [], 0, 0
    for p in range(world):
        soff.append(a)
        goff.append(b)
        a += int(send_l[p])
        b += int(got_l[p])
    handles = []
    for j in range((big + lim - 1) // lim):
        ins = [inp[soff[p] + min(j * lim, int(send_l[p])):soff[p] + min((j + 1) * lim, int(send_l[p]))] for p in range(world)]
        outs = [out[goff[p] + min(j * lim, int(got_l[p])):goff[p] + min((j + 1) * lim, int(got_l[p]))] for p in range(world)]
        if _no_list_all_to_all(dist, group):
            _packed_all_to_all(dist, outs, ins, group)
        elif async_op:
            handles.append(dist.all_to_all(outs, ins, group=group, async_op=True))
        else:
            dist.all_to_all(outs, ins, group=group)
    return handles


def _no_list_all_to_all(dist, group) -> bool:
    """gloo (the CPU tests' backend) has all_to_all_single but not the list form RCCL has."""
    try:
        return str(dist.get_backend(group)) == "gloo" and not isinstance(dist, HostStagedDist)
    except Exception:
        return False


def _packed_all_to_all(dist, outs, ins, group):
    import torch
    o = torch.empty(sum(x.numel() for x in outs), dtype=outs[0].dtype, device=outs[0].device)
    dist.all_to_all_single(o, torch.cat([x.reshape(-1) for x in ins]), output_split_sizes=[x.numel() for x in outs],
                           input_split_sizes=[x.numel() for x in ins], group=group)
    at = 0
    for x in outs:
        x.copy_(o[at:at + x.numel()])
        at += x.numel()


def _log2(g: int) -> int:
    b = g.bit_length() - 1
    if g < 1 or (1 << b) != g or g > 256:
        raise ValueError("number of ranks must be a power of two <= 256")
    return b


def _rank(dist, group=None) -> int:
    return int(dist.get_rank(group)) if group is not None else int(dist.get_rank())


def _takes_async(fn) -> bool:
    """Does this backend's collective take ``async_op``?  torch.distributed's return Work handles whose wait() orders the
    current stream after the collective; stand-ins without it (HostStagedDist, tests) run synchronously.  Decided from
    the signature -- a TypeError raised by the real backend (bad split list, dtype) is an error, not a reason to run the
    collective again."""
    import inspect
    try:
        return "async_op" in inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False


def _exchange_rows(dist, counts, capacity: int, world: int, group, flag=None, between=None, on_host: bool = True):
    """The count exchange under :func:`exchange_counts`, :func:`exchange_bucket_counts` and :func:`exchange_fine_counts`:
    one all-gather of a row [``counts`` | capacity (| ``flag``)] of int64 per rank; ``counts`` = this rank's keys per
    bucket, ``world`` destinations of equally many buckets each.  Returns (send_list, recv_list, mine, flags): ``mine`` =
    [world, buckets per rank]: row s = the sizes of source s's extents of this rank's buckets, in arrival order; ``flags``
    = every rank's flag word, on the host.  ``on_host`` False: the per-bucket counts stay on the device, only the world x
    world send matrix, the capacities and the flags come to the host, in ONE small copy.  Raises :class:`ReceiveOverflow`
    on every rank if any rank's total exceeds its capacity.
    ``between``: device work that does not depend on the other ranks' counts is queued while the counts travel and the
    host waits for them; with a backend whose collectives block the host it is queued first."""
    import torch
    nb = counts.numel()
    row = torch.cat([counts.to(torch.int64), torch.tensor([capacity], dtype=torch.int64, device=counts.device)] + ([flag] if flag is not None else []))
    rows = [torch.empty_like(row) for _ in range(world)]
    if between is not None and _takes_async(dist.all_gather):
        h = dist.all_gather(rows, row, group=group, async_op=True)
        between()
        h.wait()
    else:
        if between is not None:
            between()
        dist.all_gather(rows, row, group=group)
    allc = torch.stack(rows)                                      # [sender, bucket | capacity (| flag)]
    if on_host:
        allc = allc.cpu()                                         # one D2H
    per = nb // world
    to_rank = allc[:, :nb].view(world, world, per).sum(dim=2)     # [sender, destination]
    small = torch.cat([to_rank.reshape(-1)] + [allc[:, c] for c in range(nb, row.numel())]).cpu()   # (on the device: one D2H)
    to_rank, caps, flags = small[:world * world].view(world, world), small[world * world:world * world + world], small[world * world + world:]
    totals = to_rank.sum(dim=0)
    over = [(r, int(totals[r]), int(caps[r])) for r in range(world) if int(totals[r]) > int(caps[r])]
    if over:
        raise ReceiveOverflow("receive buffer too small on rank(s) " +
                              ", ".join(f"{r}: {t} keys for capacity {c}" for r, t, c in over) +
                              " (raise the slack -- the reference's fudge -- or use sort_sharded_u32_sampled)")
    me = _rank(dist, group)
    send_l = _Splits(to_rank[me].tolist())
    send_l.max_block = int(to_rank.max())
    return send_l, to_rank[:, me].tolist(), allc[:, me * per:(me + 1) * per], flags


def exchange_counts(dist, send, capacity: int, world: int, group=None):
    """All ranks learn the whole G x G send matrix and every rank's receive capacity
    (one all-gather of G+1 int64 per rank).  Returns (send_list, recv_list) of this rank;
    raises :class:`ReceiveOverflow` on every rank if any rank's total exceeds its capacity."""
    return _exchange_rows(dist, send, capacity, world, group)[:2]


def exchange_bucket_counts(dist, counts, capacity: int, world: int, group=None):
    """Like :func:`exchange_counts`, at the granularity of the 256 top-digit buckets: every rank learns every rank's
    bucket sizes (one all-gather of 257 int64 per rank).  Returns (send_list, recv_list, mine): ``mine[s][j]`` = keys of
    this rank's j-th bucket that source rank s holds -- the lengths of the runs this rank receives, in arrival order."""
    send_l, got_l, mine, _ = _exchange_rows(dist, counts, capacity, world, group)
    return send_l, got_l, mine.tolist()


FINE_BITS = 16          # the fine scheme orders a shard by its top 16 bits before the exchange ...
FINE_MIN_KEYS = 1 << 27  # ... when a rank holds at least this many keys (buckets of >= 2^11 keys per source)


def use_fine(n_keys: int, world: int, have_work: bool, scheme=None, _force_exchange: bool = False) -> bool:
    """Which scheme ``sort_sharded_u32`` / ``ShardedSorter`` take: ``scheme`` "fine" / "coarse" forces one (tests,
    experiments); by default the fine scheme runs when there is a second buffer, 2..8 ranks and a large shard.  Every
    rank must come to the same answer: shards of one call should be equally long (they are in bench.py)."""
    if scheme == "coarse" or (world < 2 and not _force_exchange) or not have_work:
        return False
    if scheme == "fine":
        return True
    return world <= 8 and n_keys >= FINE_MIN_KEYS


def exchange_fine_counts(dist, counts, capacity: int, world: int, group=None, hist_ok=None, between=None):
    """The fine scheme's count exchange: ``counts`` = this rank's 2^16 bucket sizes (int64, on the device).  One
    all-gather of 2^16 + 2 int64 per rank; the world x world send matrix and the capacities come to the host in ONE
    small copy, the per-bucket counts stay on the device.  Returns (send_list, recv_list, mine): ``mine`` = int64
    [world, 2^16 / world] on the device -- row s: the lengths of source s's extents of this rank's buckets, in arrival
    order.  Raises :class:`ReceiveOverflow` on every rank if any rank's total exceeds its capacity.
    ``hist_ok``: a one-element tensor on the device, non-zero = this rank has its buckets ready as histogram records; the
    records travel only if EVERY rank has -- the verdict is returned as ``send_list.use_hist``.  ``between``: the scatter
    of the low halves (:func:`_exchange_rows`)."""
    import torch
    flag = (hist_ok.to(torch.int64).reshape(1) != 0).to(torch.int64) if hist_ok is not None else torch.zeros(1, dtype=torch.int64, device=counts.device)
    send_l, got_l, mine, flags = _exchange_rows(dist, counts, capacity, world, group, flag, between, on_host=False)
    send_l.use_hist = bool((flags != 0).all())
    return send_l, got_l, mine.contiguous()


# The fine scheme exchanges only the keys' LOW halves: once the shard is ordered by its top 16 bits the upper half of a
# key is its bucket's number, which every receiver knows from the all-gathered counts.  Half the bytes cross xGMI -- one
# link per pair of GPUs: at 2^30 keys per rank a pair exchanges 2 GiB at 2 ranks, 1 GiB at 4, which takes longer than
# all of a rank's local work -- and the counting leaf reads half as much; the price is one more pass over the shard
# (read 4, write 2 bytes per key: engine.pack_low16).  (False: whole keys travel; tests and A/B comparisons)
FINE_LOW16 = True


# Dense buckets travel as HISTOGRAMS of their low halves (engine.hist2_pack): one record of 17408 bytes per source and
# bucket -- 2^16 2-bit counters + the values with three or more copies -- whatever the bucket holds, a quarter of the
# whole keys' bytes at 2^14 keys per source and bucket (2^30 keys per rank), and the receiver adds histograms instead of
# counting keys.  Used when every rank holds at least FINE_HIST_MIN_KEYS keys and no bucket overflows its record (every
# rank reports that with its counts; otherwise the low halves travel).  (False: never; tests and A/B comparisons)
FINE_HIST = True
FINE_HIST_MIN_KEYS = 3 << 28     # 12288 keys per bucket: a record is then 0.7 of the bucket's low halves
# ... and only up to this many ranks.  One GPU's measurements at 2^30 keys per rank (tools/multigpu_local_work.py,
# profiles/r03_multigpu_local_work.jsonl): a rank's local work per step is 8.8 / 8.2 / 7.9 ms at 2 / 4 / 8 ranks with
# records (order_low16 4.85 + pack 1.3 + leaf), 7.6 / 6.9 / 6.7 with low halves (order_low16 4.85 + leaf), while a pair of
# GPUs -- ONE xGMI link, 76.8 GB/s each way at best, 55-60 expected of an all-to-all -- exchanges 4 n / G bytes as whole
# keys, half of that as low halves, 1.06 n / G as records: at 2^30 keys and 58 GB/s 37 / 18.5 / 9.8 ms at 2 ranks, 18.5 / 9.3
# / 4.9 at 4, 9.3 / 4.6 / 2.5 at 8.  Records where the low halves would take longer over the link than the local work they
# hide behind (2 ranks: 9.8 against 18.5 ms per step; 4 ranks: 8.5 against 9.3 -- a tie if the links reach 66 GB/s);
# low halves where the exchange hides either way (8 ranks).
FINE_HIST_MAX_WORLD = 4
HIST2_RECORD_BYTES = 17408
RECORDS_BYTES = (1 << FINE_BITS) * HIST2_RECORD_BYTES   # a shard's buckets as records


def _wants_records(n_keys: int, world: int, send_room: int, recv_room: int) -> bool:
    """Does this rank prepare its buckets as histogram records?  (msd_sort_u32_sharded, csrc/msd_sharded.hip, states the
    same rule with the same inputs.)  Few ranks, a big shard, and room (bytes) for 2^16 records where they are packed AND
    where they arrive: records that cannot be received are never sent, so they are not packed either."""
    return FINE_HIST and world <= FINE_HIST_MAX_WORLD and n_keys >= FINE_HIST_MIN_KEYS and min(send_room, recv_room) >= RECORDS_BYTES


def _bytes_view(buf):
    import torch
    return buf.view(torch.uint8)


def _hist_splits(world: int):
    nbytes = RECORDS_BYTES // world
    sp = _Splits([nbytes] * world)
    sp.max_block = nbytes
    return sp


def _as_low16(buf):
    """The int16 view of an int32 buffer (twice the elements)."""
    import torch
    return buf.view(torch.int16)


def _send_bufs_in_work(work, n: int, low16: bool, records: bool):
    """The one-shot's send buffers, carved out of the work buffer -- dead until the leaf writes it: (the int16 buffer for
    the low halves or None, the record area or None, "both can be filled at once").  The records lie behind the low
    halves, at the next 256-byte boundary; when both do not fit they overlap, the records come first (packed from the
    keys) and the low halves are written over them only if the records do not travel after all."""
    send16 = _as_low16(work)[:n] if low16 and 2 * work.numel() >= n else None
    if not records:
        return send16, None, True
    w8 = _bytes_view(work)
    rec_at = (2 * n + 255) // 256 * 256 if send16 is not None else 0
    if w8.numel() - rec_at >= RECORDS_BYTES:
        return send16, w8[rec_at:], True
    return send16, w8, False


def _fine_prepare(engine, keys, send16, rec, apart: bool):
    """What a rank does before the fine exchange.  Returns (its 2^16 bucket sizes -- int64, on the device --, the flag "my
    buckets are ready in ``rec`` as histogram records" or None, "the low halves are ready in ``send16``": True, False, or a
    callable that makes them ready and is to be called once -- while the counts are exchanged).
    * records wanted (``rec``), and ``send16`` beside them: ``engine.order_low16`` as below, then the records are packed
      from the low halves (``engine.hist2_pack``) -- which are then also ready for the case that some rank's records
      overflow and every rank sends low halves after all; without ``send16`` (or with the records lying over it) the shard
      is ordered in place by its top 16 bits (``engine.sort_top``) and the records are packed from the keys;
    * no records, an int16 buffer ``send16``: ``engine.order_low16`` -- one in-place round on the top 8 bits, exact counts,
      the low halves scattered out of place into ``send16``: two passes over the shard less than ordering in place and
      packing afterwards (5.5 against 6.75 ms per 2^30 keys);
    * else the shard is ordered in place and whole keys (or low halves packed afterwards) travel."""
    n = keys.numel()
    if send16 is not None and send16.numel() >= n and hasattr(engine, "order_low16") and (rec is None or apart):
        if rec is not None:
            counts = engine.order_low16(keys, send16)
            return counts, engine.hist2_pack(send16[:n], engine.bounds_from_counts16(counts), rec) == 0, True
        if hasattr(engine, "order_low16_counts"):   # the scatter runs while the counts are exchanged (_exchange_rows' `between`)
            return engine.order_low16_counts(keys), None, (lambda: engine.order_low16_scatter(keys, send16))
        return engine.order_low16(keys, send16), None, True
    engine.sort_top(keys, 32 - FINE_BITS)
    b = engine.bucket_bounds(keys, 32 - FINE_BITS, 1 << FINE_BITS)
    return b[1:] - b[:-1], (engine.hist2_pack(keys, b, rec) == 0) if rec is not None else None, False


def _fine_start(engine, dist, keys, recv, capacity: int, world: int, group, send_room: int, send_bufs, async_op: bool):
    """First half of the fine scheme for one shard: prepare, exchange the counts (raises on all ranks), start -- or,
    without ``async_op``, run -- the one all-to-all into ``recv``.  The callers differ only in where the send buffers come
    from: ``send_bufs(n, low16, records)`` returns (send16, rec, apart) as :func:`_send_bufs_in_work` does, ``send_room`` =
    the bytes it has for records.  Returns what is in flight: (the view of ``recv`` being filled, the Work handles, ("fine", what
    :func:`_fine_finish` needs)) and the name of the form that travels."""
    n = keys.numel()
    send16, rec, apart = send_bufs(n, FINE_LOW16, _wants_records(n, world, send_room, 4 * recv.numel()))
    counts, hist_ok, packed = _fine_prepare(engine, keys, send16, rec, apart)
    between = packed if callable(packed) else None
    send_l, got_l, mine = exchange_fine_counts(dist, counts, capacity, world, group, hist_ok, between)
    if send_l.use_hist:      # every rank's buckets are ready as histogram records: equal blocks travel
        form, sp = "histogram records", _hist_splits(world)
        arrived, src, m, got, send = _bytes_view(recv), rec[:sum(sp)], sum(sp), list(sp), sp
    elif send16 is not None:  # the low halves arrive as int16; the leaf puts the upper halves back
        if not packed:   # (the shard was ordered in place: the records did not travel after all, or no order_low16)
            engine.pack_low16(keys, send16)
        form, arrived, src, m, got, send = "low halves", _as_low16(recv), send16, int(sum(got_l)), got_l, send_l
    else:
        form, arrived, src, m, got, send = "whole keys", recv, keys, int(sum(got_l)), got_l, send_l
    out = arrived[:m]
    return (out, all_to_all_v(dist, out, src, got, send, group, async_op), ("fine", arrived, mine, got_l)), form


def _fine_finish(engine, flight, out, rank: int, world: int):
    """Second half: wait for the exchange, then the counting leaf over what arrived, into ``out`` (a work buffer):
    source s's extents lie back to back from sum(got_l[:s]) on."""
    _, handles, (_, arrived, mine, got_l) = flight
    for h in handles:
        h.wait()
    base, at = [], 0
    for g in got_l:
        base.append(at)
        at += int(g)
    engine.merge_buckets(arrived, mine, base, 32 - FINE_BITS, rank * ((1 << FINE_BITS) // world), out, at)
    return out[:at]


def bucket_major(mine):
    """The runs a rank received (``mine[s][j]``: source-major, as the all-to-all delivers them) and where each belongs
    when every bucket is to be contiguous: (src_off, dst_off, lens) for ``engine.gather_runs`` and the bucket
    boundaries ``seg_off`` for ``engine.sort_segments``."""
    world, per = len(mine), len(mine[0])
    src_off, dst_off, lens = [], [], []
    bucket_start, at = [], 0
    for j in range(per):
        bucket_start.append(at)
        at += sum(int(mine[s][j]) for s in range(world))
    seg_off = bucket_start + [at]
    pos = 0
    fill = list(bucket_start)
    for s in range(world):
        for j in range(per):
            n = int(mine[s][j])
            src_off.append(pos)
            dst_off.append(fill[j])
            lens.append(n)
            pos += n
            fill[j] += n
    return src_off, dst_off, lens, seg_off


def _local_sort(engine, keys, rids=None, end_bit=None):
    """The engine's sort for these keys (int32: u32, int64: u64; with ``rids``: tuples), on all bits or below ``end_bit``."""
    kw = {} if end_bit is None else {"end_bit": end_bit}
    if rids is not None:
        engine.sort_pairs_u64(keys, rids, **kw)
    else:
        (engine.sort_u32 if keys.element_size() == 4 else engine.sort_u64)(keys, **kw)


def _plain_start(dist, send, keys, recv, world: int, group, rids=None, recv_rids=None, async_op: bool = False):
    """Keys already partitioned by destination (``send`` = keys per destination rank, on the device): exchange the counts
    (raises on all ranks), then one all-to-all of the keys -- and of the rids, with the same splits -- into the receive
    buffers.  Returns (keys view, rids view or None, Work handles)."""
    send_l, got_l = exchange_counts(dist, send, recv.numel(), world, group)
    m = int(sum(got_l))
    out, out_r = recv[:m], None
    handles = all_to_all_v(dist, out, keys, got_l, send_l, group, async_op)
    if rids is not None:
        out_r = recv_rids[:m]
        handles += all_to_all_v(dist, out_r, rids, got_l, send_l, group, async_op)
    return out, out_r, handles


def _exchange_and_sort(engine, dist, send, keys, recv, world: int, group, rids=None, recv_rids=None, end_bit=None):
    """:func:`_plain_start`, run to its end, and the local sort of what arrived (``end_bit``: the bits the ranks' ranges
    share are not sorted again; None: a full sort).  Returns (keys, rids) views of the receive buffers."""
    out, out_r, _ = _plain_start(dist, send, keys, recv, world, group, rids, recv_rids)
    _local_sort(engine, out, out_r, end_bit)
    return out, out_r


def _coarse_work(world: int, work_bufs):
    """The work buffers the coarse scheme uses: the arrived runs are gathered bucket-major into one of them and sorted
    there as segments on 24 bits (the local sort does not repeat the top-digit pass) -- up to 4 ranks.  Beyond, and
    without work buffers, the keys are sorted where they arrived.
    (8 ranks and more: the 32 buckets of a rank hold 2^25 keys each at 2^30 keys per rank, one more 8-bit round leaves
    2^17-key segments, beyond the fast counting leaf -- sorting the arrived keys on 29 bits measures faster: 8.5 against
    1.6 + 9.7 ms, tools/multigpu_local_work.py; 2 and 4 ranks: 9.2 and 8.9 against 13.0 and 12.5 ms)"""
    return list(work_bufs) if work_bufs and world <= 4 else []


def _coarse_start(engine, dist, keys, recv, work_bufs, world: int, group, async_op: bool):
    """First half of the coarse scheme: one top-digit pass, count exchange (raises on all ranks), the all-to-all started
    or run.  Returns what is in flight: (the view of ``recv`` being filled, the Work handles, the runs' lengths
    ``mine[s][j]`` for the gather into a work buffer -- or None: sort where they arrived)."""
    counts = engine.partition(keys, 24, 8)                       # int64[256], device of `keys`
    if not work_bufs:
        out, _, handles = _plain_start(dist, counts.view(world, 256 // world).sum(dim=1), keys, recv, world, group, async_op=async_op)
        return out, handles, None
    send_l, got_l, mine = exchange_bucket_counts(dist, counts, min(recv.numel(), min(w.numel() for w in work_bufs)), world, group)
    out = recv[:int(sum(got_l))]
    return out, all_to_all_v(dist, out, keys, got_l, send_l, group, async_op), mine


def _coarse_finish(engine, flight, work, world: int):
    """Second half: wait, then sort what arrived -- where it is, on the bits below the rank's, or gathered into ``work``."""
    arrived, handles, mine = flight
    for h in handles:
        h.wait()
    if mine is None:
        _local_sort(engine, arrived, end_bit=32 - _log2(world))
        return arrived
    out = work[:arrived.numel()]
    src_off, dst_off, lens, seg_off = bucket_major(mine)
    engine.gather_runs(out, arrived, src_off, dst_off, lens)
    engine.sort_segments(out, seg_off, 24)
    return out


def sort_sharded_u32(engine, keys, recv, dist, world: int, group=None, work=None, scheme=None, _force_exchange: bool = False):
    """Sorts the union of all ranks' ``keys`` (int32 tensors holding u32 bit patterns).
    Returns this rank's sorted range; rank r's range precedes rank r+1's.

    ``scheme``: None = choose (:func:`use_fine`), "fine" / "coarse" = force.  The fine scheme (module docstring)
    needs ``work``; its result is a view of ``work``, and ``recv`` must hold what arrives plus up to 3 elements
    (the leaf reads whole 16-byte vectors).

    With a second buffer ``work`` (as large as ``recv``) the local sort does not repeat the top-digit pass: the runs
    that arrived (per source, that source's buckets of this rank's range) are gathered bucket-major into ``work`` in
    one launch and sorted there as segments on the remaining 24 bits -- the result is a view of ``work``.  Without it
    the received keys are sorted in ``recv`` on all ``32 - log2(world)`` bits.

    Both schemes are a start and a finish (:func:`_fine_start` / :func:`_fine_finish`, :func:`_coarse_start` /
    :func:`_coarse_finish`), run here one after the other; :class:`ShardedSorter` runs them apart."""
    _log2(world)
    if world == 1 and not _force_exchange:   # (_force_exchange: tests run the whole exchange over a one-rank process group)
        engine.sort_u32(keys)
        return keys
    if use_fine(keys.numel(), world, work is not None, scheme, _force_exchange):
        flight, _ = _fine_start(engine, dist, keys, recv, min(recv.numel(), work.numel()), world, group, 4 * work.numel(),
                                lambda n, low16, records: _send_bufs_in_work(work, n, low16, records), False)
        return _fine_finish(engine, flight, work, _rank(dist, group), world)
    work_bufs = _coarse_work(world, [work] if work is not None else [])
    return _coarse_finish(engine, _coarse_start(engine, dist, keys, recv, work_bufs, world, group, False), work, world)


def sort_sharded_u64(engine, keys, recv, dist, world: int, group=None):
    """:func:`sort_sharded_u32` for u64 keys (int64 tensors holding the bit patterns): top 8 bits, one all-to-all,
    local sort with ``end_bit = 64 - log2(world)``."""
    lg = _log2(world)
    if world == 1:
        _local_sort(engine, keys)
        return keys
    send = engine.partition(keys, 56, 8).view(world, 256 // world).sum(dim=1)
    return _exchange_and_sort(engine, dist, send, keys, recv, world, group, end_bit=64 - lg)[0]


def sort_sharded_pairs_u64(engine, keys, rids, recv_keys, recv_rids, dist, world: int, group=None):
    """The reference's own job across devices: (u64 key, u64 rid) tuples held in one (keys, rids) pair of arrays per
    memory node (``sort(keys, rids, size, threads, numa, ...)``, src/msb_64.c:2261; contiguous key ranges per node
    :1596-1607, local sorting :2200-2255) -- here one pair per GPU.  One in-place pass on the top 8 key bits moves keys
    and rids together, the counts are exchanged once, keys and rids travel in two all-to-alls with the same splits,
    and every rank sorts the tuples it received on the remaining bits (``end_bit = 64 - log2(world)``, the
    reference's ``bits`` after its split, :2242).  Returns (keys, rids) views of the receive buffers; rank r's keys
    precede rank r+1's; like the reference's, the sort is unstable."""
    lg = _log2(world)
    if world == 1:
        _local_sort(engine, keys, rids)
        return keys, rids
    if recv_keys.numel() != recv_rids.numel():
        raise ValueError("receive buffers for keys and rids differ in length")
    send = engine.partition(keys, 56, 8, rids=rids).view(world, 256 // world).sum(dim=1)
    return _exchange_and_sort(engine, dist, send, keys, recv_keys, world, group, rids, recv_rids, end_bit=64 - lg)


class ShardedSorter:
    """Pipelined form of :func:`sort_sharded_u32` for a stream of shards (``bench.py --gpus N``).

    ``submit(keys)`` runs the top-digit pass on a shard, exchanges the counts and STARTS the
    all-to-all into the next receive buffer; ``collect()`` waits for the oldest exchange and sorts
    what arrived.  Calling ``submit(s)`` before ``collect(s-1)`` lets the exchange of shard s run on
    RCCL's stream (xGMI) while the compute stream sorts shard s-1 -- the exchange is as long as a
    local sort, so hiding it is what weak scaling needs.  ``recv_bufs``: at least two buffers (one
    per exchange in flight plus the one being sorted); the tensor returned by ``collect`` is a view
    of one of them -- with work buffers, of a WORK buffer -- and is overwritten ``len(recv_bufs)``
    (``len(work_bufs)``) submissions later.  ``keys`` must stay untouched until the matching ``collect`` returns.
    """

    def __init__(self, engine, dist, world: int, recv_bufs, group=None, work_bufs=None, scheme=None, _force_exchange: bool = False):
        self.engine, self.dist, self.world, self.group = engine, dist, world, group
        self.scheme = scheme              # None: by shard size (use_fine); "fine" / "coarse": forced
        self._force = _force_exchange     # (tests) one rank goes through the whole exchange
        _log2(world)
        self.recv = list(recv_bufs)
        if (world > 1 or _force_exchange) and len(self.recv) < 2:
            raise ValueError("ShardedSorter needs two receive buffers")
        self.fine_work = list(work_bufs) if work_bufs else []   # the fine scheme uses the work buffers at any rank count
        self.work = _coarse_work(world, work_bufs)
        self._wslot = 0
        self._slot = 0
        self._pending = []                # per shard in flight: (view being filled, Work handles, ...) -- bench.py reads the first two
        self._async = None
        self._send16 = []                 # fine scheme: the packed low halves of the shards whose exchange is in flight
        self._send8 = []                  # ... or their buckets' histogram records
        self.last_format = None           # what the last fine exchange moved (reporting)

    def _send_bufs(self, slot: int, device, n: int, low16: bool, records: bool):
        """The fine scheme's send buffers of a slot: one buffer of low halves and one of records per receive buffer,
        allocated when first needed; they never overlap."""
        import torch
        send16 = rec = None
        if low16:
            self._send16 += [None] * (len(self.recv) - len(self._send16))
            if self._send16[slot] is None or self._send16[slot].numel() < n:
                self._send16[slot] = torch.empty(n, dtype=torch.int16, device=device)
            send16 = self._send16[slot][:n]
        if records:
            self._send8 += [None] * (len(self.recv) - len(self._send8))
            if self._send8[slot] is None:
                self._send8[slot] = torch.empty(RECORDS_BYTES, dtype=torch.uint8, device=device)
            rec = self._send8[slot]
        return send16, rec, True

    def submit(self, keys) -> None:
        if self.world == 1 and not self._force:
            self._pending.append((keys, [], "local"))
            return
        if len(self._pending) >= len(self.recv):
            raise RuntimeError("collect() before submitting more shards than there are receive buffers")
        if self._async is None:
            self._async = _takes_async(self.dist.all_to_all_single)
        slot, recv = self._slot, self.recv[self._slot]
        if use_fine(keys.numel(), self.world, bool(self.fine_work), self.scheme, self._force):
            cap = min(recv.numel(), min(w.numel() for w in self.fine_work))
            flight, self.last_format = _fine_start(self.engine, self.dist, keys, recv, cap, self.world, self.group, RECORDS_BYTES,
                                                   lambda n, low16, records: self._send_bufs(slot, keys.device, n, low16, records), self._async)
        else:
            flight = _coarse_start(self.engine, self.dist, keys, recv, self.work, self.world, self.group, self._async)
        self._slot = (slot + 1) % len(self.recv)
        self._pending.append(flight)

    def collect(self):
        flight = self._pending.pop(0)
        if flight[2] == "local":
            self.engine.sort_u32(flight[0])
            return flight[0]
        fine = isinstance(flight[2], tuple)
        work = self.fine_work if fine else self.work
        if not work:
            return _coarse_finish(self.engine, flight, None, self.world)
        final = work[self._wslot]                        # (collect() returns a view of a work buffer, overwritten len(work) collects later)
        self._wslot = (self._wslot + 1) % len(work)
        if fine:   # the counting leaf reads the extents in the receive buffer, writes the work buffer
            return _fine_finish(self.engine, flight, final, _rank(self.dist, self.group), self.world)
        return _coarse_finish(self.engine, flight, final, self.world)

    def pending(self) -> int:
        return len(self._pending)


def _sort_sharded_sampled(engine, keys, rids, recv, recv_rids, dist, world: int, group, sample_per_rank: int, seed: int):
    import torch
    pairs = rids is not None
    if world == 1:
        _local_sort(engine, keys, rids)
        return (keys, rids) if pairs else keys
    if pairs and recv.numel() != recv_rids.numel():
        raise ValueError("receive buffers for keys and rids differ in length")
    n = keys.numel()
    m = min(sample_per_rank, n)
    mine = engine.sample(keys, m, seed + 7919 * _rank(dist, group))
    # ranks may hold different numbers of keys: gather the sample sizes, then the (padded) samples
    cnt = torch.tensor([m], dtype=torch.int64, device=keys.device)
    cnts = [torch.zeros_like(cnt) for _ in range(world)]
    dist.all_gather(cnts, cnt, group=group)
    sizes = [int(c.item()) for c in cnts]
    mmax = max(sizes)
    pad = torch.zeros(max(mmax, 1), dtype=keys.dtype, device=keys.device)
    pad[:m] = mine
    allp = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(allp, pad, group=group)
    sample = torch.cat([p[:s] for p, s in zip(allp, sizes)]).contiguous()
    if sample.numel():
        _local_sort(engine, sample)
        delim = engine.splitters(sample, world)                         # [world-1] key bit patterns, on the device
    else:
        delim = torch.zeros(world - 1, dtype=keys.dtype, device=keys.device)
    send = engine.partition_by_splitters(keys, delim, world, rids=rids) if pairs else engine.partition_by_splitters(keys, delim, world)
    out, out_r = _exchange_and_sort(engine, dist, send, keys, recv, world, group, rids, recv_rids)   # (send: range sizes, ranges contiguous)
    return (out, out_r) if pairs else out



def sort_sharded_u32_sampled(engine, keys, recv, dist, world: int, group=None, sample_per_rank: int = 65536,
                             seed: int = 0x5EED0007):
    """Skew-robust variant, the reference's own scheme (src/msb_64.c:1511-1564) with one range per rank:

      * every rank draws ``sample_per_rank`` keys at random from its UNSORTED shard
        (``engine.sample``: index = mulhi(rand64, n), :1511-1521) -- nothing is sorted before the exchange;
      * the samples are all-gathered and sorted (``engine.sort_u32``, the reference sorts its sample with
        eight passes of partition_keys, :1526-1541);
      * world-1 equi-depth delimiters with the reference's duplicate rule (``engine.splitters``,
        extract_delimiters :1304-1322) -- identical on every rank, the sample being the same;
      * ONE in-place pass cuts the shard into the ranges (delim[p-1], delim[p]]
        (``engine.partition_by_splitters``, the lower-bound range function :188-204);
      * count exchange, ONE all-to-all(v), ONE local sort of what arrived.

    A single key value heavier than 1/world of the data cannot be split (the reference's limitation too):
    balance degrades, the result stays correct as long as ``recv`` is large enough (else
    :class:`ReceiveOverflow` on every rank)."""
    return _sort_sharded_sampled(engine, keys, None, recv, None, dist, world, group, sample_per_rank, seed)


def sort_sharded_u64_sampled(engine, keys, recv, dist, world: int, group=None, sample_per_rank: int = 65536,
                             seed: int = 0x5EED0007):
    """:func:`sort_sharded_u32_sampled` for u64 keys (int64 tensors holding the bit patterns)."""
    return _sort_sharded_sampled(engine, keys, None, recv, None, dist, world, group, sample_per_rank, seed)


def sort_sharded_pairs_u64_sampled(engine, keys, rids, recv_keys, recv_rids, dist, world: int, group=None,
                                   sample_per_rank: int = 65536, seed: int = 0x5EED0007):
    """What the reference actually sorts -- (u64 key, u64 rid) tuples, one (keys, rids) pair of arrays per memory node
    (src/msb_64.c:2261) -- sharded by the reference's own skew front end (sample :1511-1521, extract_delimiters
    :1304-1322, range function :188-204) with one range per GPU: the radix split of :func:`sort_sharded_pairs_u64`
    puts ~75 % of Zipf-distributed keys on one rank, this keeps every rank near n / world.  Keys and rids move
    together in the one in-place range pass and travel in two all-to-alls with the same splits.  Returns (keys, rids)
    views of the receive buffers; rank r's keys precede rank r+1's; unstable, like the reference."""
    return _sort_sharded_sampled(engine, keys, rids, recv_keys, recv_rids, dist, world, group, sample_per_rank, seed)


def splitters_equi_depth(sorted_sample, parts: int):
    """parts-1 equi-depth delimiters from a sorted sample with the reference's duplicate
    rule (extract_delimiters, src/msb_64.c:1304-1322): if more repetitions of the picked
    value lie after the pick than before it, use value-1 so a heavy value does not
    straddle two ranges.  Range p = keys in (delim[p-1], delim[p]].  Host restatement (numpy / lists) of
    what ``msd_splitters_u32`` computes on the device; the tests check both against the compiled reference."""
    n = len(sorted_sample)
    out = []
    pct = n * 1.0 / parts
    for i in range(parts - 1):
        idx = int(pct * (i + 1) - 0.001)
        v = int(sorted_sample[idx])
        start = idx
        while start > 0 and int(sorted_sample[start]) == v:
            start -= 1
        end = idx
        while end < n and int(sorted_sample[end]) == v:
            end += 1
        if idx - start < end - idx and v:
            v -= 1
        out.append(v)
    return out

"""What msd_join_groups and msd_join_pairs have to produce (a helper module like set_expect.py, not a test).

The expectation is defined HERE, with numpy: both inputs are unsigned views of their bit patterns plus a key type
(``sort_rows_expect``'s U32 .. F64) and become order-preserving unsigned codes with ``sort_rows_expect.np_encode``.
``np.unique(return_index=True, return_counts=True)`` of each side gives its distinct values with the first index and the
length of every run, ``np.intersect1d`` the values both sides hold.  Equality is equality of codes, that is of bits: for
floats -0.0 and +0.0 differ and NaNs with equal bits are one value.

:func:`pairs` gives the index pairs of a range of ranks without building the whole product; :func:`tiles` is a numpy model
of the write kernel (csrc/msd_join.hpp): per tile of the merge path the groups whose A head lies in the tile, from the tile
and a halo of four elements, with at most one search behind the tile per side.

Plain module, no fixture: ``import join_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import search_expect as S
import set_expect as T
import sort_rows_expect as E

KEY_TYPES = S.KEY_TYPES


def groups(a_bits, b_bits, key_type):
    """``(keys, a_first, a_count, b_first, b_count)``: per value that both sides hold, ascending by code, its bit pattern
    and (uint64) the first index and the run length in A and in B"""
    a_bits, b_bits = np.asarray(a_bits), np.asarray(b_bits)
    ca, cb = E.np_encode(a_bits, key_type), E.np_encode(b_bits, key_type)
    for name, c in (("A", ca), ("B", cb)):
        assert (c[1:] >= c[:-1]).all(), "%s is not ascending in the order of its type" % name
    va, fa, na = np.unique(ca, return_index=True, return_counts=True)
    vb, fb, nb = np.unique(cb, return_index=True, return_counts=True)
    _, ia, ib = np.intersect1d(va, vb, assume_unique=True, return_indices=True)
    u = lambda x: x.astype(np.uint64)
    return a_bits[fa[ia]], u(fa[ia]), u(na[ia]), u(fb[ib]), u(nb[ib])


def total(g):
    """the number of pairs of the groups (a Python int: it may exceed 64 bits nowhere, n and m being below 2^32)"""
    return int(sum(int(p) * int(q) for p, q in zip(g[2].tolist(), g[4].tolist())))


def pairs(g, lo, hi):
    """``(ia, ib)`` (uint64) of the pairs with ranks [lo, min(hi, total)): the groups in order, within a group of p x q
    pairs rank t is (a_first + t // q, b_first + t % q)"""
    _, a_first, a_count, b_first, b_count = g
    ends = np.cumsum(a_count * b_count, dtype=np.uint64)
    tot = int(ends[-1]) if ends.size else 0
    r = np.arange(lo, max(lo, min(hi, tot)), dtype=np.uint64)
    at = np.searchsorted(ends, r, side="right")                     # the group of rank r: the first whose end lies beyond r
    t = r - (ends[at] - (a_count * b_count)[at])
    return a_first[at] + t // b_count[at], b_first[at] + t % b_count[at]


class _Window:
    """one side of a tile: reads are allowed inside [lo, hi) and at the halo indices; a search behind the tile is counted"""

    def __init__(self, x, lo, hi, halo):
        self.x, self.lo, self.hi, self.halo, self.searches = x, lo, hi, set(halo), 0

    def exists(self, i):
        return 0 <= i < len(self.x)

    def __getitem__(self, i):
        assert self.lo <= i < self.hi or i in self.halo, "index %d is neither in the tile [%d, %d) nor in its halo %s" % (i, self.lo, self.hi, sorted(self.halo))
        assert self.exists(i)
        return self.x[i]

    def upper_behind(self, v):
        """the end of the run of v that leaves the tile: the one global search"""
        self.searches += 1
        return self.hi + int(np.searchsorted(self.x[self.hi:], v, side="right"))


def tiles(a_codes, b_codes, tile):
    """The model: ``(codes, a_first, a_count, b_first, b_count)`` as the kernels compute them.  The splits are those of the
    merge (B after every A that is not larger).  In tile i, with a[a0, a1) and b[b0, b1) and the halo a[a0 - 1], a[a1],
    b[b0 - 1], b[b1]: an A element is kept iff its predecessor in A differs and b[b0 + lb] equals it, lb = |{b in tile : b <
    a}|.  Its runs end at a0 + |{a in tile : a <= v}| and b0 + |{b in tile : b <= v}| where those lie inside the tile;
    otherwise at the tile's end, unless the halo element behind the tile equals v: then one search behind the tile finds the
    end.  Asserts that every index read lies in the tile or the halo and that a tile searches at most once per side."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    sa, sb, _ = S.splits(a_codes, b_codes, tile, True)
    out = [[], [], [], [], []]
    for i in range(len(sa) - 1):
        a0, a1, b0, b1 = sa[i], sa[i + 1], sb[i], sb[i + 1]
        A = _Window(a_codes, a0, a1, [a0 - 1, a1])
        B = _Window(b_codes, b0, b1, [b0 - 1, b1])
        ka, kb = a_codes[a0:a1], b_codes[b0:b1]
        for e in range(a1 - a0):
            v = A[a0 + e]
            head = not (A.exists(a0 + e - 1) and A[a0 + e - 1] == v)
            lb = int((kb < v).sum())
            if not (head and B.exists(b0 + lb) and B[b0 + lb] == v):
                continue
            ua, ub = int((ka <= v).sum()), int((kb <= v).sum())
            a_end, b_end = a0 + ua, b0 + ub
            if ua == a1 - a0 and A.exists(a1) and A[a1] == v:
                a_end = A.upper_behind(v)
            if ub == b1 - b0 and B.exists(b1) and B[b1] == v:
                b_end = B.upper_behind(v)
            for col, x in zip(out, (v, a0 + e, a_end - (a0 + e), b0 + lb, b_end - (b0 + lb))):
                col.append(x)
        assert A.searches <= 1 and B.searches <= 1, "tile %d searches behind itself %d and %d times" % (i, A.searches, B.searches)
    return (np.array(out[0], a_codes.dtype),) + tuple(np.array(c, np.uint64) for c in out[1:])


# ---- the clamped models: inputs in ANY order, groups this library did not write (the pieces: search_expect, set_expect;
# DESIGN.md 10.13)

def global_upper(keys, lo, hi, v):
    """join_global_upper over the Checked array keys: inside [lo, hi] whatever keys holds"""
    lo0, hi0 = lo, hi
    assert lo <= hi <= len(keys)
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if keys[mid] <= v:
            lo = mid + 1
        else:
            hi = mid
    assert lo0 <= lo <= hi0
    return lo


def tiles_clamped(a_codes, b_codes, tile, cap=None, junk=S.NONE16, first=False, stats=None, counted=None):
    """The clamped model of msd_join_groups (the split, set_count_kernel with the intersection's mask, the scan,
    join_write_kernel) for inputs in ANY order.  ``cap`` None: no cap.  ``junk``, ``first``: see
    merge_expect.tiles_clamped; ``counted``: see set_expect.tiles_clamped.  Returns ``(Clamped(count, groups), junk_reads, collisions)``: count is what *d_num_groups
    receives, groups the Stores of (code, a_first, a_count, b_first, b_count)."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    n, m = len(a_codes), len(b_codes)
    A, B = S.Checked(a_codes, "a"), S.Checked(b_codes, "b")
    sa, _ = S.split_points(A.x, B.x, tile, True)
    splits = S.Checked(sa, "splits")
    tile_counts = T.count_clamped(A, B, splits, tile, T.KEEP_MASK[T.INTERSECTION]) if counted is None else counted
    count = sum(tile_counts)
    windows = S.out_windows(tile_counts, count, count if cap is None else cap)
    groups = S.Stores("groups")
    junk_reads = collisions = 0
    for i, (base, lim) in enumerate(windows):
        if base >= lim:
            continue
        t = T.ClampedTile(i, A, B, splits, tile, stats)
        na, nb = t.na, t.nb
        if na == 0:
            continue
        cnt = min(lim - base, na)
        has_a_behind = t.a0 + na < n
        a_behind = A[t.a0 + na] if has_a_behind else 0
        j = na + nb - 1 if junk == "last" else junk
        codes, below = S.Lds(tile, j, first, "codes"), S.Lds(tile, j, first, "below")
        kept_e, kept_lb = S.Lds(tile, j, first, "kept_e"), S.Lds(tile, j, first, "kept_lb")
        S.stage(A, t.a0, na, codes, 0)
        S.stage(B, t.b0, nb, codes, na)
        codes.barrier()

        def mark(e, x, lb, kept):
            below[e] = lb if kept else S.NONE16
        T.decide_a(codes, t, True, False, mark)
        below.barrier()

        def place(e, to, lb):
            kept_e[to] = e
            kept_lb[to] = lb
        marks = S.ballot_compact(below, na, cnt, tile, place)
        if stats is not None and min(marks, cnt) < cnt:
            stats.hit("unplaced")
        kept_e.barrier()
        kept_lb.barrier()
        for p in range(cnt):
            e = kept_e[p] if kept_e[p] < na - 1 else na - 1
            lb = kept_lb[p] if kept_lb[p] < nb else nb
            v = codes[e]
            af, bf = t.a0 + e, t.b0 + lb
            ua = S.lds_count(codes, 0, na, v, True)
            ub = S.lds_count(codes, na, nb, v, True)
            a_end, b_end = t.a0 + (ua if ua > e else e + 1), t.b0 + (ub if ub > lb else lb)
            if ua >= na and has_a_behind and a_behind == v:
                a_end = global_upper(A, t.a0 + na, n, v)
            if ub >= nb and t.has_b_behind and t.b_behind == v:
                b_end = global_upper(B, t.b0 + nb, m, v)
            assert base + p < lim
            assert a_end - af >= 1 and a_end <= n and b_end >= bf and b_end <= m      # what include/msd_join_hip.h promises
            groups[base + p] = (v, af, a_end - af, bf, b_end - bf)
        assert codes.junk_reads == 0 and below.junk_reads == 0
        junk_reads += kept_e.junk_reads + kept_lb.junk_reads
        collisions += below.collisions + kept_e.collisions
    assert collisions == 0                                          # (every local a has a place of its own: the groups call has no race)
    return S.Clamped(count=count, tile_counts=tile_counts, groups=groups), junk_reads, collisions


def search_trips_bound(G):
    """the most trips of the 64-ary search of join_expand_kernel over G groups: a range of len shrinks to at most
    ceil(len / 64) - 1 per trip"""
    trips, length = 0, G
    while length > 0:
        length = -(-length // 64) - 1
        trips += 1
    return trips


def expand_clamped(num_groups, groups_cap, a_first, a_count, b_first, b_count, n, m, pos_a, pos_b, cap, th, per, stats=None):
    """The clamped model of msd_join_pairs (join_offsets_kernel and the scan as wrapping sums, join_expand_kernel statement
    by statement) for ANY groups: the four arrays hold groups_cap words each, of any value below 2^64.  ``th`` threads take
    ``per`` ranks each (the kernel's 256 and 8: pair_tile = th * per).  No race and no junk: every LDS cell that is read
    was written.  Returns ``Clamped(total, out_a, out_b, trips)``: what *d_num_pairs receives, the Stores of the two outputs
    and the most trips a 64-ary search took."""
    PT = th * per
    AF, AC = S.Checked(a_first, "a_first"), S.Checked(a_count, "a_count")
    BF, BC = S.Checked(b_first, "b_first"), S.Checked(b_count, "b_count")
    assert len(AF) == len(AC) == len(BF) == len(BC) == groups_cap
    PA = None if pos_a is None else S.Checked(pos_a, "pos_a")
    PB = None if pos_b is None else S.Checked(pos_b, "pos_b")
    G = min(num_groups, groups_cap)
    offs, total = [], 0
    for g in range(G):                                                  # join_offsets_kernel, runs_scan_top_kernel
        offs.append(total)
        total = (total + AC[g] * BC[g]) & S.MASK64
    OFF = S.Checked(offs, "off")
    out_a, out_b = S.Stores("d_out_a"), S.Stores("d_out_b")
    stored = min(cap, n * m)
    grid = -(-stored // PT) if groups_cap else 0
    stop = min(total, cap)
    most_trips = 0
    for block in range(min(grid, -(-stop // PT))):                      # (a workgroup with r0 >= stop leaves before it loads anything else)
        r0 = block * PT
        assert r0 < stop
        cnt = min(stop - r0, PT)
        if G == 0:
            continue
        rel, sa, sb = S.Lds(PT, None, False, "rel"), S.Lds(PT, None, False, "sa"), S.Lds(PT, None, False, "sb")
        lo, hi, trips = 0, G, 0
        while lo < hi:
            step = (hi - lo + 63) >> 6
            c = 0
            for lane in range(64):
                at = lo + (lane + 1) * step - 1
                if at < hi and OFF[at] <= r0:
                    c += 1
            stop_at = lo + (c + 1) * step - 1
            lo += c * step
            hi = min(stop_at, hi)
            trips += 1
        most_trips = max(most_trips, trips)
        assert trips <= search_trips_bound(G), (trips, G)
        g0 = lo - 1 if lo else 0
        assert g0 < G
        for tid in range(th):
            o = 0
            for k in range(tid, PT, th):
                g = g0 + k
                if o < r0 + cnt:
                    o = OFF[g] if g < G else total
                rel[k] = (min(o - r0, cnt) if o > r0 else 0)
        rel.barrier()
        for tid in range(th):
            x0 = tid * per
            if x0 >= cnt:
                continue
            k = S.lds_count(rel, 1, PT - 1, x0, True)                   # (rel + 1)
            g = g0 + k if g0 + k < G else G - 1
            q = BC[g] if BC[g] else 1
            t0 = (r0 + x0 - OFF[g]) & S.MASK64
            row, col = t0 // q, t0 % q
            ia, ib0 = (AF[g] + row) & S.MASK64, BF[g]
            nxt = rel[k + 1] if k + 1 < PT else cnt
            for j in range(per):
                x = x0 + j
                if x < cnt:
                    if x >= nxt and k + 1 < PT:
                        k += 1
                        nxt = rel[k + 1] if k + 1 < PT else cnt
                        g = g0 + k if g0 + k < G else G - 1
                        q = BC[g] if BC[g] else 1
                        ia, ib0, col = AF[g], BF[g], 0
                    sa[x] = ia & 0xFFFFFFFF
                    sb[x] = (ib0 + col) & 0xFFFFFFFF
                    col += 1
                    if col >= q:
                        col = 0
                        ia = (ia + 1) & S.MASK64
        sa.barrier()
        sb.barrier()
        for p in range(cnt):
            ia, ib = sa[p], sb[p]
            assert r0 + p < stop
            out_a[r0 + p] = PA[ia if ia < n else n - 1] if PA is not None else ia
            out_b[r0 + p] = PB[ib if ib < m else m - 1] if PB is not None else ib
        assert rel.junk_reads == 0 and sa.junk_reads == 0 and sb.junk_reads == 0 and sa.collisions == 0
        if stats is not None:
            stats.hit("blocks")
    return S.Clamped(total=total, out_a=out_a, out_b=out_b, trips=most_trips)


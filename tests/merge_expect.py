"""What msd_merge_sorted has to produce (a helper module like search_expect.py, not a test).

The expectation is defined HERE, with numpy: both inputs are unsigned views of their bit patterns plus a key type
(``sort_rows_expect``'s U32 .. F64); the concatenation ``[A; B]`` becomes order-preserving unsigned codes with
``sort_rows_expect.np_encode``, and ``np.argsort(kind="stable")`` of the codes is the origin: the merged keys are the
concatenation's bit patterns in that order.  Stable means: among equal codes A before B, and within a side in input order.
For floats the order is IEEE-754 totalOrder on the bits, NOT numpy's or torch's float order.

:func:`tiles` is a numpy model of the two kernels (csrc/msd_merge2.hpp): the cut of the merged sequence into tiles along the
merge path -- ``search_expect.splits(..., right=True)`` is the split model -- and per tile the rank of every element.

Plain module, no fixture: ``import merge_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import search_expect as S
import sort_rows_expect as E

KEY_TYPES = S.KEY_TYPES


def expected(a_bits, b_bits, key_type):
    """``(merged_bits, origin)``: the n + m bit patterns in the stable order of their codes, and per position the index
    (uint64) in the concatenation [A; B] of the element that lands there"""
    a_bits, b_bits = np.asarray(a_bits), np.asarray(b_bits)
    for name, x in (("A", a_bits), ("B", b_bits)):
        c = E.np_encode(x, key_type)
        assert (c[1:] >= c[:-1]).all(), "%s is not ascending in the order of its type" % name
    cat = np.concatenate([a_bits, b_bits])
    origin = np.argsort(E.np_encode(cat, key_type), kind="stable")
    return cat[origin], origin.astype(np.uint64)


def tiles(a_codes, b_codes, tile):
    """The model: ``(merged_codes, origin)`` as the two kernels compute them.  The splits are those of the search's merge
    path under the RIGHT rule (B after every A that is not larger); in tile i local A element e goes to
    e + |{b in tile : b < a_e}| and local B element j to j + |{a in tile : a <= b_j}|, and position p of the tile's slice
    takes the element ranked there.  Asserts that every position is written exactly once."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    n, m = len(a_codes), len(b_codes)
    sa, sb, _ = S.splits(a_codes, b_codes, tile, True)
    merged = np.zeros(n + m, a_codes.dtype)
    origin = np.full(n + m, -1, np.int64)
    for i in range(len(sa) - 1):
        d0 = min(i * tile, n + m)
        ka, kb = a_codes[sa[i]:sa[i + 1]], b_codes[sb[i]:sb[i + 1]]
        assert len(ka) + len(kb) == min((i + 1) * tile, n + m) - d0
        ranked = [(e + int((kb < x).sum()), x, sa[i] + e) for e, x in enumerate(ka)]
        ranked += [(j + int((ka <= x).sum()), x, n + sb[i] + j) for j, x in enumerate(kb)]
        for r, x, src in ranked:
            assert 0 <= r < len(ka) + len(kb), "a rank outside the tile"
            assert origin[d0 + r] == -1, "a position written twice"
            merged[d0 + r], origin[d0 + r] = x, src
    assert (origin >= 0).all(), "a position no tile wrote"
    return merged, origin.astype(np.uint64)


def tiles_clamped(a_codes, b_codes, tile, junk=S.NONE16, first=False, stats=None):
    """The clamped model of merge_tile_kernel with values and origin, for inputs in ANY order (the pieces: search_expect).
    ``junk``: what an LDS cell that nothing wrote holds (S.JUNKS); ``first``: of two elements ranked to one place the first
    stays (else the last).  Returns ``(S.Clamped(out, vals, origin), junk_reads, collisions)``: out holds codes, vals the index
    in [A; B] of the value loaded, origin what the kernel stores."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    n, m = len(a_codes), len(b_codes)
    A, B = S.Checked(a_codes, "a"), S.Checked(b_codes, "b")
    VA, VB = S.Checked(range(n), "vals_a"), S.Checked(range(n, n + m), "vals_b")
    sa, _ = S.split_points(A.x, B.x, tile, True)
    splits = S.Checked(sa, "splits")
    out, vals, origin = S.Stores("d_out"), S.Stores("d_out_vals"), S.Stores("d_out_origin")
    junk_reads = collisions = 0
    for i in range(len(sa) - 1):
        t = S.Extent(i, n, m, splits, tile, stats)
        na, nb = t.na, t.nb
        cnt = min(na + nb, t.d1 - t.d0)
        if cnt == 0:
            continue
        last = na + nb - 1
        assert last >= 0
        j = last if junk == "last" else junk
        codes, outk, src = S.Lds(tile, j, first, "codes"), S.Lds(tile, j, first, "outk"), S.Lds(tile, j, first, "src")
        S.stage(A, t.a0, na, codes, 0)
        S.stage(B, t.b0, nb, codes, na)
        codes.barrier()

        def rank(self0):
            def f(e, x, base):
                r = e + base if e + base < last else last
                outk[r] = x
                src[r] = self0 + e
            return f
        S.merge_for_counts(codes, 0, na, na, nb, False, rank(0))       # (no barrier between the two sides)
        S.merge_for_counts(codes, na, nb, 0, na, True, rank(na))
        if stats is not None:
            stats.hit("collision", src.collisions)
            stats.hit("hole", sum(1 for p in range(cnt) if p not in src.cells))
        outk.barrier()
        src.barrier()
        for p in range(cnt):
            assert t.d0 + p < t.d1 <= n + m
            out[t.d0 + p] = outk[p]
            s = src[p] if src[p] < last else last
            from_a = s < na
            at = t.a0 + s if from_a else t.b0 + (s - na)
            vals[t.d0 + p] = VA[at] if from_a else VB[at]
            assert at < (n if from_a else m)
            origin[t.d0 + p] = at if from_a else n + at
        assert codes.junk_reads == 0                                    # (every code that is read was staged)
        junk_reads += outk.junk_reads + src.junk_reads
        collisions += src.collisions
    return S.Clamped(out=out, vals=vals, origin=origin), junk_reads, collisions

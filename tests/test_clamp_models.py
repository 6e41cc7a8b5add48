"""The clamped numpy models of the merge path (search_expect.tiles_clamped, merge_expect.tiles_clamped,
set_expect.tiles_clamped, join_expect.tiles_clamped, join_expect.expand_clamped): the second of the three layers of DESIGN.md
10.13.  They follow the tile kernels statement by statement, clamps included, with every read of an input, a split, a
position or an LDS cell index-checked and every store recorded -- so a LOAD outside an array, which a GPU test cannot see,
is an assertion here.

For ascending inputs a clamped model equals the model the other tests use; for inputs in any order -- every pair of arrays
over {0, 1, 2} with n, m <= 3, and 2000 random pairs with n, m < 40 per configuration -- no index check fails and every
store lies in the range the header promises.  LDS cells nothing wrote read as each of search_expect.JUNKS, and of the elements
ranked to one place either all first ones stay or all last ones (the two global orders of search_expect.variants, not one
choice per place).  The vectorised models that the GPU tests compare with are compared here with the statement-by-statement
ones.  Needs no GPU."""
import itertools

import numpy as np
import pytest

import join_expect as J
import merge_expect as M
import search_expect as S
import set_expect as X
import sort_rows_expect as E

TILES = (1, 3, 8, 16)
RANDOM_CASES = 2000


def ascending_inputs(distinct, trials=150):
    """the inputs of the model tests of test_merge_abi.py, test_setops_abi.py and test_join_abi.py"""
    rng = np.random.default_rng(distinct)
    for _ in range(trials):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        yield np.sort(rng.integers(0, distinct, n).astype(np.uint32)), np.sort(rng.integers(0, distinct, m).astype(np.uint32))
    yield np.array([3] * 10, np.uint32), np.array([3] * 20, np.uint32)
    yield np.array([3] * 10 + [4], np.uint32), np.array([3] * 20 + [5], np.uint32)
    yield np.array([3] * 10 + [4] * 3 + [6], np.uint32), np.array([3] * 20 + [4] + [5] + [6] * 9, np.uint32)


def small_arrays():
    """every array over {0, 1, 2} of length 0 .. 3"""
    return [np.array(x, np.uint32) for k in range(4) for x in itertools.product((0, 1, 2), repeat=k)]


def unsorted_inputs(seed):
    """every pair of small arrays, then RANDOM_CASES random pairs, n, m < 40, of few or many distinct values"""
    small = small_arrays()
    for a in small:
        for b in small:
            yield a, b
    rng = np.random.default_rng(seed)
    for _ in range(RANDOM_CASES):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        distinct = (2, 3, 5, 50, 1 << 32)[int(rng.integers(0, 5))]
        yield rng.integers(0, distinct, n).astype(np.uint32), rng.integers(0, distinct, m).astype(np.uint32)


def dense(stores, count, what):
    """the values of a Stores that holds exactly the indices [0, count), each stored once"""
    assert stores.indices() == set(range(count)), (what, sorted(stores.indices()), count)
    assert all(len(v) == 1 for v in stores.at.values()), what
    return [stores.at[i][0] for i in range(count)]


# ---- ascending inputs: the clamps change nothing

@pytest.mark.parametrize("distinct", [1, 2, 5, 50])
def test_on_ascending_inputs_the_clamped_models_are_the_models(distinct):
    stats = S.Stats()
    for a, b in ascending_inputs(distinct):
        n, m = a.size, b.size
        for tile in TILES:
            what = (a.tolist(), b.tolist(), tile)
            for right in (False, True):
                _, _, want = S.splits(a, b, tile, right)
                assert dense(S.tiles_clamped(a, b, tile, right, stats=stats), m, what) == want.tolist(), what
            want, want_origin = M.tiles(a, b, tile)
            got, junk_reads, collisions = M.tiles_clamped(a, b, tile, junk=0, stats=stats)
            assert junk_reads == 0 and collisions == 0, what
            assert dense(got.out, n + m, what) == want.tolist() and dense(got.origin, n + m, what) == want_origin.tolist(), what
            assert dense(got.vals, n + m, what) == want_origin.tolist(), what
            for op in X.OPS:
                want, want_origin = X.tiles(a, b, tile, op)
                got, junk_reads, collisions = X.tiles_clamped(a, b, tile, op, junk=0, stats=stats)
                assert junk_reads == 0 and collisions == 0 and got.count == want.size, (what, op)
                assert dense(got.out, want.size, what) == want.tolist() and dense(got.origin, want.size, what) == want_origin.tolist(), (what, op)
            want = J.tiles(a, b, tile)
            got, junk_reads, collisions = J.tiles_clamped(a, b, tile, junk=0, stats=stats)
            assert junk_reads == 0 and got.count == want[0].size, what
            assert dense(got.groups, want[0].size, what) == list(zip(*[w.tolist() for w in want])), what
    assert not stats, stats                                         # no clamp was hit


def test_on_groups_of_ascending_inputs_the_clamped_expansion_is_the_pairs():
    rng = np.random.default_rng(7)
    for trial in range(60):
        n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        distinct = (1, 2, 5, 50)[trial % 4]
        a, b = np.sort(rng.integers(0, distinct, n).astype(np.uint32)), np.sort(rng.integers(0, distinct, m).astype(np.uint32))
        g = J.groups(a, b, E.U32)
        G, total = g[0].size, J.total(g)
        pos_a, pos_b = rng.permutation(n) + 1000, rng.permutation(m) + 2000
        for th, per in ((2, 2), (4, 4), (64, 1)):
            for cap in (0, 1, th * per, total - 1 if total else 0, total, total + 5):
                for positions in (False, True):
                    slack = int(rng.integers(0, 3))                 # groups_cap above the number of groups: junk behind the last one
                    cols = [np.r_[c, rng.integers(0, 1 << 62, slack, dtype=np.uint64)].tolist() for c in g[1:]]
                    got = J.expand_clamped(G, G + slack, *cols, n, m, pos_a if positions else None, pos_b if positions else None, cap, th, per)
                    ia, ib = J.pairs(g, 0, cap)
                    stored = min(total, cap)
                    what = (a.tolist(), b.tolist(), th, per, cap, positions)
                    assert got.total == total, what
                    assert dense(got.out_a, stored, what) == (pos_a[ia.astype(np.int64)] if positions else ia).tolist(), what
                    assert dense(got.out_b, stored, what) == (pos_b[ib.astype(np.int64)] if positions else ib).tolist(), what


# ---- inputs in any order: every read inside its array (the models assert it), every store inside the promised range

@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
def test_search_of_unsorted_keys_and_needles_stores_inside_d_out(tile, right):
    rng = np.random.default_rng(tile)
    for a, b in unsorted_inputs(100 + tile):
        n, m = a.size, b.size
        for positions in (None, rng.permutation(m)):
            out = S.tiles_clamped(a, b, tile, right, positions)
            assert out.indices() <= set(range(m)), (a.tolist(), b.tolist())
            assert all(0 <= v <= n for vs in out.at.values() for v in vs), (a.tolist(), b.tolist())


@pytest.mark.parametrize("tile", TILES)
def test_merge_of_unsorted_inputs_stores_inside_the_outputs(tile):
    for a, b in unsorted_inputs(200 + tile):
        n, m = a.size, b.size
        for junk, first, got in S.variants(lambda junk, first: M.tiles_clamped(a, b, tile, junk, first)):
            what = (a.tolist(), b.tolist(), junk, first)
            for stores in (got.out, got.vals, got.origin):
                assert stores.indices() == set(range(n + m)), what                  # inside, and every cell: a slice is never cut short
                assert all(len(v) == 1 for v in stores.at.values()), what           # the tiles' slices are disjoint
            assert all(0 <= v[0] < n + m for v in got.origin.at.values()), what
            assert all(0 <= v[0] < n + m for v in got.vals.at.values()), what       # (the index in [A; B] of the value loaded)


def caps_of(count):
    return (None, count - 1, 1, 0) if count else (None, 0, 1)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("op", X.OPS, ids=[X.OP_NAMES[op] for op in X.OPS])
def test_set_operations_on_unsorted_inputs_store_inside_the_window(tile, op):
    for at, (a, b) in enumerate(unsorted_inputs(300 + 10 * tile + op)):
        n, m = a.size, b.size
        counted = X.tiles_clamped(a, b, tile, op, 0)[0].tile_counts    # (a cap of 0: the count alone)
        count = sum(counted)
        for cap in (caps_of(count) if at % 8 == 0 or n + m <= 6 else (None,)):          # (the four caps on the small pairs and every eighth random one)
            for junk, first, got in S.variants(lambda junk, first: X.tiles_clamped(a, b, tile, op, cap, junk, first, counted=counted)):
                what = (a.tolist(), b.tolist(), cap, junk, first)
                stored = count if cap is None else min(count, cap)
                assert got.count == count, what                     # the count kernel has no race and reads no junk
                assert got.out.indices() == set(range(stored)) and got.origin.indices() == set(range(stored)), what    # inside, and every cell
                assert all(len(v) == 1 for v in got.out.at.values()), what          # the tiles' windows are disjoint
                assert all(0 <= v[0] < n + m for v in got.origin.at.values()), what


@pytest.mark.parametrize("tile", TILES)
def test_groups_of_unsorted_inputs_store_inside_the_window(tile):
    for at, (a, b) in enumerate(unsorted_inputs(400 + tile)):
        n, m = a.size, b.size
        counted = J.tiles_clamped(a, b, tile, 0)[0].tile_counts
        count = sum(counted)
        for cap in (caps_of(count) if at % 8 == 0 or n + m <= 6 else (None,)):          # (the four caps on the small pairs and every eighth random one)
            for junk, first, got in S.variants(lambda junk, first: J.tiles_clamped(a, b, tile, cap, junk, first, counted=counted)):
                what = (a.tolist(), b.tolist(), cap, junk, first)
                stored = count if cap is None else min(count, cap)
                assert got.count == count and got.groups.indices() == set(range(stored)), what
                for (_, af, ac, bf, bc), in got.groups.at.values():
                    assert ac >= 1 and af + ac <= n and bc >= 0 and bf + bc <= m, what


def made_up_groups(rng, groups_cap, n, m):
    """groups this library did not write: counts of 0, counts up to 2^63 (the products wrap), firsts beyond n and m"""
    def column(small):
        kind = rng.integers(0, 4, groups_cap)
        x = rng.integers(0, small + 1, groups_cap, dtype=np.uint64)
        x[kind == 1] = 0
        big = rng.integers(0, 1 << 63, groups_cap, dtype=np.uint64, endpoint=True)
        x[kind == 2] = big[kind == 2]
        return x.tolist()
    return column(n + 3), column(4), column(m + 3), column(4)


@pytest.mark.parametrize("th,per", [(2, 2), (4, 4), (64, 2)])
def test_pairs_of_made_up_groups_store_inside_the_outputs(th, per):
    rng = np.random.default_rng(th)
    PT = th * per
    most_trips = 0
    for trial in range(1500):
        n, m = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        groups_cap = int(rng.integers(0, 9)) if trial % 3 else int(rng.integers(60, 200))
        num_groups = (0, groups_cap // 2, groups_cap, groups_cap + 3, 1 << 40)[trial % 5]      # below and above groups_cap
        a_first, a_count, b_first, b_count = made_up_groups(rng, groups_cap, n, m)
        if trial % 4 == 0:                                          # small products: a total that is around the caps
            a_count, b_count = [x % 4 for x in a_count], [x % 3 for x in b_count]
        positions = trial % 2 == 1
        pos_a, pos_b = (10000 + rng.permutation(n), 20000 + rng.permutation(m)) if positions else (None, None)
        G = min(num_groups, groups_cap)
        total = sum(p * q for p, q in zip(a_count[:G], b_count[:G])) & S.MASK64
        for cap in (0, 1, PT - 1, PT, PT + 1, 3 * PT + 1, 1 << 62):
            got = J.expand_clamped(num_groups, groups_cap, a_first, a_count, b_first, b_count, n, m, pos_a, pos_b, cap, th, per)
            what = (trial, n, m, groups_cap, num_groups, cap)
            assert got.total == total, what
            stored = min(total, cap)
            assert got.out_a.indices() <= set(range(min(stored, -(-min(cap, n * m) // PT) * PT))), what     # (the grid is that of min(cap, n * m) ranks)
            assert got.out_a.indices() == got.out_b.indices(), what
            if positions:                                           # ia < n and ib < m were clamped before a position was loaded
                assert all(10000 <= v[0] < 10000 + n for v in got.out_a.at.values()), what
                assert all(20000 <= v[0] < 20000 + m for v in got.out_b.at.values()), what
            most_trips = max(most_trips, got.trips)
    assert 2 <= most_trips <= J.search_trips_bound(200)


def test_the_64_ary_search_ends_for_arbitrary_offsets():
    """the offsets are wrapping sums: not ascending.  [lo, hi) shrinks every trip, and the first group stays below G."""
    assert [J.search_trips_bound(G) for G in (0, 1, 64, 65, 4096, 1 << 28)] == [0, 1, 1, 2, 2, 5]
    rng = np.random.default_rng(5)
    for trial in range(300):
        G = int(rng.integers(1, 400))
        a_count = rng.integers(0, 1 << 63, G, dtype=np.uint64, endpoint=True).tolist()
        b_count = rng.integers(0, 1 << 63, G, dtype=np.uint64, endpoint=True).tolist()
        first = rng.integers(0, 5, G).tolist()
        got = J.expand_clamped(G, G, first, a_count, first, b_count, 5, 5, None, None, 25, 4, 2)     # (the model asserts trips and g0 < G)
        assert got.out_a.indices() <= set(range(25))


# ---- the vectorised models that the GPU tests compare with are the statement-by-statement models

@pytest.mark.parametrize("tile", TILES)
def test_the_vectorised_models_are_the_index_checked_ones(tile):
    """search_expect.stored_clamped against tiles_clamped (the multiset of (index, value) stores, both rules, with and without
    positions) and set_expect.count_np against count_clamped (the tile counts of the four operations; the intersection's are
    those of the groups call) on inputs in any order: what tests/test_gpu_untrusted_order.py compares the GPU with at the real
    tile is what the index-checked models say"""
    rng = np.random.default_rng(500 + tile)
    for a, b in unsorted_inputs(500 + tile):
        what = (a.tolist(), b.tolist(), tile)
        for right in (False, True):
            for positions in (None, rng.permutation(b.size)):
                out = S.tiles_clamped(a, b, tile, right, positions)
                index, value = S.stored_clamped(a, b, tile, right, positions)
                assert sorted(zip(index.tolist(), value.tolist())) == sorted((i, v) for i, vs in out.at.items() for v in vs), (what, right, positions)
        A, B = S.Checked(a, "a"), S.Checked(b, "b")
        splits = S.Checked(S.split_points(A.x, B.x, tile, True)[0], "splits")
        for op in X.OPS:
            assert X.count_np(a, b, tile, op) == X.count_clamped(A, B, splits, tile, X.KEEP_MASK[op]), (what, op)

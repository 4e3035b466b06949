"""The block tables of tests/test_gpu_every_alignment_lag.py hold what that file claims (no GPU needed): every (own, tap) pair of
instantiations an element size allows, every byte count of lag_base's zeroed head at each pair, every last-unit count at each
(alignment, lag), the clamp edges, the wide merge's four-element accesses at every alignment, both parities of every tap, the
restore pass's cut words — and numpy's inverse of numpy's transform is the identity on a sample of each table, so the references
stand on their own feet.  The element side of a block lies `a` elements behind a multiple of 64 bytes in an image that starts at
a multiple of 16, so its address mod 16 is a * k.  Thinning a table fails here."""
import numpy as np
import pytest

import test_gpu_every_alignment_lag as eal
import test_gpu_fields as fld
import test_gpu_planes_grid as grd
import test_gpu_planes_grid_hist as hst
import test_gpu_planes_lag as lag
from test_gpu_every_alignment import shift_class

ELEMS = eal.ELEMS


def _multiples(k):
    return set(range(0, 16, k))


def test_class_functions():
    for A in range(16):
        assert eal.own(0x7F0000 + A) == (A // 4, A % 4)
        for k in ELEMS:
            for D in (1, 2, 3, 5, 16, 17, 4097, 1 << 40, eal.TOP):
                assert eal.tap(0x7F0000 + A, D, k) == eal.own((A - D * k) % 16), (A, D, k)
    for k in ELEMS:
        assert list(eal.aligns(k)) == list(range(16 // k)) and {a * k for a in eal.aligns(k)} == _multiples(k)
        assert len(eal.all_pairs(k)) == (16 // k) ** 2
    # the instantiations the families' own layouts (0, 1 or 3 elements behind a multiple of 64) never reached
    ran = {k: {eal.own(a * k)[0] for a in (0, 1, 3)} for k in ELEMS}
    assert ran == {1: {0}, 2: {0, 1}, 4: {0, 1, 3}, 8: {0, 2}}
    assert eal.subset_dists((2, 3, 5), 9) == [(2, 1), (3, 1), (5, 1), (5, 0), (7, 0), (8, 0)]
    assert eal.subset_dists((1, 300), 300) == [(1, 1)] and eal.subset_dists((), 50) == []


@pytest.mark.parametrize("k", ELEMS)
def test_lag_small_has_every_pair_head_and_tail(k):
    blocks = eal._lag_small(k)
    assert len(blocks) == 4096 // k and max(n for n, _, _ in blocks) == 32 and all(1 <= D < n for n, D, _ in blocks)
    taps = [(a * k, D) for n, D, a in blocks]
    assert {(eal.own(A), eal.tap(A, D, k)) for A, D in taps} == eal.all_pairs(k)
    # at each pair every D mod 16 that goes with it: zb = (D - e0) k bytes of the head are zeroed, whole dwords and, at one and
    # two bytes, a part of one
    heads = {(eal.own(A), eal.tap(A, D, k), D % 16) for A, D in taps}
    assert heads == {(eal.own(A), eal.tap(A, D, k), D % 16) for A in _multiples(k) for D in range(16)} and len(heads) == 256 // k
    assert {(D * k) % 4 for _, D in taps} == ({0} if k >= 4 else {0, 2} if k == 2 else {0, 1, 2, 3})
    for a in eal.aligns(k):
        for D in range(1, 17):
            assert {n % 16 for n, d, b in blocks if (d, b) == (D, a)} == set(range(16)), (k, a, D)
    eal._assert_pairs(taps, k)
    eal._assert_heads(taps, k)


def test_lag_edges_clamp_on_every_side(shafa):
    for k in ELEMS:
        whole = eal._lag_blocks(shafa, k)
        caps = eal._caps([n for n, _, _ in whole])
        lo = len(eal._lag_small(k))
        edges = eal._lag_edges(k)
        assert whole[lo:lo + len(edges)] == edges and len(edges) == 21 * (16 // k)
        for a in eal.aligns(k):
            mine = [(n, D) for n, D, b in edges if b == a]
            want = [(n, D) for n in (1, 15, 16, 17, 33) for D in (n - 1, n, n + 1, n + 2) if D >= 1]
            want += [(17, 1 << 40), (17, eal.TOP)]
            assert mine == want, (k, a)
        rows = [(n, D, a, c) for (n, D, a), c in zip(edges, caps[lo:])]
        assert {c - n for n, _, _, c in rows} == {0, 1, 2}
        assert any(D == n - 1 for n, D, _, _ in rows)                      # the last element alone has a base
        assert any(n <= D < c for n, D, _, c in rows)                      # between the size and the capacity: unclamped
        assert any(D == n == c for n, D, _, c in rows) and any(D > c for n, D, _, c in rows)        # clamped to the capacity
        # ... and a lag that reaches the kernel at or past the size at every alignment the element size has
        assert {a for n, D, a, c in rows if n <= D} == set(eal.aligns(k)), k


def test_lag_large_taps_reach_other_passes_and_tiles(shafa):
    T = shafa.PLANES_TILE
    for k in ELEMS:
        blocks = eal._lag_large(k, T)
        assert len(blocks) == 21 * (16 // k)
        for a in eal.aligns(k):
            assert sorted((n, D) for n, D, b in blocks if b == a) == sorted(
                (n, D) for D in (eal.PASS - 1, eal.PASS, eal.PASS + 1, T - 1, T, T + 1, T + eal.PASS + 17)
                for n in (D + 1, D + 17, D + eal.PASS + 1)), (k, a)
        assert {D % 16 for _, D, _ in blocks} == {15, 0, 1}                 # the unit that holds element D: its last, first, second
        assert all(D < n for n, D, _ in blocks) and any(n - D > eal.PASS for n, D, _ in blocks)


def test_lag_wide_stores_at_every_alignment(shafa):
    strip = shafa.PLANES_LAG_STRIP
    assert strip == 256 and lag._geom(shafa, 1 << 20, strip)[1] == strip and lag._geom(shafa, 1 << 20, strip - 1)[1] == strip - 1
    for k in ELEMS:
        blocks = eal._lag_wide(k, strip)
        assert len(blocks) == 64 * (16 // k)
        assert {L % 16 for _, L, _ in blocks} == set(range(16)) and all(strip <= L < n for n, L, _ in blocks)
        assert max(n for n, _, _ in blocks) == 33 * (strip + 15) + 7
        assert any(lag._geom(shafa, n, L)[5] > 1 for n, L, _ in blocks)    # two chunks: the sums and their scan run
        for a in eal.aligns(k):
            mine = [(n, L) for n, L, b in blocks if b == a]
            assert mine == [(n, L) for L in range(strip, strip + 16) for n in (L + 1, 2 * L + 3, 8 * L + L // 2, 33 * L + 7)]
            at, rd, fours, tails = set(), set(), 0, 0
            for n, L in mine:
                four, tail = eal.wide_lanes(n, L)
                at |= set(((a * k + four * k) % 16).tolist())
                rd |= set((four % 4).tolist())
                fours, tails = fours + four.size, tails + tail.size
            # at every alignment of the block: a store at every multiple of k, a dword read of a plane at every residue mod 4
            assert at == _multiples(k) and rd == {0, 1, 2, 3} and fours and tails, (k, a)
    # the lanes of wide_lanes cover every element once
    for n, L in ((257, 256), (515, 257), (8957, 271), (2 * 259 + 3, 259)):
        four, tail = eal.wide_lanes(n, L)
        seen = np.zeros(n + 8, np.int64)
        for i in four:
            seen[i:i + 4] += 1
        for i in tail:
            r, c = divmod(int(i), L)
            for j in range(4):
                if c + j < L and i + j < n:
                    seen[i + j] += 1
        assert (seen[:n] == 1).all() and not seen[n:].any(), (n, L)


def test_grid_table_has_every_pair_on_both_sides(shafa):
    T, strip = shafa.PLANES_TILE, shafa.PLANES_LAG_STRIP
    sets = eal._grid_sets(shafa)
    assert sets[:11] == ((1, 2), (1, 3), (2, 3), (3, 5, 15), (1, 16), (15, 16, 17), (1, 4, 16), (2, 7, 11), (5, 8, 13), (6, 9, 14),
                         (4, 8, 12))
    wide = eal._wide_sets(strip)
    assert sets[11:] == wide and set(wide) == {(g, strip + j) for g in (1, 3) for j in range(4)} | {(2, strip + 1, 2 * strip + 3)}
    assert all(len(s) in (2, 3) and all(x < y for x, y in zip(s, s[1:])) for s in sets)
    for k in ELEMS:
        blocks = eal._grid_blocks(shafa, k)
        for s in sets:
            for a in eal.aligns(k):
                want = {1, 15, 16, 17, 33, max(s) + 1, sum(s) + 1, sum(s) + 17, T + 1} | ({33 * max(s) + 7} if s in wide else set())
                assert {n for n, t, b in blocks if (t, b) == (s, a)} == want, (k, s, a)
        taps = [(a * k, D, par) for n, s, a in blocks for D, par in eal.subset_dists(s, n)]
        assert {(eal.own(A), eal.tap(A, D, k)) for A, D, _ in taps} == eal.all_pairs(k), k
        assert {(eal.tap(A, D, k), par) for A, D, par in taps} == {(eal.own(A), par) for A in _multiples(k) for par in (0, 1)}, k
        # every tap instantiation on both sides at every alignment of the own unit, too
        tap_qs = {eal.own(B)[0] for B in _multiples(k)}
        assert {(A, eal.tap(A, D, k)[0], par) for A, D, par in taps} >= {(A, q, par) for A in _multiples(k) for q in tap_qs
                                                                         for par in (0, 1)}, k
        # the difference merge's blocks and the lag merge's at every alignment, in one table
        for first_is_1 in (True, False):
            assert {a for n, s, a in blocks if (s[0] == 1) == first_is_1 and n > s[0]} == set(eal.aligns(k)), k
        # the passes in place at a wide lag: four-element accesses at every multiple of k, the four-wide path and its tail
        for a in eal.aligns(k):
            at, tails = set(), 0
            for n, s, b in blocks:
                for g in s[1:]:
                    if b == a and strip <= g < n:
                        four, tail = eal.wide_lanes(n, g)
                        at |= set(((a * k + four * k) % 16).tolist())
                        tails += tail.size
            assert at == _multiples(k) and tails, (k, a)
        caps = eal._caps([n for n, _, _ in blocks])
        assert {c - n for c, (n, _, _) in zip(caps, blocks)} == {0, 1, 2}


def test_hist_table(shafa):
    T = shafa.PLANES_TILE
    sets = eal._grid_sets(shafa) + ((),)
    assert eal.CANDS == [(), (1,), (64,), (4096,), (1, 64), (1, 4096), (64, 4096), (1, 64, 4096)]
    for k in ELEMS:
        rows = eal._hist_rows(shafa, k)
        own_rows = [r for r in rows if r[0] != T + 21]
        assert sorted((n, s, a) for n, s, a, _ in own_rows) == sorted((n, s, a) for s in sets for a in eal.aligns(k)
                                                                       for n in (1, 15, 16, 17, 33, T + 1))
        assert len({reg for _, _, _, reg in own_rows}) == len(own_rows)   # a region each
        assert {a for n, s, a, _ in rows if s == () and n == T + 1} == set(eal.aligns(k))          # plain: no difference, no fold
        for a in eal.aligns(k):
            shared = [(s, reg) for n, s, b, reg in rows if b == a and n == T + 21]
            assert [s for s, _ in shared] == eal.CANDS and len({reg for _, reg in shared}) == 1, (k, a)
        assert len({reg for n, _, _, reg in rows if n == T + 21}) == 16 // k
        taps = [(a * k, D, par) for n, s, a, _ in rows for D, par in eal.subset_dists(s, n)]
        assert {(eal.own(A), eal.tap(A, D, k)) for A, D, _ in taps} == eal.all_pairs(k), k
        assert {(eal.tap(A, D, k), par) for A, D, par in taps} == {(eal.own(A), par) for A in _multiples(k) for par in (0, 1)}, k


@pytest.mark.parametrize("k", eal.FIELD_ELEMS)
def test_quant_table_cut_words_and_outliers(shafa, k):
    T = shafa.PLANES_TILE
    blocks = eal._quant_blocks(shafa, k)
    counts = set(range(18)) | {33, T - 1, T, T + 1, 2 * T + 3}
    assert len(blocks) == (16 // k) * 5 * 23
    for a in eal.aligns(k):
        for s in ((1,), (3,), (1, 3), (2, 3, 5), (1, 16, T)):
            assert {n for n, t, b, _, _ in blocks if (t, b) == (s, a)} == counts, (k, a, s)
    # steps and bounds: test_gpu_fields._blocks' five steps in turn and its bound
    ref = fld._blocks(shafa, k)
    assert [b[3] for b in blocks[:5]] == [b[3] for b in ref[:5]] and {b[3] for b in blocks} == {b[3] for b in ref}
    assert all(bound == fld._exact(step * (0.5 + 2.0 ** -6), k) for _, _, _, step, bound in blocks)
    # the restore pass's cut words
    assert {eal.cut_words(a * k, n, k) for n, _, a, _, _ in blocks} == {(A, B) for A in _multiples(k) for B in _multiples(k)}
    assert any(0 < n * k < 16 and a * k + n * k <= 16 for n, _, a, _, _ in blocks)      # inside one 16-byte word, not all of it
    assert {a for n, _, a, _, _ in blocks if a and n > T} == set(eal.aligns(k)) - {0}   # a cut word two tiles share
    taps = [(a * k, D, par) for n, s, a, _, _ in blocks for D, par in eal.subset_dists(s, n)]
    assert {(eal.own(A), eal.tap(A, D, k)) for A, D, _ in taps} == eal.all_pairs(k)
    assert {(eal.tap(A, D, k), par) for A, D, par in taps} == {(eal.own(A), par) for A in _multiples(k) for par in (0, 1)}
    # the model leaves outliers at a block's first and last element, which _values plants, at every alignment and end
    ends = set()
    for b, (n, s, a, step, bound) in enumerate(blocks):
        if not n:
            continue
        x = fld._values(n, k, step, T, 10100 + k + b)
        code, xr, good = fld._model(x, step, bound)
        assert not good[0] and not good[-1], (k, n, a)
        ends.add(eal.cut_words(a * k, n, k))
        # numpy's inverse of numpy's transform on the codes
        if b % 7 == 0:
            planes = grd._z_planes(code.tobytes(), k, s)
            assert grd._x_bytes(planes, k, s) == code.tobytes(), (k, n, s)
    assert len(ends) == (16 // k) ** 2


@pytest.mark.parametrize("k", ELEMS)
def test_the_references_invert_themselves(shafa, k):
    """numpy's inverse of numpy's transform is the identity on a sample of every table (the layouts assert it for every block
    when they are built on the GPU machine)"""
    rng = np.random.default_rng(k)
    for n, D, a in eal._lag_blocks(shafa, k)[::41]:
        raw = lag._random(n, k, rng)
        assert lag._x_bytes(lag._z_planes(raw, k, D), k, D) == raw, (n, D)
    for n, s, a in eal._grid_blocks(shafa, k)[::29]:
        raw = lag._random(n, k, rng)
        assert grd._x_bytes(grd._z_planes(raw, k, s), k, s) == raw, (n, s)
    for n, s, a, _ in eal._hist_rows(shafa, k)[::53]:
        raw = lag._random(n, k, rng)
        c = hst._counts(raw, k, s)
        assert c.shape == (k, 256) and (c.sum(1) == n).all(), (n, s)
    # one lag a block is the grid reference's one-lag case
    raw = lag._random(300, k, rng)
    assert grd._z_planes(raw, k, (7,)).tobytes() == lag._z_planes(raw, k, 7).tobytes()
    assert shift_class(5, "split") == eal.own(5)

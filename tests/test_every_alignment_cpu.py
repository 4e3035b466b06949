"""The block tables of tests/test_gpu_every_alignment.py hold what that file claims (no GPU needed): every start alignment meets
every end the element size allows, every (element, base) pair has a base, every width, alignment and count is there, and
shift_class names 16 instantiation classes for either kind.  Thinning a table fails here."""
import numpy as np
import pytest

import pkgload
import test_gpu_every_alignment as ea
import test_gpu_planes_diff as dif


def _pairs(blocks, k):
    """(start mod 16, end mod 16) of regions of n elements of k bytes"""
    return {(a, (a + n * k) % 16) for n, a, *_ in blocks}


def test_shift_classes():
    split = {sh: ea.shift_class(0x7F0000 + sh, "split") for sh in range(16)}
    merge = {sh: ea.shift_class(0x7F0000 + sh, "merge") for sh in range(16)}
    assert split == {sh: (sh // 4, sh % 4) for sh in range(16)}
    # merge: the shift is 16 - sh, and sh = 0 is Q = 4 — planes_merge's `switch (sh == 0 ? 4u : m >> 2)`
    assert merge[0] == (4, 0) and merge[1] == (3, 3) and merge[4] == (3, 0) and merge[9] == (1, 3) and merge[12] == (1, 0)
    assert merge[13] == (0, 3) and merge[15] == (0, 1)
    for kind, got in (("split", split), ("merge", merge)):
        assert len(set(got.values())) == 16 and set(got.values()) == ea.all_classes(kind)
    assert {q for q, _ in merge.values()} == {0, 1, 2, 3, 4} and (0, 0) not in merge.values()
    assert {r for _, r in merge.values()} == {r for _, r in split.values()} == {0, 1, 2, 3}
    # the classes the short lists of the families' own files never reached
    assert {merge[sh][0] for sh in (0, 1, 3, 5, 7, 8, 15)} == {0, 2, 3, 4}
    assert {split[sh][0] for sh in (0, 1, 15)} == {0, 3}


def test_plane_tables_reach_every_start_and_end(shafa):
    T = shafa.PLANES_TILE
    blocks = ea._plane_blocks(T)
    assert len(blocks) == 672 and sum(n for n, _ in blocks) == 16 * 66119
    assert {n for n, _ in blocks} >= set(range(34)) | {ea.PASS - 1, ea.PASS, ea.PASS + 1, T - 1, T, T + 1, T + ea.PASS + 17, 2 * T + 5}
    for k in ea.ELEMS:
        small = [(n, a) for n, a in blocks if n <= 33]
        assert _pairs(small, k) == {(a, (a + k * j) % 16) for a in range(16) for j in range(16 // k)}, k
        # each of these ends after one, two and three units' worth of elements too
        for lo, hi in ((1, 16), (17, 32)):
            assert _pairs([(n, a) for n, a in small if lo <= n <= hi], k) == _pairs(small, k), (k, lo)
    for a in range(16):                                                    # every large count at every alignment
        assert sum(1 for n, b in blocks if b == a and n >= ea.PASS - 1) == 8
    caps = ea._caps([n for n, _ in blocks])
    assert {c - n for c, (n, _) in zip(caps, blocks)} == {0, 1, 2}
    # the merge's second alignment is a permutation with no fixed point that changes the byte part and the dword part
    assert sorted((a + 9) % 16 for a in range(16)) == list(range(16))


def test_xor_table_has_every_pair_with_a_base(shafa):
    T = shafa.PLANES_TILE
    blocks = ea._xor_blocks(T)
    assert len(blocks) == 256 * 4 + 46 * 3
    assert [b for b, (_, _, ab) in enumerate(blocks) if ab is None] == list(range(6, len(blocks), 7))
    allp = {(a, ab) for a in range(16) for ab in range(16)}
    based = [(n, a, ab) for n, a, ab in blocks if ab is not None]
    assert {(a, ab) for _, a, ab in based} == allp
    for p in allp:                                                         # at most one of a pair's four small counts lost its base
        assert sum(1 for n, a, ab in based if (a, ab) == p and n <= 33) >= 3, p
    large = [(n, a, ab) for n, a, ab in blocks if n >= ea.PASS]
    assert len(large) == 138 and {n for n, _, _ in large} == {ea.PASS, ea.PASS + 1, T + 1}
    # the LDS pass (both sides 16-aligned, or no base) and the direct path, with and without a base
    assert any(a == 0 and ab == 0 for _, a, ab in large) and any(a == 0 and ab is None for _, a, ab in large)
    assert any(a == 0 and ab not in (0, None) for _, a, ab in large) and any(a != 0 and ab == 0 for _, a, ab in large)
    assert len({a for _, a, ab in large if ab == a}) >= 12                  # a = ab: the two sides shift alike
    for k in ea.ELEMS:
        assert {(a, (a + n * k) % 16) for n, a, _ in blocks if n <= 33} == \
            {(a, (a + n * k) % 16) for a in range(16) for n in (1, 16, 17, 33)}, k


def test_record_tables_have_every_width_alignment_and_count(shafa):
    records = pkgload.load_submodule("records")
    assert ea.WIDTHS == tuple(range(1, shafa.RECORDS_MAX_WIDTH + 1))
    for w in ea.WIDTHS:
        P = records.records_pass(w)
        blocks = ea._record_blocks(P)
        assert sorted(blocks) == sorted((n, a) for a in range(16) for n in (1, 15, 16, 17, P + 1)), w
        assert _pairs(blocks, w) == {(a, (a + n * w) % 16) for a in range(16) for n in (1, 15, 16, 17, P + 1)}, w
        if w % 2:                                                          # an odd width: the ends a + w, a - w and a
            assert all(len({e for s, e in _pairs(blocks, w) if s == a}) == 3 for a in range(16)), w
    # over the widths every start meets every end
    assert {p for w in ea.WIDTHS for p in _pairs(ea._record_blocks(records.records_pass(w)), w)} == \
        {(a, e) for a in range(16) for e in range(16)}


def test_find_tables():
    assert ea.FIND_M == (1, 3, 4, 5, 17, 255) and ea.FIND_TILE == 8192 and ea.BORDERS == (32, 2048, 8192)
    for m in ea.FIND_M:
        table = ea._find_regions(m)
        assert {n for n, _ in table} == {m, m + 1, 33, 2049, 8193}, m
        assert [a for _, a in table] == list(range(16)) * (len(table) // 16), m     # region i at alignment i mod 16
        for n, a in table:
            fit = [s for s in ea._find_starts(n, m, a) if 0 <= s and s + m <= n]
            assert n < m or {0, n - m} <= set(fit), (m, n, a)
        if m >= 2:                                                         # the last start of these sizes straddles each border
            for n, B in ((33, 32), (2049, 2048), (8193, 8192)):
                assert n < m or n - m < B < n, (m, n)


@pytest.mark.parametrize("k", ea.ELEMS)
def test_diff_data_wraps_and_carries(k):
    """the three kinds of data of the differences' sweep are what they say"""
    rng = np.random.default_rng(k)
    U, M = dif.UINT[k], 1 << (8 * k)
    for n in (0, 1, 33):
        for b in range(3):
            assert len(ea._diff_data(b, n, k, rng)) == n * k
    wraps = 0
    for _ in range(8):
        walk = [int(x) for x in np.frombuffer(ea._diff_data(1, 33, k, rng), U)]
        assert walk[0] == M - 3
        wraps += sum(1 for x, y in zip(walk, walk[1:]) if abs(x - y) > M // 2)
    assert wraps >= 8, k
    assert {int(x) for x in np.frombuffer(ea._diff_data(2, 4096, k, rng), U)} == {0, 1, M // 2 - 1, M // 2, M - 1}
    first = np.frombuffer(ea._diff_data(0, 33, k, rng), U)[0]
    assert int(first) >= M // 2
    # numpy's inverse of numpy's transform on each kind: the reference stands on its own feet
    for b in range(3):
        raw = ea._diff_data(b, 33, k, rng)
        assert dif._x_bytes(dif._z_planes(raw, k), k) == raw

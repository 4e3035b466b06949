"""The lagged plane kernels (csrc/planes_lag.hip: lagged differences, Lorenzo differences, their histograms, the error-bounded
quantiser) at every element alignment and every tap alignment, against numpy on the host; nothing is compared with device code.

Their split side is planes.hip's word-shifting direct path run twice a unit.  The lane's OWN unit goes through load_words /
shift_into<E, Q, false> at sh = address mod 16, Q = sh >> 2 a template parameter and r = sh & 3 a run-time byte shift: own(A).
Every TAP unit goes through lag_base, which reads the region "moved up by dist elements" at an alignment of its own,
(address - dist E) mod 16, with a switch, read guards and a byte mask (the zb bytes in front of element dist) of its own:
tap(A, dist).  The element side lies at multiples of E, so a * E for a in range(16 / E) is every alignment there is.  The
families' own files place the element side 0, 1 or 3 elements behind a multiple of 64 bytes, never crossed with the lag or the
count; here every alignment meets every lag residue and every count residue, every (own, tap) pair occurs, and every test
asserts over the real device addresses that the classes its table promises do.  Merge's wide form (lag_store4, lag_d4, lag_src4:
four elements or a dword of each plane at the element's alignment) and the restore pass's cut words are swept the same way.

The references, the 0xA5 images compared WHOLE and the guards are the families' own (test_gpu_planes_lag._Layout,
test_gpu_planes_grid._Layout, test_gpu_planes_grid_hist._Blocks / _counts, test_gpu_fields._Layout / _model).  All blocks of one
(family, element size) go through ONE launch per direction.  The tables are plain functions of the tile, pass and strip sizes,
so tests/test_every_alignment_lag_cpu.py checks without a GPU that they hold what they claim."""
import itertools

import numpy as np
import pytest

import test_gpu_fields as fld
import test_gpu_planes_grid as grd
import test_gpu_planes_grid_hist as hst
import test_gpu_planes_lag as lag
from test_gpu_every_alignment import _batch, _dn, _once, _same_image, all_classes, shift_class
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
FIELD_ELEMS = (4, 8)
PASS = 4096                                                                # the elements of one pass of a planes workgroup
TOP = (1 << 64) - 1
SMALL = (1, 15, 16, 17, 33)
GRID_SETS = ((1, 2), (1, 3), (2, 3), (3, 5, 15), (1, 16), (15, 16, 17), (1, 4, 16), (2, 7, 11), (5, 8, 13), (6, 9, 14), (4, 8, 12))
CANDS = hst.CANDS                                                          # eight candidate rows on one region


# ---------------------------------------------------------------- the instantiations an address and a distance select
def own(A):
    """(Q, r) of the lane's own unit: load_words / shift_into<E, Q, false> of the region at address A"""
    return shift_class(A, "split")


def tap(A, D, k):
    """(Q, r) of lag_base's switch for a tap at distance D: the region at A moved up by D elements of k bytes"""
    return shift_class(A - D * k, "split")


def aligns(k):
    """the element side's alignments in ELEMENTS: a * k is every multiple of k below 16"""
    return range(16 // k)


def all_pairs(k):
    """every (own, tap) pair an element size allows: (16 / k)^2"""
    return {(own(A), own(B)) for A in range(0, 16, k) for B in range(0, 16, k)}


def subset_dists(lags, n):
    """(dist, parity) of the taps of a block of n elements: the sums of the non-empty subsets of its lags below n (a lag at or
    past the capacity is no lag; a distance at or past n has no element behind it)"""
    out = []
    for r in range(1, len(lags) + 1):
        for sub in itertools.combinations(lags, r):
            if sum(sub) < n:
                out.append((sum(sub), r & 1))
    return out


def wide_lanes(n, L):
    """lag_merge_wide over a block of n elements at lag L >= PLANES_LAG_STRIP: the first index i of every four-element access
    (lag_d4 / lag_src4 / lag_store4: `whole && i + 4 <= n`) and of every lane and row that goes element by element instead"""
    rows = -(-n // L)
    col0 = np.arange(0, L, 4, dtype=np.int64)                              # strip0 + 4 cl over all strips
    i = np.arange(rows, dtype=np.int64)[:, None] * L + col0[None, :]
    four = (col0 + 4 <= L)[None, :] & (i + 4 <= n)
    return i[four], i[~four & (i < n)]


def cut_words(A, n, k):
    """(start mod 16, end mod 16) of a region of n elements at address A: the restore pass's cut words"""
    return (A % 16, (A + n * k) % 16)


# ---------------------------------------------------------------- the block tables (no GPU needed: test_every_alignment_lag_cpu.py)
def _caps(ns):
    return [n + (b % 3) for b, n in enumerate(ns)]


def _lag_small(k):
    """table 1, (n, D, a): every alignment, every lag 1 .. 16, the sixteen counts behind it: every (own, tap) pair, every byte
    count zb of the zeroed head at each, every last-unit count c = 1 .. 16 at each (a, D)"""
    return [(n, D, a) for a in aligns(k) for D in range(1, 17) for n in range(D + 1, D + 17)]


def _lag_edges(k):
    """table 2: a lag just below, at and past the size; with capacities n + b % 3 a lag between the size and the capacity reaches
    the kernel unclamped"""
    out = []
    for a in aligns(k):
        for n in SMALL:
            out += [(n, D, a) for D in (n - 1, n, n + 1, n + 2) if D >= 1]
        out += [(17, 1 << 40, a), (17, TOP, a)]
    return out


def _lag_large(k, T):
    """table 3: the tap's unit lies in another pass or another tile, the unit that holds element D at every position in a lane"""
    return [(n, D, a) for a in aligns(k) for D in (PASS - 1, PASS, PASS + 1, T - 1, T, T + 1, T + PASS + 17)
            for n in (D + 1, D + 17, D + PASS + 1)]


def _lag_wide(k, strip):
    """table 4: merge's wide form at every L mod 16; L mod 4 != 0 gives the lane whose four columns are not all the row's"""
    return [(n, L, a) for a in aligns(k) for L in range(strip, strip + 16) for n in (L + 1, 2 * L + 3, 8 * L + L // 2, 33 * L + 7)]


def _lag_blocks(shafa, k):
    T, strip = shafa.PLANES_TILE, shafa.PLANES_LAG_STRIP
    return _lag_small(k) + _lag_edges(k) + _lag_large(k, T) + _lag_wide(k, strip)


def _wide_sets(strip):
    """the lag sets whose further passes run in place over the elements in the wide form (lag_src4)"""
    return tuple((g, strip + j) for g in (1, 3) for j in range(4)) + ((2, strip + 1, 2 * strip + 3),)


def _grid_sets(shafa):
    return GRID_SETS + _wide_sets(shafa.PLANES_LAG_STRIP)


def _grid_blocks(shafa, k):
    """table 5, (n, lags, a): every lag set at every alignment and count"""
    T, wide = shafa.PLANES_TILE, _wide_sets(shafa.PLANES_LAG_STRIP)
    out = []
    for s in _grid_sets(shafa):
        counts = SMALL + (max(s) + 1, sum(s) + 1, sum(s) + 17, T + 1) + ((33 * max(s) + 7,) if s in wide else ())
        out += [(n, s, a) for a in aligns(k) for n in counts]
    return out


def _hist_rows(shafa, k):
    """table 6, (n, lags, a, region): the grid table's sets and a plain candidate at the small counts and T + 1, every row a
    region of its own, and at every alignment eight candidate rows on ONE region"""
    T = shafa.PLANES_TILE
    rows = [(n, s, a) for s in _grid_sets(shafa) + ((),) for a in aligns(k) for n in SMALL + (T + 1,)]
    rows = [r + (i,) for i, r in enumerate(rows)]
    first = len(rows)
    for a in aligns(k):
        rows += [(T + 21, c, a, first + a) for c in CANDS]
    return rows


def QUANT_SETS(T):
    return ((1,), (3,), (1, 3), (2, 3, 5), (1, 16, T))


def _quant_blocks(shafa, k):
    """table 7, (n, lags, a, step, bound): steps and bounds as test_gpu_fields._blocks gives them"""
    T = shafa.PLANES_TILE
    counts = tuple(range(18)) + (33, T - 1, T, T + 1, 2 * T + 3)
    steps = [2.0 ** -10, fld._exact(1e-3, k), fld._exact(0.37, k), 3.0, fld._exact(1e-7, k)]
    out = []
    for b, (a, s, n) in enumerate((a, s, n) for a in aligns(k) for s in QUANT_SETS(T) for n in counts):
        step = steps[b % len(steps)]
        out.append((n, s, a, step, fld._exact(step * (0.5 + 2.0 ** -6), k)))
    return out


# ---------------------------------------------------------------- what a table promises, over addresses
def _assert_own(addrs, k):
    want = {own(A) for A in range(0, 16, k)}
    got = {own(p) for p in addrs}
    assert got == want and want <= all_classes("split"), (k, sorted(want - got))


def _assert_pairs(taps, k):
    """taps: (address, distance) of every tap that subtracts or adds something"""
    got = {(own(p), tap(p, D, k)) for p, D in taps}
    assert len(all_pairs(k)) == (16 // k) ** 2 and got == all_pairs(k), (k, sorted(all_pairs(k) - got))


def _assert_heads(taps, k):
    """at every (own, tap) pair every D mod 16 that goes with it: the sixteen byte counts of the zeroed head, at E = 1 and 2
    the partial dword among them"""
    got = {(own(p), tap(p, D, k), D % 16) for p, D in taps}
    want = {(own(A), tap(A, D, k), D) for A in range(0, 16, k) for D in range(16)}
    assert len(want) == 256 // k and got >= want, (k, sorted(want - got)[:8])


def _assert_wide(addr_el, addr_pl, blocks, k, strip):
    """lag_store4's (and lag_src4's) four-element accesses lie at every multiple of k mod 16, lag_d4's dword reads of a plane at
    every residue mod 4 (addr_pl None: a pass in place, no plane is read), and both the four-wide path and its tail occur"""
    at, rd, tails = set(), set(), 0
    for b, (p, (n, L, _)) in enumerate(zip(addr_el, blocks)):
        if L < strip or L >= n:
            continue
        four, tail = wide_lanes(n, L)
        at |= set(((p + four * k) % 16).tolist())
        if addr_pl is not None:
            rd |= set(((addr_pl[b] + four) % 4).tolist())
        tails += tail.size
    assert at == set(range(0, 16, k)) and tails, (k, sorted(at), tails)
    assert addr_pl is None or rd == {0, 1, 2, 3}, (k, sorted(rd))


# ---------------------------------------------------------------- 1, 2. lagged differences: tables 1 to 4 in one launch
def _lag(shafa, k):
    blocks = _lag_blocks(shafa, k)
    return blocks, _once(("lag sweep", k), lambda: lag._Layout(k, blocks, 9800 + k))


@pytest.mark.parametrize("k", ELEMS)
def test_lag_split(shafa, k):
    blocks, L = _lag(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_el, d_pl = lag._to(L.el), lag._fill(L.pl.size)
        addr = [d_el.data_ptr() + o for o in L.off]
        assert [p % 16 for p in addr] == [a * k for _, _, a in blocks] and d_pl.data_ptr() % 16 == 0
        taps = [(p, D) for p, (n, D, _) in zip(addr, blocks) if D < n]
        _assert_own(addr, k)
        _assert_pairs(taps, k)
        _assert_heads(taps[:len(_lag_small(k))], k)                        # table 1 alone holds them all
        bt.split_planes_lag_dev(st, k, L.lag, d_el, L.off, _caps(L.n), _dn(L.n), d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"lag split, E = {k}, planes; blocks are (n, lag, a)")
        _same_image(d_el, L.el, L.off, 1, blocks, f"lag split, E = {k}, the input; blocks are (n, lag, a)")
    finally:
        bt.close()


@pytest.mark.parametrize("k", ELEMS)
def test_lag_merge(shafa, k):
    blocks, L = _lag(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_n, cap = _dn(L.n), _caps(L.n)
        for name, pl, el in (("numpy's planes", L.pl, L.el), ("random planes", L.zpl, L.zel)):
            d_pl, d_out = lag._to(pl), lag._fill(el.size)
            addr = [d_out.data_ptr() + o for o in L.off]
            assert [p % 16 for p in addr] == [a * k for _, _, a in blocks] and d_pl.data_ptr() % 16 == 0
            _assert_own(addr, k)
            _assert_wide(addr, [d_pl.data_ptr() + o for o in L.poff[::k]], blocks, k, shafa.PLANES_LAG_STRIP)
            bt.merge_planes_lag_dev(st, k, L.lag, d_pl, L.poff, cap, d_n, d_out, L.off)
            assert bt.finish(st, nb) == (0, [0] * nb), k
            _same_image(d_out, el, L.off, 1, blocks, f"lag merge of {name}, E = {k}, elements; blocks are (n, lag, a)")
            _same_image(d_pl, pl, L.poff, k, blocks, f"lag merge of {name}, E = {k}, the input; blocks are (n, lag, a)")
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. Lorenzo differences: table 5
def _grid(shafa, k):
    blocks = _grid_blocks(shafa, k)
    return blocks, _once(("grid sweep", k), lambda: grd._Layout(k, blocks, 9900 + k))


def _grid_taps(addr, blocks):
    return [(p, D, par) for p, (n, s, _) in zip(addr, blocks) for D, par in subset_dists(s, n)]


def _assert_grid_classes(addr, blocks, k):
    assert [p % 16 for p in addr] == [a * k for _, _, a in blocks]
    taps = _grid_taps(addr, blocks)
    _assert_own(addr, k)
    _assert_pairs([(p, D) for p, D, _ in taps], k)
    # every tap instantiation on sub_words' side (an odd subset) and on add_words' (an even one)
    sides = {(tap(p, D, k), par) for p, D, par in taps}
    assert sides == {(own(A), par) for A in range(0, 16, k) for par in (0, 1)}, k


@pytest.mark.parametrize("k", ELEMS)
def test_grid_split(shafa, k):
    blocks, L = _grid(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_el, d_pl = lag._to(L.el), lag._fill(L.pl.size)
        assert d_pl.data_ptr() % 16 == 0
        _assert_grid_classes([d_el.data_ptr() + o for o in L.off], blocks, k)
        bt.split_planes_grid_dev(st, k, L.lags, d_el, L.off, _caps(L.n), _dn(L.n), d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"grid split, E = {k}, planes; blocks are (n, lags, a)")
        _same_image(d_el, L.el, L.off, 1, blocks, f"grid split, E = {k}, the input; blocks are (n, lags, a)")
    finally:
        bt.close()


@pytest.mark.parametrize("k", ELEMS)
def test_grid_merge(shafa, k):
    """blocks whose smallest lag is 1 (the difference merge's) and blocks whose smallest lag is not (the lag merge's first pass)
    in the SAME launch: each family skips the other's blocks, at every alignment"""
    blocks, L = _grid(shafa, k)
    nb = len(blocks)
    strip = shafa.PLANES_LAG_STRIP
    st, bt = _batch(shafa, nb)
    try:
        d_n, cap = _dn(L.n), _caps(L.n)
        for name, pl, el in (("numpy's planes", L.pl, L.el), ("random planes", L.zpl, L.zel)):
            d_pl, d_out = lag._to(pl), lag._fill(el.size)
            addr = [d_out.data_ptr() + o for o in L.off]
            assert [p % 16 for p in addr] == [a * k for _, _, a in blocks] and d_pl.data_ptr() % 16 == 0
            for first_is_1 in (True, False):                               # both families at every alignment
                mine = [p for p, (n, s, _) in zip(addr, blocks) if (s[0] == 1) == first_is_1 and n > s[0]]
                assert {p % 16 for p in mine} == set(range(0, 16, k)), (k, first_is_1)
            assert {shift_class(p, "merge") for p, (n, s, _) in zip(addr, blocks) if s[0] == 1} == \
                {shift_class(A, "merge") for A in range(0, 16, k)}, k         # the difference merge's own shift
            # the passes in place at a wide lag: lag_src4 / lag_store4 at every multiple of k
            wide = [(p, (n, g, a)) for p, (n, s, a) in zip(addr, blocks) for g in s[1:] if g >= strip]
            _assert_wide([w[0] for w in wide], None, [w[1] for w in wide], k, strip)
            bt.merge_planes_grid_dev(st, k, L.lags, d_pl, L.poff, cap, d_n, d_out, L.off)
            assert bt.finish(st, nb) == (0, [0] * nb), k
            _same_image(d_out, el, L.off, 1, blocks, f"grid merge of {name}, E = {k}, elements; blocks are (n, lags, a)")
            _same_image(d_pl, pl, L.poff, k, blocks, f"grid merge of {name}, E = {k}, the input; blocks are (n, lags, a)")
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. the histograms: table 6
class _HistLayout:
    """table 6 laid out: one region per distinct region number (test_gpu_planes_grid_hist._Blocks places it and fills the
    guards), one block per row, `want` the whole count buffer, guards included"""

    def __init__(self, k, rows, seed):
        rng = np.random.default_rng(seed)
        regions = {}
        for n, _, a, reg in rows:
            assert regions.setdefault(reg, (n, a)) == (n, a)
        raws = {reg: lag._random(n, k, rng) for reg, (n, a) in regions.items()}
        order = list(regions)
        B = hst._Blocks(k, [(raws[reg], (), regions[reg][1]) for reg in order])
        place = dict(zip(order, B.off))
        self.k, self.nb, self.el = k, len(rows), B.el
        self.n, self.lags, self.off = [r[0] for r in rows], [tuple(r[1]) for r in rows], [place[r[3]] for r in rows]
        self.want = np.full(2 * hst.GUARD + self.nb * k * 256, hst.A5, np.uint64)
        self.foff = [(hst.GUARD + b * k * 256) * 8 for b in range(self.nb)]
        for b, (n, lags, a, reg) in enumerate(rows):
            self.want[hst.GUARD + b * k * 256:hst.GUARD + (b + 1) * k * 256] = hst._counts(raws[reg], k, lags).reshape(-1)


@pytest.mark.parametrize("k", ELEMS)
def test_grid_histograms(shafa, k):
    import torch
    rows = _hist_rows(shafa, k)
    L = _once(("hist sweep", k), lambda: _HistLayout(k, rows, 10000 + k))
    blocks = [r[:3] for r in rows]
    nb = len(rows)
    st, bt = _batch(shafa, nb)
    try:
        d_el = lag._to(L.el)
        whole, d_freq = hst._freq(nb * k)
        addr = [d_el.data_ptr() + o for o in L.off]
        _assert_grid_classes(addr, blocks, k)
        assert {own(p) for p, (n, s, _) in zip(addr, blocks) if s == ()} == {own(A) for A in range(0, 16, k)}       # plain rows
        shared = [p for p, r in zip(addr, rows) if r[0] == shafa.PLANES_TILE + 21]
        assert {own(p) for p in shared} == {own(A) for A in range(0, 16, k)} and len(shared) == 8 * len(set(shared))
        bt.hist_planes_grid_dev(st, k, L.lags, d_el, L.off, _caps(L.n), _dn(L.n), d_freq)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(whole.view(torch.uint8), L.want.view(np.uint8), L.foff, 1, blocks,
                    f"grid histograms, E = {k}, d_freq as bytes ({k} x 256 int64 a block); blocks are (n, lags, a)")
        _same_image(d_el, L.el, L.off, 1, blocks, f"grid histograms, E = {k}, the input; blocks are (n, lags, a)")
    finally:
        bt.close()


# ---------------------------------------------------------------- 5, 6. the quantiser: table 7
def _quant(shafa, k):
    blocks = _quant_blocks(shafa, k)
    return blocks, _once(("quant sweep", k), lambda: fld._Layout(shafa, k, blocks, 10100 + k))


def _record_places(ns):
    """every block has room for all its elements; two guard records in front, one behind every block"""
    ooff, pos = [], 2
    for n in ns:
        ooff.append(pos)
        pos += n + 1
    return ooff, pos


def _assert_cut_words(addr, blocks, k, T):
    """the restore pass's cut words: every (start, end) pair mod 16 the element size allows, a block inside one 16-byte word, and
    a cut word that two tiles share (a tile border inside a word)"""
    got = {cut_words(p, n, k) for p, (n, *_) in zip(addr, blocks)}
    assert got == {(A, B) for A in range(0, 16, k) for B in range(0, 16, k)}, k
    assert any(0 < n * k < 16 and p % 16 + n * k <= 16 for p, (n, *_) in zip(addr, blocks)), k
    assert any(n > T and (p + T * k) % 16 for p, (n, *_) in zip(addr, blocks)), k


@pytest.mark.parametrize("k", FIELD_ELEMS)
def test_quant_split(shafa, k):
    blocks, L = _quant(shafa, k)
    show = [b[:3] for b in blocks]
    nb = len(blocks)
    found = [len(r) for r in L.rec]
    ooff, room = _record_places(L.n)
    st, bt = _batch(shafa, nb)
    try:
        d_el, d_pl, d_outl, d_cnt = lag._to(L.el), lag._fill(L.pl.size), fld._fill64(2 * room), fld._fill64(nb + 2)
        addr = [d_el.data_ptr() + o for o in L.off]
        assert d_pl.data_ptr() % 16 == 0
        _assert_grid_classes(addr, show, k)
        bt.split_planes_grid_quant_dev(st, k, L.lags, L.step, L.bound, d_el, L.off, _caps(L.n), _dn(L.n), d_pl, L.poff, d_outl, ooff,
                                       L.n, d_cnt[1:nb + 1])
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_pl, L.pl, L.poff, k, show, f"quantising split, E = {k}, planes; blocks are (n, lags, a)")
        _same_image(d_el, L.el, L.off, 1, show, f"quantising split, E = {k}, the input; blocks are (n, lags, a)")
        cnt = d_cnt.tolist()
        bad = [(show[b], cnt[b + 1], found[b]) for b in range(nb) if cnt[b + 1] != found[b]]
        assert not bad, f"quantising split, E = {k}: (block (n, lags, a), outliers counted, the model's) {bad[:4]}"
        assert cnt[0] == cnt[-1] == fld.FILL64 - (1 << 64)
        rec = fld._rec_img(d_outl)
        want = np.full_like(rec, fld.FILL64)
        for b in range(nb):
            rec[ooff[b]:ooff[b] + found[b]] = fld._sorted(rec[ooff[b]:ooff[b] + found[b]])
            want[ooff[b]:ooff[b] + found[b]] = L.rec[b]
            assert rec[ooff[b]:ooff[b] + found[b]].tobytes() == L.rec[b].tobytes(), \
                f"quantising split, E = {k}: records of block {show[b]}"
        assert rec.tobytes() == want.tobytes(), k
    finally:
        bt.close()


@pytest.mark.parametrize("k", FIELD_ELEMS)
def test_quant_merge(shafa, k):
    import torch
    blocks, L = _quant(shafa, k)
    show = [b[:3] for b in blocks]
    nb = len(blocks)
    found = [len(r) for r in L.rec]
    ooff, room = _record_places(L.n)
    recs = np.full((room, 2), fld.FILL64, np.uint64)
    for b in range(nb):
        recs[ooff[b]:ooff[b] + found[b]] = L.rec[b]
    st, bt = _batch(shafa, nb)
    try:
        d_pl, d_out = lag._to(L.pl), lag._fill(L.el.size)
        d_rec = lag._to(recs.view(np.int64).reshape(-1))
        addr = [d_out.data_ptr() + o for o in L.off]
        assert [p % 16 for p in addr] == [a * k for _, _, a, _, _ in blocks] and d_pl.data_ptr() % 16 == 0
        _assert_cut_words(addr, blocks, k, shafa.PLANES_TILE)
        bt.merge_planes_grid_quant_dev(st, k, L.lags, L.step, d_pl, L.poff, _caps(L.n), _dn(L.n), d_rec, ooff, found, d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_out, L.out, L.off, 1, show, f"quantising merge, E = {k}, elements; blocks are (n, lags, a)")
        _same_image(d_pl, L.pl, L.poff, k, show, f"quantising merge, E = {k}, the planes; blocks are (n, lags, a)")
        assert lag._img(d_rec.view(torch.uint8)) == recs.tobytes(), k
        L.within_bound(d_out.cpu().numpy())
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. the drivers on views t[j:] of one parent
INT_DTYPES = ("uint8", "int16", "int32", "int64")                           # one per element size
N0 = 3000


def _views(dtype, seed):
    """every view parent[j:], j in range(16 / itemsize), of one parent of `dtype`: a walk of small steps (its differences
    compress) -> (views, their raw bytes)"""
    import torch
    dt = getattr(torch, dtype)
    k = torch.empty((), dtype=dt).element_size()
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(-3, 4, N0 + 16), dtype=np.int64).astype(np.uint64).astype(lag.UINT[k])
    parent = torch.from_numpy(x.view(np.uint8).copy()).to(_dev()).view(dt)
    assert parent.data_ptr() % 16 == 0
    views = [parent[j:] for j in aligns(k)]
    assert [v.data_ptr() % 16 for v in views] == list(range(0, 16, k)) and all(v.is_contiguous() for v in views)
    return k, views, [x[j:].tobytes() for j in aligns(k)]


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_grid_and_strided_drivers_on_views(shafa, dtype):
    k, views, raws = _views(dtype, 10200)
    keep = [v.clone() for v in views]
    strip = shafa.PLANES_LAG_STRIP
    for lags in ((1, 37, strip + 44), (3, strip + 1)):                     # the difference merge first, the lag merge first
        cts = shafa.compress_grids(views, lags=lags)
        for v, ct, raw in zip(views, cts, raws):
            grd._check_item(shafa, v, ct, raw, lags)
        back = shafa.decompress_grids(cts)
        assert len(back) == len(views) and all(lag._same(b, kp) for b, kp in zip(back, keep)), (dtype, lags)
    sets = [(), (1,), (1, 37), (3, strip + 1), (2, 5, 11)]
    for v, raw in zip(views, raws):
        got = shafa.grid_histograms(v, sets).cpu().numpy().astype(np.uint64)
        assert got.tobytes() == np.stack([hst._counts(raw, k, c) for c in sets]).tobytes(), (dtype, v.data_ptr() % 16)
    for g in (7, strip + 3):
        cts = shafa.compress_strided(views, lag=g)
        for v, ct, raw in zip(views, cts, raws):
            lag._check_item(shafa, v, ct, raw, g)
        back = shafa.decompress_strided(cts)
        assert len(back) == len(views) and all(lag._same(b, kp) for b, kp in zip(back, keep)), (dtype, g)
    assert all(lag._same(v, kp) for v, kp in zip(views, keep)), dtype


@pytest.mark.parametrize("k", FIELD_ELEMS)
def test_field_drivers_on_views(shafa, k):
    import torch
    i = np.arange(N0 + 16, dtype=np.float64)
    x = (100 * np.sin(i / 23) + 0.01 * i).astype(fld.FLOAT[k])
    for j, at in enumerate((0, 1, 3, 1500, N0 + 15)):                      # NaNs of distinct payloads, in every view's head too
        x[at] = np.nan
        x.view(lag.UINT[k])[at] |= lag.UINT[k](0x100 + j)
    parent = torch.from_numpy(x.copy()).to(_dev())
    assert parent.data_ptr() % 16 == 0
    views = [parent[j:] for j in aligns(k)]
    assert [v.data_ptr() % 16 for v in views] == list(range(0, 16, k))
    keep = [v.clone() for v in views]
    err = 1e-2
    for lags in ((1, 37), (3, 300)):
        items = shafa.compress_fields(views, err, lags=lags)
        backs = shafa.decompress_fields(items)
        assert len(backs) == len(views)
        for v, it, b in zip(views, items, backs):
            assert it.step != 0.0 and it.lags == lags and b.dtype == v.dtype and b.shape == v.shape
            nan = torch.isnan(v)
            assert int(nan.sum()) >= 2 and set(torch.nonzero(nan).reshape(-1).tolist()) <= set(it.outlier_pos.cpu().tolist())
            assert torch.equal(fld._bits(b)[nan], fld._bits(v)[nan])      # the NaNs bit for bit
            assert float((b[~nan].double() - v[~nan].double()).abs().max()) <= it.bound <= err, (k, lags, v.data_ptr() % 16)
    assert all(torch.equal(fld._bits(v), fld._bits(kp)) for v, kp in zip(views, keep))

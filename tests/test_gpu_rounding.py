"""shafa_hipd_split_planes_grid_round_dev / shafa_hipd_merge_planes_grid_round_dev / shafa_hipd_hist_planes_grid_round_dev
(csrc/planes_lag.hip) and the drivers on top (shafa-cd_amd/rounding.py) against numpy on the host.  The rule (include/shafa_hip.h:
"Point-wise relative bounds") is restated here in numpy (_rule), one unsigned operation of the element's width per operation:
codes, restored bits and which elements are good are compared integer for integer; the planes are numpy's grid differences of the
codes (test_gpu_planes_grid._z_planes) and, on the device, split_planes_grid_dev's over the model's codes; the histograms are
np.bincount over those planes.

The shapes are the grid tests': a lane has 16 elements, a tile T = PLANES_TILE.  Every buffer holds 0xA5 where no data lies, and
every comparison is of whole images."""
import numpy as np
import pytest

from test_gpu_planes_grid import _z_planes
from test_gpu_planes_lag import FILL, UINT, _al16, _fill, _img, _sizes, _to
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

MANT = {"float16": 10, "bfloat16": 7, "float32": 23, "float64": 52}
ELEM = {"float16": 2, "bfloat16": 2, "float32": 4, "float64": 8}
FILL64 = int.from_bytes(bytes([FILL] * 8), "little")


def _rule(x, mant, keep):
    """the header's rule: x an array of unsigned bit patterns of the element's width -> (the codes as unsigned integers, x' as
    bits, good)"""
    U = x.dtype.type
    W = 8 * x.dtype.itemsize
    d = U(mant - keep)
    MAG, INF, MIN = U((1 << (W - 1)) - 1), U(((1 << (W - 1 - mant)) - 1) << mant), U(1 << mant)
    S, M = x >> U(W - 1), x & MAG
    if mant == keep:
        rn = M
    else:
        rn = (M + U((1 << (mant - keep - 1)) - 1) + ((M >> d) & U(1))) >> d
    R = np.where(M >= INF, M >> d, rn)
    code = np.where(S == 1, U(0) - R, R)
    neg = code >> U(W - 1)
    a = np.where(neg == 1, U(0) - code, code)
    back = (a << d) & MAG
    xr = (neg << U(W - 1)) | back
    good = np.where((M < MIN) | (M >= INF), back == M, back < INF)
    return code, xr, good


def _restored(x, xr, good):
    """what the merge leaves: x' for a good element, the element's own bits for an outlier"""
    return np.where(good, xr, x)


def _records(x, good):
    """the model's records, sorted: [count, 2] of {position, bits}"""
    pos = np.flatnonzero(~good)
    return np.stack([pos.astype(np.uint64), x[pos].astype(np.uint64)], 1).reshape(-1, 2)


def _to_bits(v, fmt):
    """float64 values -> the bit patterns of a format (bfloat16: float32 truncated, test data need not be rounded)"""
    if fmt == "bfloat16":
        return (v.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return v.astype({"float16": np.float16, "float32": np.float32, "float64": np.float64}[fmt]).view(UINT[ELEM[fmt]])


def _specials(fmt, keep):
    """the bit patterns the contract names: +-0, denormals with and without dropped bits, the smallest normal, exact ties with the
    kept LSB 0 and 1, a mantissa of all ones, the largest finite value, +-Inf, a NaN with payload in the kept bits only, one with
    payload in the dropped bits, one that would truncate to Inf"""
    mant, W = MANT[fmt], 8 * ELEM[fmt]
    d = mant - keep
    SIGN, INF, MIN = 1 << (W - 1), ((1 << (W - 1 - mant)) - 1) << mant, 1 << mant
    one = (INF >> 1) & ~(MIN - 1)                                          # the bits of 1.0
    half = (1 << d) >> 1
    even, odd = (one >> d) & ~1, (one >> d) | 1
    out = [0, SIGN, 1 << d if d < mant else 2, (1 << d) | half if d else 1, 3 | SIGN, MIN, MIN | half,
           (even << d) | half, (odd << d) | half, SIGN | (even << d) | half, SIGN | (odd << d) | half,
           one | (MIN - 1), SIGN | one | (MIN - 1), INF - 1, SIGN | (INF - 1), INF, SIGN | INF,
           INF | (MIN >> 1), SIGN | INF | (MIN >> 1), INF | (MIN >> 1) | 1, INF | 1, SIGN | INF | half if half else INF | 1]
    return [v for v in out]


def _values(n, fmt, keep, T_tile, seed):
    """n elements as bits: a ramp with a sine on it that walks over many binades with both signs, the specials sprinkled through
    it, and planted at the first and the last element, at 15 / 16 / 17 and across the tile border"""
    i = np.arange(n, dtype=np.float64)
    span = {"float16": 12, "bfloat16": 60, "float32": 60, "float64": 400}[fmt]
    v = (1.0 + 0.37 * np.sin(i / 11 + seed)) * 2.0 ** (span * np.sin(i / 301 + 0.1 * seed)) * np.where((i // 7) % 3 == 1, -1.0, 1.0)
    x = _to_bits(v, fmt).copy()
    U = x.dtype.type
    sp = _specials(fmt, keep)
    for j, v in enumerate(sp):
        x[5 + j + seed % 3:n:97] = U(v)
    for j, at in enumerate(sorted({0, n - 1, 15, 16, 17, T_tile - 1, T_tile, T_tile + 1})):
        if 0 <= at < n:
            x[at] = U(sp[(3 + 5 * j + seed) % len(sp)])
    return x


class _Layout:
    """blocks (n elements, tuple of lags, element side `a` ELEMENTS behind a multiple of 64 bytes, format, keep) of one element
    size in host images: `el` the element side, `codes` the model's codes in its place, `pl` numpy's planes of the codes' folded
    differences, `out` what the merge leaves, `rec` each block's sorted records, `freq` the planes' byte counts [nb * k * 256].
    All FILL where no data lies.  `xs`: the blocks' own bit patterns, for the tests that bring them."""

    def __init__(self, shafa, blocks, seed=0, xs=None):
        k = self.k = ELEM[blocks[0][3]]
        self.n, self.lags = [b[0] for b in blocks], [tuple(b[1]) for b in blocks]
        self.mant, self.keep = [MANT[b[3]] for b in blocks], [b[4] for b in blocks]
        self.off, self.poff, self.x = [], [], []
        pos, ppos = 0, 16
        for n, _, a, _, _ in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + a * k
            self.off.append(pos)
            pos += n * k
            for _ in range(k):
                self.poff.append(ppos)
                ppos += _al16(n) + 32
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.pl = np.full(ppos + 16, FILL, np.uint8)
        self.codes, self.out = self.el.copy(), self.el.copy()
        self.rec, self.good = [], []
        self.freq = np.zeros(len(blocks) * k * 256, np.uint64)
        for b, (n, lags, _, fmt, keep) in enumerate(blocks):
            assert ELEM[fmt] == k
            x = _values(n, fmt, keep, shafa.PLANES_TILE, seed + b) if xs is None else xs[b]
            assert x.dtype == UINT[k] and x.size == n
            code, xr, good = _rule(x, MANT[fmt], keep)
            sl = slice(self.off[b], self.off[b] + n * k)
            self.el[sl] = x.view(np.uint8)
            self.codes[sl] = code.view(np.uint8)
            self.out[sl] = _restored(x, xr, good).view(np.uint8)
            planes = _z_planes(code.tobytes(), k, lags)
            for j in range(k):
                self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = planes[j]
                self.freq[(b * k + j) * 256:(b * k + j + 1) * 256] = np.bincount(planes[j], minlength=256)
            self.x.append(x)
            self.rec.append(_records(x, good))
            self.good.append(good)


def _stream():
    import torch
    return torch.cuda.Stream(device=_dev())


def _fill64(n):
    """n int64 of FILL bytes"""
    import torch
    return torch.full((n * 8,), FILL, dtype=torch.uint8, device=_dev()).view(torch.int64)


def _rec_img(d_outl):
    return d_outl.cpu().numpy().view(np.uint64).reshape(-1, 2)


def _sorted(rec):
    return rec[np.argsort(rec[:, 0], kind="stable")]


def _u64img(t):
    return t.cpu().numpy().view(np.uint64)


def _all_three(shafa, L, cap, lag_rows=None):
    """one launch of split, of merge and of hist over the blocks of L on one batch, every buffer whole against the host images:
    the planes against numpy's and against split_planes_grid_dev over the model's codes, the counts and the sorted records, the
    merge's output from numpy's planes and the model's records, the histograms against np.bincount over the planes and the hist
    entry's outlier counts against the split's"""
    import torch
    k, nb = L.k, len(L.n)
    lags = L.lags if lag_rows is None else lag_rows
    found = [len(r) for r in L.rec]
    ooff, pos = [], 2                                                      # two guard records in front
    for n in L.n:
        ooff.append(pos)
        pos += n + 1                                                       # room for every element, one guard record behind
    st = _stream()
    bt = shafa.Batch(nb * k, 1 << 20)
    try:
        d_n = _sizes(L.n)
        d_el, d_pl, d_outl, d_cnt = _to(L.el), _fill(L.pl.size), _fill64(2 * pos), _fill64(nb + 2)
        assert d_el.data_ptr() % 16 == 0
        bt.split_planes_grid_round_dev(st, k, lags, L.mant, L.keep, d_el, L.off, cap, d_n, d_pl, L.poff, d_outl, ooff, L.n,
                                       d_cnt[1:nb + 1])
        # the form it replaces: the model's codes through the exact integer split
        d_codes, d_pl2 = _to(L.codes), _fill(L.pl.size)
        bt.split_planes_grid_dev(st, k, lags, d_codes, L.off, cap, d_n, d_pl2, L.poff)
        # the histograms without the planes
        d_freq, d_hcnt = _fill64(nb * k * 256 + 2), _fill64(nb + 2)
        bt.hist_planes_grid_round_dev(st, k, lags, L.mant, L.keep, d_el, L.off, cap, d_n, d_freq[1:-1], d_hcnt[1:nb + 1])
        assert bt.finish(st, nb) == (0, [0] * nb)
        got = d_pl.cpu().numpy()
        bad = [(b, L.n[b], L.lags[b], L.keep[b], L.mant[b]) for b in range(nb)
               if any(got[o:o + L.n[b]].tobytes() != L.pl[o:o + L.n[b]].tobytes() for o in L.poff[b * k:b * k + k])]
        assert not bad, bad[:8]
        assert got.tobytes() == L.pl.tobytes() == _img(d_pl2)
        assert _img(d_el) == L.el.tobytes()
        assert d_cnt.tolist() == [FILL64 - (1 << 64)] + found + [FILL64 - (1 << 64)]
        rec = _rec_img(d_outl)
        want = np.full_like(rec, FILL64)
        for b in range(nb):
            rec[ooff[b]:ooff[b] + found[b]] = _sorted(rec[ooff[b]:ooff[b] + found[b]])
            want[ooff[b]:ooff[b] + found[b]] = L.rec[b]
        assert rec.tobytes() == want.tobytes()
        hf = _u64img(d_freq)
        bad = [(b, L.n[b], L.lags[b]) for b in range(nb)
               if hf[1 + b * k * 256:1 + (b + 1) * k * 256].tobytes() != L.freq[b * k * 256:(b + 1) * k * 256].tobytes()]
        assert not bad, bad[:8]
        assert hf[0] == FILL64 and hf[-1] == FILL64 and hf[1:-1].tobytes() == L.freq.tobytes()
        assert d_hcnt.tolist() == d_cnt.tolist()
        # merge: numpy's planes and the model's records
        d_pl, d_out = _to(L.pl), _fill(L.el.size)
        d_rec = _to(want.view(np.int64).reshape(-1))
        bt.merge_planes_grid_round_dev(st, k, lags, L.mant, L.keep, d_pl, L.poff, cap, d_n, d_rec, ooff, found, d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        got = d_out.cpu().numpy()
        bad = [(b, L.n[b], L.lags[b], L.keep[b], L.mant[b]) for b in range(nb)
               if got[L.off[b]:L.off[b] + L.n[b] * k].tobytes() != L.out[L.off[b]:L.off[b] + L.n[b] * k].tobytes()]
        assert not bad, bad[:8]
        assert got.tobytes() == L.out.tobytes()
        assert _img(d_pl) == L.pl.tobytes() and _img(d_rec.view(torch.uint8)) == want.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 1. the kernels: one launch each over a table of blocks
def _blocks(shafa, k):
    T = shafa.PLANES_TILE
    counts = (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3)
    rows = [(1,), (3,), (1, 3), (2, 3, 5), (1, 16, T), None]               # None: a lag at the capacity, plain planes
    fmts = {2: ("bfloat16", "float16"), 4: ("float32",), 8: ("float64",)}[k]
    kinds = [(f, keep) for f in fmts for keep in (0, 1, MANT[f] // 2, MANT[f] - 1, MANT[f])]
    offs = tuple(range(8)) if k == 2 else (0, 1, 3)
    out = []
    for b, (s, n) in enumerate((s, n) for s in rows for n in counts):
        f, keep = kinds[(b + b // len(kinds)) % len(kinds)]
        out.append((n, s if s is not None else (n + 5,), offs[b % len(offs)], f, keep))
    return out


@pytest.mark.parametrize("k", (2, 4, 8))
def test_one_launch_each_against_the_model(shafa, k):
    blocks = _blocks(shafa, k)
    L = _Layout(shafa, blocks, 10 * k)
    assert sum(len(r) for r in L.rec) > 100
    # every alignment, format and keep is in the table, and every kind of outlier and of good special with both outcomes
    assert {b[2] for b in blocks} == set(range(8) if k == 2 else (0, 1, 3))
    assert {(b[3], b[4]) for b in blocks} == {(f, kp) for f in MANT if ELEM[f] == k for kp in (0, 1, MANT[f] // 2, MANT[f] - 1, MANT[f])}
    W = 8 * k
    kinds = set()
    for (n, _, _, f, keep), x, good in zip(blocks, L.x, L.good):
        INF, MIN, MAG = ((1 << (W - 1 - MANT[f])) - 1) << MANT[f], 1 << MANT[f], (1 << (W - 1)) - 1
        M = x.astype(np.uint64) & np.uint64(MAG)
        for name, sel in (("zero", M == 0), ("denormal", (M > 0) & (M < MIN)), ("normal", (M >= MIN) & (M < INF)), ("inf", M == INF),
                          ("nan", M > INF)):
            kinds |= {(name, bool(g)) for g in np.unique(good[sel])}
    assert kinds == {("zero", True), ("denormal", True), ("denormal", False), ("normal", True), ("normal", False), ("inf", True),
                     ("nan", True), ("nan", False)}
    _all_three(shafa, L, [n + 5 for n in L.n])


@pytest.mark.parametrize("k", (2, 4, 8))
def test_block_borders_inside_a_run(shafa, k):
    """test_gpu_field_hist's test of the same name for the rounding histogram: sixty-four blocks of 100 .. 3000 elements, a tile
    each and so eight to a run, alternately all outliers and clean, neighbours at different keeps: a count flushed to the wrong
    block, or a counter not cleared at a border, shows in the neighbour.  An outlier here is a NaN whose lowest mantissa bit is
    set, at a keep below the mantissa's width: the bit is dropped, so the element does not come back (include/shafa_hip.h)"""
    rng = np.random.default_rng(900 + k)
    ns = rng.integers(100, 3001, 64).tolist()
    ns[0], ns[1], ns[-1] = 100, 3000, 3000
    nb = len(ns)
    rows = [(1,), (1, 7), (3,), (2, 3, 50)]
    fmts = {2: ("bfloat16", "float16"), 4: ("float32",), 8: ("float64",)}[k]
    blocks = [(n, rows[b % 4], (0, 1, 3)[b % 3], fmts[b // 2 % len(fmts)], 1 + b % 5) for b, n in enumerate(ns)]
    assert all(p[4] != q[4] and p[4] < MANT[p[3]] for p, q in zip(blocks, blocks[1:] + blocks[:1]))

    def nans(n, fmt):
        W, mant = 8 * k, MANT[fmt]
        inf = ((1 << (W - 1 - mant)) - 1) << mant
        sign = (np.arange(n) % 3 == 1).astype(UINT[k]) << UINT[k](W - 1)
        return sign | UINT[k](inf | 1) | ((np.arange(n) % 5).astype(UINT[k]) << UINT[k](mant - 1))        # quiet and signalling

    def clean(n, fmt):
        return _to_bits(np.arange(n) * 0.5 + 3 * np.sin(np.arange(n) / 5), fmt)

    # both ways round, so that every block is once behind a block of outliers and once in front of one
    for first in (0, 1):
        L = _Layout(shafa, blocks, xs=[nans(n, b[3]) if i % 2 == first else clean(n, b[3]) for i, (n, b) in enumerate(zip(ns, blocks))])
        found = [len(r) for r in L.rec]
        assert found == [n if b % 2 == first else 0 for b, n in enumerate(ns)]
        st = _stream()
        bt = shafa.Batch(nb * k, 1 << 20)
        try:
            d_n, d_el = _sizes(ns), _to(L.el)
            d_freq, d_hcnt = _fill64(nb * k * 256 + 2), _fill64(nb + 2)
            bt.hist_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_el, L.off, ns, d_n, d_freq[1:-1], d_hcnt[1:nb + 1])
            # device code against device code: the rounding split's planes through hist256, and the split's own counts
            d_pl, d_freq2, d_cnt = _fill(L.pl.size), _fill64(nb * k * 256 + 4), _fill64(nb + 2)
            bt.split_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_el, L.off, ns, d_n, d_pl, L.poff, None, [0] * nb, [0] * nb,
                                           d_cnt[1:nb + 1])
            bt.hist256(st, d_pl, L.poff, [n for n in ns for _ in range(k)], d_freq2[2:-2])
            assert bt.finish(st, nb * k) == (0, [0] * nb * k)
            assert d_hcnt.tolist() == [FILL64 - (1 << 64)] + found + [FILL64 - (1 << 64)] == d_cnt.tolist()
            hf = _u64img(d_freq)
            assert (hf[1:-1].reshape(nb, k, 256).sum(2) == np.array(ns, np.uint64)[:, None]).all()         # every plane's counts sum to n
            assert hf.tobytes() == _u64img(d_freq2)[1:-1].tobytes()
            assert hf[0] == FILL64 and hf[-1] == FILL64 and hf[1:-1].tobytes() == L.freq.tobytes()
            assert _img(d_el) == L.el.tobytes()
        finally:
            bt.close()


# ---------------------------------------------------------------- 2. exhaustive at 16 bits
def test_every_16_bit_pattern_at_every_keep(shafa):
    """all 65 536 bit patterns of bfloat16 and of float16, one block each per keep: 8 + 11 blocks in one launch of each of split,
    merge and hist"""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    rows = [(1,), (1, 256), (3,), (65536,)]
    blocks = [(65536, rows[i % 4], (0, 5, 2, 7)[i % 4], f, keep)
              for i, (f, keep) in enumerate((f, keep) for f in ("bfloat16", "float16") for keep in range(MANT[f] + 1))]
    assert len(blocks) == 8 + 11
    L = _Layout(shafa, blocks, xs=[x] * len(blocks))
    assert all(len(r) == 0 for b, r in zip(blocks, L.rec) if b[4] == MANT[b[3]]) and sum(len(r) for r in L.rec) > 1000
    _all_three(shafa, L, [65536] * len(blocks))


# ---------------------------------------------------------------- 3. capacities
@pytest.mark.parametrize("fmt", ("bfloat16", "float16", "float32", "float64"))
def test_capacities_below_the_outliers(shafa, fmt):
    """a block with no room and three outliers, one with room for two of its five: the counts are those found, the planes are
    complete, the two records written are two of the model's, nothing lies behind them"""
    k, mant = ELEM[fmt], MANT[fmt]
    keep = mant // 2
    W = 8 * k
    INF = ((1 << (W - 1 - mant)) - 1) << mant
    bad = [INF - 1, INF | 1, 1, (1 << (W - 1)) | (INF - 1), INF | (1 << (mant - 1)) | 1]
    xs = []
    for n, at in ((40, (0, 16, 39)), (50, (3, 15, 17, 31, 49))):
        x = _to_bits(np.arange(n) * 0.5 + 1, fmt).copy()
        x[list(at)] = np.array(bad[:len(at)], UINT[k])
        xs.append(x)
    L = _Layout(shafa, [(40, (1,), 0, fmt, keep), (50, (1, 3), 1, fmt, keep)], xs=xs)
    assert [len(r) for r in L.rec] == [3, 5]
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes(L.n)
        d_el, d_pl, d_outl, d_cnt = _to(L.el), _fill(L.pl.size), _fill64(2 * 6), _fill64(2)
        bt.split_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_el, L.off, L.n, d_n, d_pl, L.poff, d_outl, [1, 2], [0, 2], d_cnt)
        assert bt.finish(st, 2) == (0, [0, 0])
        assert d_cnt.tolist() == [3, 5]
        assert _img(d_pl) == L.pl.tobytes()
        rec = _rec_img(d_outl)
        assert rec[:2].tolist() == [[FILL64] * 2] * 2 and rec[4:].tolist() == [[FILL64] * 2] * 2
        mine = {tuple(r) for r in L.rec[1].tolist()}
        assert tuple(rec[2].tolist()) in mine and tuple(rec[3].tolist()) in mine and rec[2, 0] != rec[3, 0]
        # no record buffer at all where every capacity is 0
        d_pl = _fill(L.pl.size)
        bt.split_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_el, L.off, L.n, d_n, d_pl, L.poff, None, [0, 0], [0, 0], d_cnt)
        assert bt.finish(st, 2) == (0, [0, 0])
        assert d_cnt.tolist() == [3, 5] and _img(d_pl) == L.pl.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. a record past its block
@pytest.mark.parametrize("fmt", ("bfloat16", "float32", "float64"))
def test_a_record_at_the_blocks_size_is_refused(shafa, fmt):
    """three blocks; the middle one has a record at position n (and one inside): its code is OUTSIDE_MODULE, the record is not
    written — the element behind the block stays FILL — and its neighbours are right"""
    k, mant = ELEM[fmt], MANT[fmt]
    n = [33, 20, 17]
    L = _Layout(shafa, [(n[0], (1,), 0, fmt, 2), (n[1], (1, 3), 1, fmt, 3), (n[2], (2,), 3, fmt, mant)], 3)
    recs = [L.rec[0], np.array([[7, 0x3F80], [n[1], 0x1111]], np.uint64), L.rec[2]]
    want = L.out.copy()
    code, xr, good = _rule(L.x[1], mant, 3)
    img = xr.copy()                                                        # no outlier of its own is patched: only record 7
    img[7] = 0x3F80
    want[L.off[1]:L.off[1] + n[1] * k] = img.view(np.uint8)
    ooff, pos = [], 0
    for r in recs:
        ooff.append(pos)
        pos += len(r)
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes(n)
        d_pl, d_out = _to(L.pl), _fill(L.el.size)
        d_rec = _to(np.concatenate(recs).view(np.int64).reshape(-1))
        bt.merge_planes_grid_round_dev(st, k, L.lags, L.mant, L.keep, d_pl, L.poff, [c + 5 for c in n], d_n, d_rec, ooff,
                                       [len(r) for r in recs], d_out, L.off)
        assert bt.finish(st, 3, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [0, shafa.OUTSIDE_MODULE, 0])
        assert _img(d_out) == want.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. behind a busy stream
def test_behind_a_busy_stream_one_finish(shafa):
    """2^19 + 3 bfloat16 at lags (1, 64, 4096) and 2^18 + 1 doubles at (3, 4097), split and merged back behind a large torch
    kernel on the same stream: four launches on one batch, nothing synchronised in between, one finish"""
    import torch
    dev = _dev()
    cases = [("bfloat16", (1 << 19) + 3, (1, 64, 4096), 3, 3), ("float64", (1 << 18) + 1, (3, 4097), 1, 20)]
    Ls = [_Layout(shafa, [(n, g, a, f, keep)], 77) for f, n, g, a, keep in cases]
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_el = [_to(L.el) for L in Ls]
        d_pl = [_fill(L.pl.size) for L in Ls]
        d_out = [_fill(L.el.size) for L in Ls]
        d_outl = [_fill64(2 * c[1]) for c in cases]
        d_cnt = [_fill64(1) for _ in cases]
        found = [len(L.rec[0]) for L in Ls]
        half = torch.tensor([[c[1] // 2, c[1] - c[1] // 2] for c in cases], dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(st):
            busy = torch.empty(1 << 26, dtype=torch.float32, device=dev)
            busy.normal_()                                                 # 256 MiB written
            d_n = half.sum(dim=1)                                          # the sizes exist only behind it
            for i, (f, n, g, a, keep) in enumerate(cases):
                bt.split_planes_grid_round_dev(st, Ls[i].k, [g], Ls[i].mant, Ls[i].keep, d_el[i], Ls[i].off, [n], d_n[i:i + 1],
                                               d_pl[i], Ls[i].poff, d_outl[i], [0], [n], d_cnt[i])
            for i, (f, n, g, a, keep) in enumerate(cases):                 # the records where the split puts them, all the model's
                bt.merge_planes_grid_round_dev(st, Ls[i].k, [g], Ls[i].mant, Ls[i].keep, d_pl[i], Ls[i].poff, [n], d_n[i:i + 1],
                                               d_outl[i], [0], [found[i]], d_out[i], Ls[i].off)
            assert bt.finish(st, 1) == (0, [0])
        for i, L in enumerate(Ls):
            assert d_cnt[i].tolist() == [found[i]] and found[i] > 8, cases[i]
            assert _sorted(_rec_img(d_outl[i])[:found[i]]).tobytes() == L.rec[0].tobytes(), cases[i]
            assert _img(d_pl[i]) == L.pl.tobytes(), cases[i]
            assert _img(d_out[i]) == L.out.tobytes(), cases[i]
    finally:
        bt.close()


# ---------------------------------------------------------------- 6. the drivers
INTT = {2: "int16", 4: "int32", 8: "int64"}
NAN_AT = (0, 70000, 131071)


def _field_bits(fmt):
    """DESIGN 7.28's [32, 64, 64] field in a format, flat, as bits (torch's own conversion), with three NaNs planted whose payload
    is in the low bits"""
    import torch
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.float64)
    f = 1000 * np.sin(x / 9) * np.cos(y / 13) * np.sin(z / 7 + 0.3)
    k = ELEM[fmt]
    bits = torch.from_numpy(f).to(getattr(torch, fmt)).reshape(-1).view(getattr(torch, INTT[k])).numpy().view(UINT[k]).copy()
    W, mant = 8 * k, MANT[fmt]
    INF = ((1 << (W - 1 - mant)) - 1) << mant
    for j, at in enumerate(NAN_AT):
        bits[at] = UINT[k](INF | (1 << (mant - 1)) | (1 + j))
    return bits


def _tensor(bits, fmt, shape=None):
    import torch
    k = ELEM[fmt]
    t = torch.from_numpy(bits.view({2: np.int16, 4: np.int32, 8: np.int64}[k]).copy()).to(_dev()).view(getattr(torch, fmt))
    return t if shape is None else t.reshape(shape)


def _bits(t):
    import torch
    return t.contiguous().view(getattr(torch, INTT[t.element_size()]))


def _np_bits(t):
    return _bits(t).cpu().numpy().reshape(-1).view(UINT[t.element_size()])


def _weights():
    """DESIGN 7.20's weight tensor: (randn(2^20, seed 1) * 0.02) as bfloat16"""
    import torch
    g = torch.Generator().manual_seed(1)
    return (torch.randn(1 << 20, generator=g) * 0.02).to(torch.bfloat16).to(_dev())


@pytest.mark.parametrize("fmt,keep", [("float32", 10), ("float64", 10), ("float16", 3), ("bfloat16", 3)])
def test_round_trip_of_the_field_and_it_pays(shafa, fmt, keep, capsys):
    import torch
    k, mant = ELEM[fmt], MANT[fmt]
    bits = _field_bits(fmt)
    t = _tensor(bits, fmt, (32, 64, 64))
    before = _np_bits(t).copy()
    code, xr, good = _rule(bits, mant, keep)
    assert np.flatnonzero(~good).tolist() == list(NAN_AT)
    lags = (1, 64, 4096)
    # one tensor, no coder
    planes, pos, pbits = shafa.round_field(t, keep, lags)
    assert planes.cpu().numpy().tobytes() == _z_planes(code.tobytes(), k, lags).tobytes()
    want = _records(bits, good)
    assert pos.dtype == pbits.dtype == torch.int64
    assert pos.cpu().numpy().astype(np.uint64).tolist() == want[:, 0].tolist()
    assert pbits.cpu().numpy().view(np.uint64).tolist() == want[:, 1].tolist()
    back = shafa.restore_rounded(planes, t.dtype, t.shape, lags, keep, pos, pbits)
    assert back.dtype == t.dtype and back.shape == t.shape
    assert _np_bits(back).tobytes() == _restored(bits, xr, good).tobytes()
    # the drivers
    items = shafa.compress_rounded(t, keep)
    again = shafa.compress_rounded(t, keep)
    it = items[0]
    assert type(it) is shafa.CompressedRounded and it.dtype == t.dtype and it.shape == tuple(t.shape) and it.lags == lags
    assert it.keep_bits == keep and it.outlier_pos.cpu().tolist() == list(NAN_AT)
    planes_bytes = sum(sum(int(x.numel()) for x in p.values()) if isinstance(p, dict) else int(p.numel()) for p in it.planes)
    assert it.nbytes == planes_bytes + (8 + k) * 3
    other = again[0]
    assert other.nbytes == it.nbytes and torch.equal(other.outlier_pos, it.outlier_pos) and torch.equal(other.outlier_bits, it.outlier_bits)
    back = shafa.decompress_rounded(items)[0]
    assert back.dtype == t.dtype and back.shape == t.shape and _np_bits(t).tobytes() == before.tobytes()
    assert _np_bits(back).tobytes() == _restored(bits, xr, good).tobytes()     # the NaNs bit for bit among them
    ok = torch.isfinite(t)
    rel = ((back[ok].double() - t[ok].double()).abs() / t[ok].double().abs().clamp_min(1e-300)).max()
    assert float(rel) <= 2.0 ** -(keep + 1)
    lossless = shafa.compress_grids(t, lags=lags)[0].nbytes
    with capsys.disabled():
        print(f"\n[rounding] {fmt} [32, 64, 64] keep {keep}: compress_rounded {it.nbytes} B, compress_grids {lossless} B, "
              f"raw {t.numel() * k} B, outliers 3")
    assert it.nbytes < lossless


def test_weights_without_differences_and_the_sizes(shafa, capsys):
    import torch
    w = _weights()
    bits = _np_bits(w)
    for keep in (3, 2):
        it = shafa.compress_rounded(w, keep, lags=())[0]
        assert it.lags == () and it.keep_bits == keep and it.outlier_pos.numel() == 0
        code, xr, good = _rule(bits, 7, keep)
        assert good.all()
        back = shafa.decompress_rounded(it)[0]
        assert _np_bits(back).tobytes() == xr.tobytes()
        with capsys.disabled():
            print(f"\n[rounding] bf16 weights 2^20 keep {keep} lags (): {it.nbytes} B of {w.numel() * 2}")
    lagged = shafa.compress_rounded(w, 3, lags=(1,))[0]
    plain = shafa.compress_rounded(w, 3, lags=())[0]
    with capsys.disabled():
        print(f"\n[rounding] bf16 weights keep 3: lags (1,) {lagged.nbytes} B, lags () {plain.nbytes} B")
    assert plain.nbytes < lagged.nbytes
    # rounded_sizes: noise wants no differences, the field wants some
    f = _tensor(_field_bits("float32"), "float32", (32, 64, 64))
    sizes = shafa.rounded_sizes([w, f], [3, 10])
    assert sizes[0][0][0] == () and len(sizes[1][0][0]) >= 1
    assert [e[0] for e in sizes[0]] != [] and all(e[2] == 0 for e in sizes[0]) and all(e[2] == 3 for e in sizes[1])
    assert sorted(e[0] for e in sizes[1]) == sorted(shafa.grids._subsets((1, 64, 4096)))
    # the model's sizes are those of the histograms: the numbers of outliers and rows that sum to numel
    freq, outl = shafa.rounded_histograms(f, [10, 10, 23], [(1, 64, 4096), (), (1,)])
    assert freq.sum(2).eq(f.numel()).all() and outl.tolist() == [3, 3, 0]
    code = _rule(_np_bits(f), 23, 10)[0]
    for row, g in ((0, (1, 64, 4096)), (1, ())):
        planes = _z_planes(code.tobytes(), 4, g)
        assert freq[row].cpu().numpy().tolist() == [np.bincount(planes[j], minlength=256).tolist() for j in range(4)]


def test_mixed_lists_and_the_fallback(shafa):
    import torch
    dev = _dev()
    f4 = _tensor(_field_bits("float32"), "float32", (32, 64, 64))[:3]
    f8 = _tensor(_field_bits("float64"), "float64", (32, 64, 64))[:2]
    h = _tensor(_field_bits("float16"), "float16")[:5000]
    b = _tensor(_field_bits("bfloat16"), "bfloat16")[1:4001]
    # a tensor of inexact denormals: every element an outlier, so it is kept lossless
    den = torch.arange(1, 3001, dtype=torch.int32, device=dev).mul(2).add(1).view(torch.float32)
    ts = [f4, den, f8, torch.empty((0, 4), dtype=torch.float16, device=dev), torch.tensor(2.5, dtype=torch.bfloat16, device=dev), h, b]
    keeps = [10, 5, 20, 3, 2, 4, 3]
    lags = [(1, 64, 4096), (1,), (1, 64), (1,), (), (1,), ()]
    items = shafa.compress_rounded(ts, keeps, lags=lags)
    assert [it.keep_bits for it in items] == [10, None, 20, 3, 2, 4, 3]
    assert [it.lags for it in items] == lags
    assert items[1].outlier_pos.numel() == 0
    ref = shafa.compress_grids(den, lags=(1,))[0]
    assert items[1].nbytes == ref.nbytes
    backs = shafa.decompress_rounded(items)
    for t, it, kp, bk in zip(ts, items, keeps, backs):
        assert bk.dtype == t.dtype and bk.shape == t.shape
        x = _np_bits(t)
        if it.keep_bits is None:
            assert _np_bits(bk).tobytes() == x.tobytes()
            continue
        code, xr, good = _rule(x, shafa.MANTISSA_BITS[t.dtype], kp)
        assert _np_bits(bk).tobytes() == _restored(x, xr, good).tobytes()
        assert it.outlier_pos.cpu().tolist() == np.flatnonzero(~good).tolist()
    assert float(backs[4]) == 2.5 and backs[3].numel() == 0
    # default lags are the axis lags
    it = shafa.compress_rounded(f4, 10)[0]
    assert it.lags == (1, 64, 4096)


def test_fit_keep_bits_and_rates(shafa):
    bits = _field_bits("float32")
    f = _tensor(bits, "float32", (32, 64, 64))
    rates = shafa.rounded_rates(f, [7, 10, 15])
    assert [r[0] for r in rates] == [7, 10, 15] and [r[2] for r in rates] == [3, 3, 3]
    assert rates[0][1] < rates[1][1] < rates[2][1]
    budget = rates[1][1] + 1
    keep = shafa.fit_keep_bits(f, budget, keeps=[7, 10, 15])
    assert keep == 10
    every = shafa.rounded_rates(f, list(range(24)))
    best = shafa.fit_keep_bits(f, budget)
    assert best == max(k for k, nb, no in every if nb <= budget and no <= shafa.fields.outlier_capacity(f.numel())) and best >= 10
    assert shafa.fit_keep_bits(f, 0) is None
    it = shafa.compress_rounded(f, best)[0]
    good = _rule(bits, 23, best)[2]
    assert it.keep_bits == best and int(it.outlier_pos.numel()) == int((~good).sum()) == 3
    # with () for lags, and for a 16-bit tensor
    h = _tensor(_field_bits("bfloat16"), "bfloat16")
    assert shafa.fit_keep_bits(h, 1 << 30, lags=()) == 7
    assert shafa.rounded_rates(h[:0], [1, 2]) == [(1, 0, 0), (2, 0, 0)]

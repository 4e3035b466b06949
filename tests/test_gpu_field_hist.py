"""shafa_hipd_hist_planes_grid_quant_dev (csrc/planes_lag.hip) and field_histograms / field_sizes / choose_field_lags / field_rates /
fit_abs_error on top against numpy on the host.  The rule (include/shafa_hip.h: "Error-bounded fields") is restated here in numpy
(_rule), one numpy operation in T per IEEE operation; the counts are np.bincount over the planes that
tests/test_gpu_planes_grid.py's numpy expectation (_z_planes) gives for the codes, the outlier counts the number of elements the
rule does not call good, the sizes those of tests/test_field_hist_cpu.py's model with the host's Module T.  Device code is
compared with device code where a test says so: hist256 over the planes of shafa_hipd_split_planes_grid_quant_dev, and that
entry's own count of outliers.

The shapes are the borders of the kernel: a lane has 16 elements, a tile T = PLANES_TILE, a workgroup a run of R = PLANES_HIST_RUN
tiles of the capacities.  d_freq and d_outl_n arrive filled with 0xA5 between guard words that must survive, and every comparison
is of the whole buffer."""
import functools

import numpy as np
import pytest

from test_field_hist_cpu import field_model, field_model_sizes, planted
from test_gpu_fields import _values
from test_gpu_planes_grid import _stream, _z_planes
from test_gpu_planes_lag import FILL, _al16, _fill, _img, _sizes, _to
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

FLOAT = {4: np.float32, 8: np.float64}
INT = {4: np.int32, 8: np.int64}
GUARD = 32                                                                 # int64 words on either side of the counts
A5 = int.from_bytes(bytes([FILL] * 8), "little")


def _torch():
    import torch
    return torch


def _rule(x, step, bound):
    """the header's rule: x a float32 or float64 array, step and bound Python floats exactly representable in its type -> (the
    codes as signed integers, which elements are good)"""
    k, T = x.dtype.itemsize, x.dtype.type
    inv = T(1.0 / step)                                                    # the double division, rounded to T once
    with np.errstate(all="ignore"):
        t = x * inv
        inside = np.abs(t) < T(2.0 ** (8 * k - 2))                         # false for a NaN
        code = np.where(inside, np.rint(t), T(0)).astype(INT[k])
        xr = code.astype(T) * T(step)
        if k == 4:
            miss = np.abs(x.astype(np.float64) - xr.astype(np.float64)) <= np.float64(bound)
        else:
            miss = np.abs(x - xr) <= T(bound)
    return code, inside & miss


def _counts(x, lags, step, bound):
    """([k, 256] counts of the planes of x's codes at this row of lags, the outliers)"""
    k = x.dtype.itemsize
    code, good = _rule(x, step, bound)
    planes = _z_planes(code.tobytes(), k, lags)
    return np.stack([np.bincount(planes[j], minlength=256) for j in range(k)]).astype(np.uint64), int((~good).sum())


def _exact(v, k):
    return float(FLOAT[k](v))


class _Blocks:
    """blocks (x, row of lags, element side `a` ELEMENTS behind a multiple of 64 bytes, step, bound) of floats of k bytes: `el` the
    host image of the element side, FILL where no data lies, `want` the whole count buffer and `outl` the whole buffer of
    outlier counts, guards included.  A block whose x is an int is the block of that index once more: the same region."""

    def __init__(self, k, blocks):
        self.k, self.nb = k, len(blocks)
        self.lags, self.step, self.bound = [tuple(b[1]) for b in blocks], [b[3] for b in blocks], [b[4] for b in blocks]
        self.n, self.off, self.x = [], [], []
        pos = 0
        for x, _, a, _, _ in blocks:
            if isinstance(x, int):
                self.off.append(self.off[x])
                self.x.append(self.x[x])
            else:
                assert x.dtype == FLOAT[k]
                pos = (pos + 16 + 63) // 64 * 64 + a * k
                self.off.append(pos)
                self.x.append(x)
                pos += x.size * k
            self.n.append(self.x[-1].size)
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.want = np.full(2 * GUARD + self.nb * k * 256, A5, np.uint64)
        self.outl = np.full(2 * GUARD + self.nb, A5, np.uint64)
        for b in range(self.nb):
            self.el[self.off[b]:self.off[b] + self.n[b] * k] = self.x[b].view(np.uint8)
            c, o = _counts(self.x[b], self.lags[b], self.step[b], self.bound[b])
            self.want[GUARD + b * k * 256:GUARD + (b + 1) * k * 256] = c.reshape(-1)
            self.outl[GUARD + b] = o

    def zero(self, b):
        self.want[GUARD + b * self.k * 256:GUARD + (b + 1) * self.k * 256] = 0
        self.outl[GUARD + b] = 0

    def found(self):
        return self.outl[GUARD:-GUARD].tolist()


def _guarded(words):
    """a buffer of int64: (the whole tensor, 0xA5 everywhere; the view the entry gets)"""
    whole = _fill((2 * GUARD + words) * 8).view(_torch().int64)
    return whole, whole[GUARD:GUARD + words]


def _u64img(t):
    return t.cpu().numpy().view(np.uint64)


def _check(B, whole_f, whole_o):
    got, got_o = _u64img(whole_f), _u64img(whole_o)
    w = B.k * 256
    bad = [(b, B.n[b], B.lags[b]) for b in range(B.nb)
           if got[GUARD + b * w:GUARD + (b + 1) * w].tobytes() != B.want[GUARD + b * w:GUARD + (b + 1) * w].tobytes()]
    assert not bad, bad[:8]
    assert got.tobytes() == B.want.tobytes()
    bad = [(b, B.n[b], int(got_o[GUARD + b]), int(B.outl[GUARD + b])) for b in range(B.nb) if got_o[GUARD + b] != B.outl[GUARD + b]]
    assert not bad, bad[:8]
    assert got_o.tobytes() == B.outl.tobytes()
    return got


def _run(shafa, B, cap, dn=None, want_codes=None, split=False):
    """one launch over the blocks of B, one finish; both whole buffers and the element side against the host images.  split: in
    the same launch sequence the quantising split into planes, hist256 over them and the split's own counts of outliers — device
    code against device code"""
    st = _stream()
    k, nb = B.k, B.nb
    bt = shafa.Batch(nb * k, 1 << 20)
    try:
        d_n = _sizes(B.n if dn is None else dn)
        d_el = _to(B.el)
        assert d_el.data_ptr() % 16 == 0
        whole_f, d_freq = _guarded(nb * k * 256)
        whole_o, d_outl_n = _guarded(nb)
        bt.hist_planes_grid_quant_dev(st, k, B.lags, B.step, B.bound, d_el, B.off, cap, d_n, d_freq, d_outl_n)
        if split:
            poff, pn, pos = [], [], 0
            for n in B.n:
                for _ in range(k):
                    poff.append(pos)
                    pn.append(n)
                    pos += _al16(n) + 16
            d_pl = _fill(pos + 16)
            whole_f2, d_freq2 = _guarded(nb * k * 256)
            whole_o2, d_outl_n2 = _guarded(nb)
            bt.split_planes_grid_quant_dev(st, k, B.lags, B.step, B.bound, d_el, B.off, cap, d_n, d_pl, poff, None, [0] * nb, [0] * nb,
                                           d_outl_n2)
            bt.hist256(st, d_pl, poff, pn, d_freq2)
        if want_codes is None:
            assert bt.finish(st, nb * k) == (0, [0] * nb * k)
        else:
            assert bt.finish(st, nb, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want_codes)
        got = _check(B, whole_f, whole_o)
        if split:
            assert _u64img(whole_f2).tobytes() == got.tobytes()
            assert _u64img(whole_o2).tobytes() == _u64img(whole_o).tobytes()
        assert _img(d_el) == B.el.tobytes()
        return got
    finally:
        bt.close()


# ---------------------------------------------------------------- 1. by hand
@pytest.mark.parametrize("k", (4, 8))
def test_eight_elements_worked_out_by_hand(shafa, k):
    """step 1/4, bound 1/8 + 1/64: x = 0.25 0.5 1.0 NaN 2.3 -0.75 3.1 4.0.  t = 1 2 4 NaN 9.2 -3 12.4 16, codes 1 2 4 0 9 -3 12 16;
    x' = .25 .5 1 0 2.25 -.75 3 4; |x - x'| = 0 0 0 - .05 0 .1 0: all good but the NaN, which has no code: one outlier.
    Lags (1,): d = 1 1 2 -4 9 -12 15 4, z = 2 2 4 7 18 23 30 8.  Lags (1, 3): (1 - S^3) of that: d = 1 1 2 -5 8 -14 19 -5,
    z = 2 2 4 9 16 27 38 9.  Plane 0 counts those, every other plane eight zeros."""
    x = np.array([0.25, 0.5, 1.0, np.nan, 2.3, -0.75, 3.1, 4.0], FLOAT[k])
    step, bound = 0.25, 0.125 + 2.0 ** -6
    code, good = _rule(x, step, bound)
    assert code.tolist() == [1, 2, 4, 0, 9, -3, 12, 16] and good.tolist() == [True] * 3 + [False] + [True] * 4
    by_hand = {(1,): [2, 2, 4, 7, 18, 23, 30, 8], (1, 3): [2, 2, 4, 9, 16, 27, 38, 9]}
    for lags, z in by_hand.items():
        c, o = _counts(x, lags, step, bound)
        assert o == 1 and c[0].tolist() == np.bincount(z, minlength=256).tolist(), lags
        assert all(c[j, 0] == 8 and c[j].sum() == 8 for j in range(1, k)), lags
    B = _Blocks(k, [(x, lags, a, step, bound) for lags, a in zip(by_hand, (1, 0))])
    got = _run(shafa, B, [8, 11])
    assert got[GUARD + 2] == 2 and got[GUARD + 30] == 1 and got[GUARD + k * 256 + 9] == 2 and got[GUARD + 256] == 8
    assert B.found() == [1, 1]


# ---------------------------------------------------------------- 2. the kernel: one launch over all the shapes
def _sweep(shafa, k):
    T, R = shafa.PLANES_TILE, shafa.PLANES_HIST_RUN
    counts = (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3, R * T - 1, R * T + 1)
    rows = [(1,), (3,), (1, 3), (2, 3, 5), (1, 16, T), (1, 1 << 40)]       # the last: a lag past every capacity
    steps = [2.0 ** -10, _exact(1e-3, k), _exact(0.37, k), 3.0, _exact(1e-7, k)]
    out = []
    for b, (s, n) in enumerate((s, n) for s in rows for n in counts):
        step = steps[b % len(steps)]
        out.append((_values(n, k, step, T, 10 * k + b), s, (0, 1, 3)[b % 3], step, _exact(step * (0.5 + 2.0 ** -6), k)))
    return out


@pytest.mark.parametrize("k", (4, 8))
def test_one_launch_against_the_model_and_the_split_entry(shafa, k):
    blocks = _sweep(shafa, k)
    B = _Blocks(k, blocks)
    # every planted kind is in the set, with both outcomes where it has two
    allx = np.concatenate(B.x)
    allg = np.concatenate([_rule(x, s, e)[1] for x, s, e in zip(B.x, B.step, B.bound)])
    assert (np.isnan(allx) & ~allg).any() and (np.isinf(allx) & ~allg).any() and (np.signbit(allx) & (allx == 0) & allg).any()
    assert ((allx != 0) & (np.abs(allx) < float(np.finfo(FLOAT[k]).tiny)) & allg).any()
    assert sum(B.found()) > 100 and {(o % 64) // k for o in B.off} == {0, 1, 3}
    got = _run(shafa, B, [n + 5 for n in B.n], split=True)
    sums = got[GUARD:-GUARD].reshape(B.nb, k, 256).sum(2)
    assert (sums == np.array(B.n, np.uint64)[:, None]).all()               # every plane's counts sum to n


# ---------------------------------------------------------------- 3. block borders inside a workgroup's run
@pytest.mark.parametrize("k", (4, 8))
def test_block_borders_inside_a_run(shafa, k):
    """sixty-four blocks of 100 .. 3000 elements, a tile each and so eight to a run, alternately all NaN and clean: a count
    flushed to the wrong block, or a counter not cleared at a border, shows in the neighbour"""
    rng = np.random.default_rng(900 + k)
    ns = rng.integers(100, 3001, 64).tolist()
    ns[0], ns[1], ns[-1] = 100, 3000, 3000
    step, bound = 0.5, _exact(0.26, k)
    rows = [(1,), (1, 7), (3,), (2, 3, 50)]

    def clean(n):
        return (np.arange(n) * 0.5 + 3 * np.sin(np.arange(n) / 5)).astype(FLOAT[k])

    # both ways round, so that every block is once behind a block of outliers and once in front of one
    for first in (0, 1):
        B = _Blocks(k, [(np.full(n, np.nan, FLOAT[k]) if b % 2 == first else clean(n), rows[b % 4], (0, 1, 3)[b % 3], step, bound)
                        for b, n in enumerate(ns)])
        assert B.found() == [n if b % 2 == first else 0 for b, n in enumerate(ns)]
        got = _run(shafa, B, ns)
        assert (got[GUARD:-GUARD].reshape(64, k, 256).sum(2) == np.array(ns, np.uint64)[:, None]).all()


@pytest.mark.parametrize("k", (4, 8))
def test_every_lane_counts(shafa, k):
    """all-NaN blocks of 2 T + 3 and R T + 1 elements: every lane of every unit counts, the last unit a partial one; the planes
    are all zeros"""
    T, R = shafa.PLANES_TILE, shafa.PLANES_HIST_RUN
    ns = [2 * T + 3, R * T + 1]
    B = _Blocks(k, [(np.full(n, np.nan, FLOAT[k]), s, a, 0.25, 0.125) for n, s, a in zip(ns, [(1, 64), (1,)], (3, 0))])
    assert B.found() == ns
    got = _run(shafa, B, [n + 5 for n in ns], split=True)
    assert got[GUARD] == ns[0] and got[GUARD + k * 256] == ns[1]


# ---------------------------------------------------------------- 4. the drivers' shape: blocks on ONE region
@pytest.mark.parametrize("k", (4, 8))
def test_eight_blocks_on_one_region(shafa, k):
    """four rows of lags x two steps, all eight blocks the same 3 T + 21 elements"""
    T = shafa.PLANES_TILE
    n = 3 * T + 21
    x = _values(n, k, 2.0 ** -10, T, 33)
    rows = [(1,), (64,), (1, 64), (1, 64, 4096)]
    first = (x, rows[0], 3, 2.0 ** -10, _exact(2.0 ** -10 * 0.51, k))
    blocks = [first] + [(0, s, 3, step, _exact(step * 0.51, k)) for step in (2.0 ** -10, _exact(0.013, k)) for s in rows][1:]
    B = _Blocks(k, blocks)
    assert len(set(B.off)) == 1 and B.found()[0] > 0
    _run(shafa, B, [n] * 8)


@pytest.mark.parametrize("k", (4, 8))
def test_nine_blocks_one_past_its_capacity(shafa, k):
    """two empty blocks, one past its capacity (OUTSIDE_MODULE, its counts and its outliers 0), six of mixed sizes and rows"""
    T = shafa.PLANES_TILE
    ns = [17, 0, T + 1, 15, 3 * T + 5, 4100, 0, 1024, 2 * T]
    lags = [(1, 3), (1,), (1, 256), (1, 1 << 40), (1, 5, 300), (2,), (7, 8, 9), (64,), (3, 257, 8000)]
    step = _exact(1e-3, k)
    B = _Blocks(k, [(_values(n, k, step, T, 50 + b), s, (0, 1, 3)[b % 3], step, _exact(step * 0.51, k))
                    for b, (n, s) in enumerate(zip(ns, lags))])
    bad = 4
    assert B.found()[bad] > 0
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    _run(shafa, B, cap)
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    B.zero(bad)
    _run(shafa, B, cap, dn, [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)])


# ---------------------------------------------------------------- 5. behind a busy stream
def test_four_launches_behind_a_busy_stream_one_finish(shafa):
    """floats and doubles, two launches each on one batch behind a large torch kernel, the sizes from a kernel on the stream too,
    nothing synchronised in between"""
    torch = _torch()
    dev = _dev()
    T = shafa.PLANES_TILE
    Bs = []
    for k, n, rows in ((4, (1 << 18) + 3, [(1, 64, 4096), (1,)]), (8, (1 << 17) + 1, [(3, 4097), (1, 64)])):
        step = _exact(1e-3, k)
        for s in rows:
            Bs.append(_Blocks(k, [(_values(n, k, step, T, 77), s, 3, step, _exact(step * 0.51, k)),
                                  (_values(1000, k, step, T, 78), (1, 3), 1, step, _exact(step * 0.51, k))]))
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_el = [_to(B.el) for B in Bs]
        bufs = [(_guarded(2 * B.k * 256), _guarded(2)) for B in Bs]
        half = torch.tensor([[[n // 2, n - n // 2] for n in B.n] for B in Bs], dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(st):
            busy = torch.empty(1 << 26, dtype=torch.float32, device=dev)
            busy.normal_()                                                 # 256 MiB written
            d_n = half.sum(dim=2)                                          # the sizes exist only behind it
            for i, B in enumerate(Bs):
                bt.hist_planes_grid_quant_dev(st, B.k, B.lags, B.step, B.bound, d_el[i], B.off, B.n, d_n[i], bufs[i][0][1], bufs[i][1][1])
            assert bt.finish(st, 2) == (0, [0, 0])
        for B, ((whole_f, _), (whole_o, _)) in zip(Bs, bufs):
            _check(B, whole_f, whole_o)
            assert B.found()[0] > 8
    finally:
        bt.close()


# ---------------------------------------------------------------- 6. the drivers
@functools.lru_cache(maxsize=None)
def _fields(k):
    """DESIGN 7.28's field as floats with the three NaNs of tests/test_gpu_fields.py planted, [32, 64, 64]"""
    return planted(k).reshape(32, 64, 64)


CANDS = [(1,), (64,), (4096,), (1, 64), (1, 4096), (64, 4096), (1, 64, 4096)]


@pytest.mark.parametrize("k", (4, 8))
def test_field_histograms_equals_the_entry_and_numpy(shafa, k):
    torch = _torch()
    a = _fields(k)[:6]
    t = torch.from_numpy(a).to(_dev())
    sets = [(64,), (1, 64), (1,), (1, 64), (5, 64, 4096)]
    errs = [1e-1, 1e-2, 1e-2, 1e-3, 1e-1]                                  # the same lags twice, with different bounds
    freq, outl = shafa.field_histograms(t, errs, sets)
    assert freq.dtype == outl.dtype == torch.int64 and tuple(freq.shape) == (5, k, 256) and tuple(outl.shape) == (5,)
    assert freq.device == outl.device == t.device
    x = a.reshape(-1)
    want = [field_model(shafa, shafa.fields, x, e, c) for e, c in zip(errs, sets)]
    assert freq.cpu().numpy().astype(np.uint64).tobytes() == np.stack([w[0] for w in want]).tobytes()
    assert outl.tolist() == [w[1] for w in want] and min(outl.tolist()) >= 1            # the NaN at 0
    assert not torch.equal(freq[1], freq[3])
    one, one_o = shafa.field_histograms(t, 1e-2, [(1, 64)])
    assert torch.equal(one[0], freq[1]) and one_o.tolist() == [want[1][1]]
    params = [shafa.fields._params("test", e, k) for e in errs]
    st = _stream()
    bt = shafa.Batch(5, 1 << 20)
    try:
        _, d_freq = _guarded(5 * k * 256)
        _, d_outl_n = _guarded(5)
        bt.hist_planes_grid_quant_dev(st, k, sets, [p[0] for p in params], [p[1] for p in params], t, [0] * 5, [t.numel()] * 5,
                                      _sizes([t.numel()] * 5), d_freq, d_outl_n)
        assert bt.finish(st, 5) == (0, [0] * 5)
        assert torch.equal(d_freq.view(5, k, 256), freq) and torch.equal(d_outl_n, outl)
    finally:
        bt.close()
    f0, o0 = shafa.field_histograms(t, 1e-2, [])
    assert tuple(f0.shape) == (0, k, 256) and tuple(o0.shape) == (0,)
    f0, o0 = shafa.field_histograms(t[:0], [1e-2, 1.0], [(1,), (1, 2)])
    assert tuple(f0.shape) == (2, k, 256) and int(f0.abs().sum()) == 0 and o0.tolist() == [0, 0]


def test_field_sizes_and_choose_field_lags_equal_the_model(shafa):
    """integer for integer on float32 and float64 in one call, with an empty and a 0-dimensional tensor among them"""
    torch = _torch()
    F = shafa.fields
    dev = _dev()
    a4, a8 = _fields(4)[:8], _fields(8)[:5]
    ts = [torch.from_numpy(a4).to(dev), torch.empty((0, 4), dtype=torch.float32, device=dev), torch.from_numpy(a8).to(dev),
          torch.tensor(2.5, dtype=torch.float64, device=dev)]
    errs = [1e-2, 1.0, 1e-4, 0.5]
    got = shafa.field_sizes(ts, errs)
    want = [field_model_sizes(shafa, F, a4.reshape(-1), 1e-2, CANDS), [((), 0, 0)], field_model_sizes(shafa, F, a8.reshape(-1), 1e-4, CANDS),
            [((), 0, 0)]]
    assert got == want
    assert all(len(e) == 3 and e[2] >= 1 for e in got[0] + got[2])         # the planted NaNs are counted
    assert shafa.choose_field_lags(ts, errs) == [w[0][0] for w in want]
    # one bound for all; explicit candidates, one list for all and one per tensor; explicit axes
    both = [ts[0], ts[2]]
    x = [a4.reshape(-1), a8.reshape(-1)]
    assert shafa.field_sizes(both, 1e-1) == [field_model_sizes(shafa, F, v, 1e-1, CANDS) for v in x]
    cands = [(2, 3), (64,), (1, 1 << 40)]
    assert shafa.field_sizes(both, 1e-2, candidates=cands) == [field_model_sizes(shafa, F, v, 1e-2, cands) for v in x]
    per = [[(1, 64, 4096)], [(7,), (1, 300), (300,)]]
    assert shafa.field_sizes(both, [1e-1, 1e-3], candidates=per) == [field_model_sizes(shafa, F, v, e, c)
                                                                     for v, e, c in zip(x, (1e-1, 1e-3), per)]
    assert shafa.field_sizes(ts[0], 1e-2, axes=(0, 2)) == [field_model_sizes(shafa, F, x[0], 1e-2, [(1,), (4096,), (1, 4096)])]
    assert shafa.field_sizes([ts[1], ts[3]], 1e-3) == [[((), 0, 0)]] * 2 and shafa.choose_field_lags([ts[3]], 1e-3) == [()]


@pytest.mark.parametrize("k", (4, 8))
def test_field_rates_and_fit_abs_error(shafa, k):
    torch = _torch()
    F = shafa.fields
    a = _fields(k)[:8]
    t = torch.from_numpy(a).to(_dev())
    n = t.numel()
    bounds = [1.0, 1e-1, 3e-2, 1e-2, 1e-3, 1e-30]                          # the last: every element an outlier
    for lags in (None, (1, 64)):
        g = lags or (1, 64, 4096)
        rates = shafa.field_rates(t, bounds, lags=lags)
        assert [r[0] for r in rates] == bounds
        assert rates == [(e,) + shafa.field_sizes(t, e, candidates=[g])[0][0][1:] for e in bounds]  # six field_sizes calls
        assert rates == [(e,) + field_model(shafa, F, a.reshape(-1), e, g)[:0:-1] for e in bounds]  # and numpy
        assert rates[-1][2] > F.outlier_capacity(n)
        ok = [r for r in rates if r[2] <= F.outlier_capacity(n)]
        assert len(ok) >= 3 and ok[0][1] < ok[-1][1]                                                # a smaller bound costs bytes
        for budget in [r[1] for r in ok] + [ok[1][1] - 1, 10 ** 9]:
            fits = [r[0] for r in ok if r[1] <= budget]
            assert shafa.fit_abs_error(t, budget, bounds, lags=lags) == (min(fits) if fits else None), budget
        assert shafa.fit_abs_error(t, 0, bounds, lags=lags) is None
        assert shafa.fit_abs_error(t, 10 ** 9, bounds[::-1], lags=lags) == min(r[0] for r in ok)    # never a bound past the capacity
    assert shafa.field_rates(t, [1e-2], axes=(2,)) == [(1e-2,) + field_model(shafa, F, a.reshape(-1), 1e-2, (1,))[:0:-1]]
    assert shafa.field_rates(t[:0], [1e-2, 1.0]) == [(1e-2, 0, 0), (1.0, 0, 0)] and shafa.fit_abs_error(t[:0], 0, [1e-2, 1.0]) == 1e-2


def test_noise_sorts_every_candidate_last(shafa):
    """a noise tensor at 10^-30: every element of every candidate is an outlier, compress_fields keeps it lossless, and the list
    is the model's, all of it behind the capacity"""
    torch = _torch()
    F = shafa.fields
    a = np.random.default_rng(5).standard_normal((64, 300)).astype(np.float32)
    t = torch.from_numpy(a).to(_dev())
    got = shafa.field_sizes(t, 1e-30)[0]
    assert [e[0] for e in got] == [(1,), (300,), (1, 300)] and all(e[2] == a.size > F.outlier_capacity(a.size) for e in got)
    assert got == field_model_sizes(shafa, F, a.reshape(-1), 1e-30, [(1,), (300,), (1, 300)])
    assert all(e[1] >= (8 + 4) * a.size for e in got)
    assert shafa.compress_fields(t, 1e-30, lags=[got[0][0]])[0].step == 0.0
    # the same where the planes would be small: every other row NaN is past the capacity too, whatever the bytes
    clean = (np.arange(64 * 300) * 1e-3).astype(np.float32).reshape(64, 300)
    mixed = np.where(np.arange(64)[:, None] % 2 == 0, clean, np.float32(np.nan))
    got = shafa.field_sizes(torch.from_numpy(mixed).to(_dev()), 1e-3)[0]
    assert all(e[2] >= 32 * 300 > F.outlier_capacity(a.size) for e in got)
    assert got == field_model_sizes(shafa, F, mixed.reshape(-1), 1e-3, [(1,), (300,), (1, 300)])


@pytest.mark.parametrize("k", (4, 8))
def test_the_model_beside_the_files(shafa, k, capsys):
    """DESIGN 7.28's field at 10^-1 and 10^-2: the model's nbytes and compress_fields' per candidate, printed for DESIGN 7.31.
    Only that the pick is the model's minimum is asserted: the model is of order 0 and knows no RLE, blocks or headers."""
    torch = _torch()
    a = _fields(k)
    t = torch.from_numpy(a).to(_dev())
    for err in (1e-1, 1e-2):
        sizes = shafa.field_sizes(t, err)[0]
        pick = shafa.choose_field_lags(t, err)[0]
        items = shafa.compress_fields([t] * len(sizes), err, lags=[c for c, _, _ in sizes])
        real = {it.lags: it.nbytes for it in items}
        with capsys.disabled():
            print(f"\n[field_sizes] float{8 * k} [32, 64, 64] abs_error {err}: pick {pick}, measured best "
                  f"{min(real, key=lambda c: (real[c], len(c), c))}")
            for c, nb, no in sizes:
                print(f"[field_sizes]   {str(c):16} model {nb:7d} B  compress_fields {real[c]:7d} B  outliers {no}")
        assert sorted(c for c, _, _ in sizes) == sorted(CANDS) and all(no == 3 for _, _, no in sizes)
        assert pick == sizes[0][0] and sizes[0][1] == min(nb for _, nb, _ in sizes)
        assert all(int(it.outlier_pos.numel()) == 3 for it in items)

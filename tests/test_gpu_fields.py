"""shafa_hipd_split_planes_grid_quant_dev / shafa_hipd_merge_planes_grid_quant_dev (csrc/planes_lag.hip) and the field drivers on top
(shafa-cd_amd/fields.py) against numpy on the host.  The rule (include/shafa_hip.h: "Error-bounded fields") is restated here in
numpy, one numpy operation in T per IEEE operation: codes, restored values and which elements are good are compared integer for
integer and bit for bit; the planes are numpy's grid differences of the codes (test_gpu_planes_grid._z_planes) and, on the device,
split_planes_grid_dev's over the model's codes.

The shapes are the grid tests': a lane has 16 elements, a tile T = PLANES_TILE.  Every buffer holds 0xA5 where no data lies, and
every comparison is of whole images."""
import numpy as np
import pytest

from test_gpu_planes_grid import _z_planes
from test_gpu_planes_lag import FILL, UINT, _al16, _fill, _img, _sizes, _to
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

FLOAT = {4: np.float32, 8: np.float64}
INT = {4: np.int32, 8: np.int64}
TORCH = {4: "float32", 8: "float64"}


def _model(x, step, bound):
    """the rule: x a float32 or float64 array, step and bound Python floats exactly representable in its type -> (codes as signed
    integers, x' = T(code) * step, good)"""
    k = x.dtype.itemsize
    T = x.dtype.type
    inv = T(1.0 / step)                                                    # the double division, rounded to T once
    with np.errstate(all="ignore"):
        t = x * inv
        inside = np.abs(t) < T(2.0 ** (8 * k - 2))                         # false for a NaN
        code = np.where(inside, np.rint(t), T(0)).astype(INT[k])
        xr = code.astype(T) * T(step)
        if k == 4:
            good = inside & (np.abs(x.astype(np.float64) - xr.astype(np.float64)) <= np.float64(bound))
        else:
            good = inside & (np.abs(x - xr) <= T(bound))
    return code, xr, good


def _restored(x, xr, good):
    """what the merge leaves: x' for a good element, the element's own bits for an outlier"""
    U = UINT[x.dtype.itemsize]
    return np.where(good, xr.view(U), x.view(U))


def _records(x, good):
    """the model's records, sorted: [count, 2] of {position, bits}"""
    pos = np.flatnonzero(~good)
    return np.stack([pos.astype(np.uint64), x.view(UINT[x.dtype.itemsize])[pos].astype(np.uint64)], 1).reshape(-1, 2)


def _values(n, k, step, T_tile, seed):
    """n elements: a smooth ramp with a sine on it in units of the step, and planted in it exact ties (j + 1/2) step, denormals,
    -0.0, t just below and at 2^(8 k - 2), and NaN, +-Inf and 10^38 at the first and the last element, at 15 / 16 / 17 and across
    the tile border"""
    T = FLOAT[k]
    i = np.arange(n, dtype=np.float64)
    x = ((0.37 * i + 40 * np.sin(i / 11) + seed) * step).astype(T)
    edge = float(np.nextafter(T(2.0 ** (8 * k - 2)), T(0)))
    with np.errstate(all="ignore"):
        for at, v in ((5, None), (7, 1e-41 if k == 4 else 1e-310), (9, -0.0), (11, edge * step), (12, 2.0 ** (8 * k - 2) * step),
                      (13, -edge * step)):
            idx = np.arange(at, n, 97)
            x[idx] = ((idx + 0.5) * step).astype(T) if v is None else T(v)
        special = [np.nan, np.inf, -np.inf, 1e38]
        for j, at in enumerate(sorted({0, n - 1, 15, 16, 17, T_tile - 1, T_tile, T_tile + 1})):
            if 0 <= at < n:
                x[at] = T(special[j % 4])
    return x


class _Layout:
    """blocks (n elements, tuple of lags, element side `a` ELEMENTS behind a multiple of 64 bytes, step, bound) of floats of k
    bytes in host images: `el` the element side, `codes` the model's codes in its place, `pl` numpy's planes of the codes' folded
    differences, `out` what the merge leaves, `rec` each block's sorted records.  All FILL where no data lies."""

    def __init__(self, shafa, k, blocks, seed=0):
        self.k, self.n, self.lags = k, [b[0] for b in blocks], [tuple(b[1]) for b in blocks]
        self.step, self.bound = [b[3] for b in blocks], [b[4] for b in blocks]
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
        for b, (n, lags, _, step, bound) in enumerate(blocks):
            x = _values(n, k, step, shafa.PLANES_TILE, seed + b)
            code, xr, good = _model(x, step, bound)
            sl = slice(self.off[b], self.off[b] + n * k)
            self.el[sl] = x.view(np.uint8)
            self.codes[sl] = code.view(np.uint8)
            self.out[sl] = _restored(x, xr, good).view(np.uint8)
            planes = _z_planes(code.tobytes(), k, lags)
            for j in range(k):
                self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = planes[j]
            self.x.append(x)
            self.rec.append(_records(x, good))
            self.good.append(good)

    def within_bound(self, got_el):
        """every finite good element of the image got_el is within its block's bound: in float64 for float32, in longdouble for
        float64"""
        W = np.float64 if self.k == 4 else np.longdouble
        for b, x in enumerate(self.x):
            y = got_el[self.off[b]:self.off[b] + x.size * self.k].view(x.dtype)
            g = self.good[b] & np.isfinite(x)
            assert np.all(np.abs(x[g].astype(W) - y[g].astype(W)) <= W(self.bound[b])), b


def _stream():
    import torch
    return torch.cuda.Stream(device=_dev())


def _exact(v, k):
    return float(FLOAT[k](v))


def _fill64(n):
    """n int64 of FILL bytes"""
    import torch
    return torch.full((n * 8,), FILL, dtype=torch.uint8, device=_dev()).view(torch.int64)


def _rec_img(d_outl):
    return d_outl.cpu().numpy().view(np.uint64).reshape(-1, 2)


def _sorted(rec):
    return rec[np.argsort(rec[:, 0], kind="stable")]


FILL64 = int.from_bytes(bytes([FILL] * 8), "little")


# ---------------------------------------------------------------- 1. by hand
@pytest.mark.parametrize("k", (4, 8))
def test_eight_elements_worked_out_by_hand(shafa, k):
    """step 1/4, bound 1/8 + 1/64: x = 0.25 0.5 1.0 NaN 2.3 -0.75 3.1 4.0.  t = 1 2 4 NaN 9.2 -3 12.4 16, codes 1 2 4 0 9 -3 12 16;
    x' = .25 .5 1 0 2.25 -.75 3 4; |x - x'| = 0 0 0 - .05 0 .1 0: all good but the NaN, which has no code.
    Lags (1,): d = 1 1 2 -4 9 -12 15 4, z = 2 2 4 7 18 23 30 8.  Lags (1, 3): (1 - S^3) of that: d = 1 1 2 -5 8 -14 19 -5,
    z = 2 2 4 9 16 27 38 9.  The merge leaves x' and, at 3, the NaN's own bits."""
    T, U = FLOAT[k], UINT[k]
    x = np.array([0.25, 0.5, 1.0, np.nan, 2.3, -0.75, 3.1, 4.0], T)
    x.view(U)[3] |= U(0x1234)                                              # a payload, to come back bit for bit
    step, bound = 0.25, 0.125 + 2.0 ** -6
    code, xr, good = _model(x, step, bound)
    assert code.tolist() == [1, 2, 4, 0, 9, -3, 12, 16] and good.tolist() == [True] * 3 + [False] + [True] * 4
    assert xr.tolist() == [0.25, 0.5, 1.0, 0.0, 2.25, -0.75, 3.0, 4.0]
    by_hand = {(1,): [2, 2, 4, 7, 18, 23, 30, 8], (1, 3): [2, 2, 4, 9, 16, 27, 38, 9]}
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes([8])
        for lags, z in by_hand.items():
            assert _z_planes(code.tobytes(), k, lags)[0].tolist() == z and not _z_planes(code.tobytes(), k, lags)[1:].any(), lags
            el = np.full(64 + 8 * k, FILL, np.uint8)
            el[16:16 + 8 * k] = x.view(np.uint8)
            d_el, d_pl, d_out = _to(el), _fill(16 * k + 64), _fill(64 + 16 * k)
            d_outl, d_cnt = _fill64(2 * 4), _fill64(1)
            poff = [32 + 16 * j for j in range(k)]
            bt.split_planes_grid_quant_dev(st, k, [lags], [step], [bound], d_el, [16], [8], d_n, d_pl, poff, d_outl, [1], [2], d_cnt)
            assert bt.finish(st, 1) == (0, [0])
            want = bytes([FILL] * 32) + b"".join(bytes(z if j == 0 else [0] * 8) + bytes([FILL] * 8) for j in range(k)) + bytes([FILL] * 32)
            assert _img(d_pl) == want, lags
            assert d_cnt.tolist() == [1]
            assert _rec_img(d_outl).tolist() == [[FILL64] * 2, [3, int(x.view(U)[3])], [FILL64] * 2, [FILL64] * 2]
            bt.merge_planes_grid_quant_dev(st, k, [lags], [step], d_pl, poff, [8], d_n, d_outl, [1], [1], d_out, [8 * k])
            assert bt.finish(st, 1) == (0, [0])
            assert _img(d_out) == bytes([FILL] * 8 * k) + _restored(x, xr, good).tobytes() + bytes([FILL] * 64), lags
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. the kernels: one launch each way over all the shapes
def _blocks(shafa, k):
    T = shafa.PLANES_TILE
    counts = (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3)
    rows = [(1,), (3,), (1, 3), (2, 3, 5), (1, 16, T), (1, 1 << 40)]
    steps = [2.0 ** -10, _exact(1e-3, k), _exact(0.37, k), 3.0, _exact(1e-7, k)]
    out = []
    for b, (s, n) in enumerate((s, n) for s in rows for n in counts):
        step = steps[b % len(steps)]
        out.append((n, s, (0, 1, 3)[b % 3], step, _exact(step * (0.5 + 2.0 ** -6), k)))
    return out


@pytest.mark.parametrize("k", (4, 8))
def test_one_launch_each_way_against_the_model(shafa, k):
    import torch
    blocks = _blocks(shafa, k)
    L = _Layout(shafa, k, blocks, 10 * k)
    nb = len(blocks)
    cap = [n + 5 for n in L.n]
    found = [len(r) for r in L.rec]
    assert sum(found) > 100
    # every planted kind is in the set with both outcomes where it has two
    allx, allg = np.concatenate(L.x), np.concatenate(L.good)
    assert (np.isnan(allx) & ~allg).any() and (np.isinf(allx) & ~allg).any() and (np.signbit(allx) & (allx == 0) & allg).any()
    tiny = float(np.finfo(FLOAT[k]).tiny)
    assert ((allx != 0) & (np.abs(allx) < tiny) & allg).any()
    ooff, pos = [], 2                                                      # two guard records in front
    for n in L.n:
        ooff.append(pos)
        pos += n + 1                                                       # room for every element, one guard record behind
    st = _stream()
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_n = _sizes(L.n)
        d_el, d_pl, d_outl, d_cnt = _to(L.el), _fill(L.pl.size), _fill64(2 * pos), _fill64(nb + 2)
        bt.split_planes_grid_quant_dev(st, k, L.lags, L.step, L.bound, d_el, L.off, cap, d_n, d_pl, L.poff, d_outl, ooff, L.n,
                                       d_cnt[1:nb + 1])
        # the form it replaces: the model's codes through the exact integer split
        d_codes, d_pl2 = _to(L.codes), _fill(L.pl.size)
        bt.split_planes_grid_dev(st, k, L.lags, d_codes, L.off, cap, d_n, d_pl2, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb)
        got = d_pl.cpu().numpy()
        bad = [(L.n[b], L.lags[b]) for b in range(nb)
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
        # merge: numpy's planes and the model's records
        d_pl, d_out = _to(L.pl), _fill(L.el.size)
        d_rec = _to(want.view(np.int64).reshape(-1))
        bt.merge_planes_grid_quant_dev(st, k, L.lags, L.step, d_pl, L.poff, cap, d_n, d_rec, ooff, found, d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        got = d_out.cpu().numpy()
        bad = [(L.n[b], L.lags[b]) for b in range(nb)
               if got[L.off[b]:L.off[b] + L.n[b] * k].tobytes() != L.out[L.off[b]:L.off[b] + L.n[b] * k].tobytes()]
        assert not bad, bad[:8]
        assert got.tobytes() == L.out.tobytes()
        assert _img(d_pl) == L.pl.tobytes() and _img(d_rec.view(torch.uint8)) == want.tobytes()
        L.within_bound(got)
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. capacities
@pytest.mark.parametrize("k", (4, 8))
def test_capacities_below_the_outliers(shafa, k):
    """a block with no room and three outliers, one with room for two of its five: the counts are those found, the planes are
    complete, the two records written are two of the model's, nothing lies behind them"""
    T = FLOAT[k]
    step, bound = 0.5, 0.25
    xs = []
    for n, at in ((40, (0, 16, 39)), (50, (3, 15, 17, 31, 49))):
        x = (np.arange(n) * 0.5).astype(T)
        x[list(at)] = np.array([np.nan, np.inf, -np.inf, 1e38, np.nan][:len(at)], T)
        xs.append(x)
    L = _Layout(shafa, k, [(40, (1,), 0, step, bound), (50, (1, 3), 1, step, bound)])
    for b, x in enumerate(xs):                                             # this test's values in the layout's places
        code, xr, good = _model(x, step, bound)
        L.el[L.off[b]:L.off[b] + x.size * k] = x.view(np.uint8)
        planes = _z_planes(code.tobytes(), k, L.lags[b])
        for j in range(k):
            L.pl[L.poff[b * k + j]:L.poff[b * k + j] + x.size] = planes[j]
        L.rec[b] = _records(x, good)
    assert [len(r) for r in L.rec] == [3, 5]
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes(L.n)
        d_el, d_pl, d_outl, d_cnt = _to(L.el), _fill(L.pl.size), _fill64(2 * 6), _fill64(2)
        bt.split_planes_grid_quant_dev(st, k, L.lags, L.step, L.bound, d_el, L.off, L.n, d_n, d_pl, L.poff, d_outl, [1, 2], [0, 2], d_cnt)
        assert bt.finish(st, 2) == (0, [0, 0])
        assert d_cnt.tolist() == [3, 5]
        assert _img(d_pl) == L.pl.tobytes()
        rec = _rec_img(d_outl)
        assert rec[:2].tolist() == [[FILL64] * 2] * 2 and rec[4:].tolist() == [[FILL64] * 2] * 2
        mine = {tuple(r) for r in L.rec[1].tolist()}
        assert tuple(rec[2].tolist()) in mine and tuple(rec[3].tolist()) in mine and rec[2, 0] != rec[3, 0]
        # no record buffer at all where every capacity is 0
        d_pl = _fill(L.pl.size)
        bt.split_planes_grid_quant_dev(st, k, L.lags, L.step, L.bound, d_el, L.off, L.n, d_n, d_pl, L.poff, None, [0, 0], [0, 0], d_cnt)
        assert bt.finish(st, 2) == (0, [0, 0])
        assert d_cnt.tolist() == [3, 5] and _img(d_pl) == L.pl.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. a record past its block
@pytest.mark.parametrize("k", (4, 8))
def test_a_record_at_the_blocks_size_is_refused(shafa, k):
    """three blocks; the middle one has a record at position n (and one inside): its code is OUTSIDE_MODULE, the record is not
    written — the element behind the block stays FILL — and its neighbours are right"""
    n = [33, 20, 17]
    L = _Layout(shafa, k, [(n[0], (1,), 0, 0.5, 0.25), (n[1], (1, 3), 1, 0.25, 0.125), (n[2], (2,), 3, 0.5, 0.25)], 3)
    recs = [L.rec[0], np.array([[7, 0x3F80], [n[1], 0x1111]], np.uint64), L.rec[2]]
    want = L.out.copy()
    x1 = L.x[1]
    code, xr, good = _model(x1, 0.25, 0.125)
    img = xr.view(UINT[k]).copy()                                          # no outlier of its own is patched: only record 7
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
        bt.merge_planes_grid_quant_dev(st, k, L.lags, L.step, d_pl, L.poff, [c + 5 for c in n], d_n, d_rec, ooff,
                                       [len(r) for r in recs], d_out, L.off)
        assert bt.finish(st, 3, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [0, shafa.OUTSIDE_MODULE, 0])
        assert _img(d_out) == want.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. behind a busy stream
def test_behind_a_busy_stream_one_finish(shafa):
    """2^19 + 3 floats at lags (1, 64, 4096) and 2^18 + 1 doubles at (3, 4097), split and merged back behind a large torch kernel
    on the same stream: four launches on one batch, nothing synchronised in between, one finish"""
    import torch
    dev = _dev()
    cases = [(4, (1 << 19) + 3, (1, 64, 4096), 3, _exact(1e-3, 4)), (8, (1 << 18) + 1, (3, 4097), 1, 1e-9)]
    Ls = [_Layout(shafa, k, [(n, g, a, s, _exact(s * 0.51, k))], 77) for k, n, g, a, s in cases]
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
            for i, (k, n, g, a, s) in enumerate(cases):
                bt.split_planes_grid_quant_dev(st, k, [g], Ls[i].step, Ls[i].bound, d_el[i], Ls[i].off, [n], d_n[i:i + 1], d_pl[i],
                                               Ls[i].poff, d_outl[i], [0], [n], d_cnt[i])
            for i, (k, n, g, a, s) in enumerate(cases):                    # the records where the split puts them, all the model's
                bt.merge_planes_grid_quant_dev(st, k, [g], Ls[i].step, d_pl[i], Ls[i].poff, [n], d_n[i:i + 1], d_outl[i], [0],
                                               [found[i]], d_out[i], Ls[i].off)
            assert bt.finish(st, 1) == (0, [0])
        for i, L in enumerate(Ls):
            assert d_cnt[i].tolist() == [found[i]] and found[i] > 8, cases[i]
            assert _sorted(_rec_img(d_outl[i])[:found[i]]).tobytes() == L.rec[0].tobytes(), cases[i]
            assert _img(d_pl[i]) == L.pl.tobytes(), cases[i]
            assert _img(d_out[i]) == L.out.tobytes(), cases[i]
    finally:
        bt.close()


# ---------------------------------------------------------------- 6. the drivers
def _field(k):
    """DESIGN 7.28's [32, 64, 64] field as floats, with three NaNs of distinct payloads planted"""
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.float64)
    f = (1000 * np.sin(x / 9) * np.cos(y / 13) * np.sin(z / 7 + 0.3)).astype(FLOAT[k])
    flat = f.reshape(-1)
    for j, at in enumerate((0, 70000, flat.size - 1)):
        flat[at] = np.nan
        flat.view(UINT[k])[at] |= UINT[k](0x100 + j)
    return f


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.mark.parametrize("k", (4, 8))
def test_quantize_and_restore_against_the_entries(shafa, k):
    import torch
    f = _field(k)[:5]
    t = torch.from_numpy(f).to(_dev())
    lags = (1, 64, 4096)
    planes, pos, bits = shafa.quantize_field(t, 0.01, lags)
    step, bound = shafa.fields._params("test", 0.01, k)
    code, xr, good = _model(f.reshape(-1), step, bound)
    assert planes.cpu().numpy().tobytes() == _z_planes(code.tobytes(), k, lags).tobytes()
    want = _records(f.reshape(-1), good)
    assert pos.dtype == bits.dtype == torch.int64 and len(want) >= 1
    assert pos.cpu().numpy().astype(np.uint64).tolist() == want[:, 0].tolist()
    assert bits.cpu().numpy().view(np.uint64).tolist() == want[:, 1].tolist()
    back = shafa.restore_field(planes, t.dtype, t.shape, lags, step, pos, bits)
    assert back.dtype == t.dtype and back.shape == t.shape
    assert back.cpu().numpy().reshape(-1).view(UINT[k]).tobytes() == _restored(f.reshape(-1), xr, good).tobytes()
    # more outliers than the first launch has room for: every one of them is found by the second
    noise = torch.from_numpy(np.random.default_rng(k).standard_normal(5000).astype(FLOAT[k])).to(_dev())
    planes, pos, bits = shafa.quantize_field(noise, 1e-30, (1,))
    assert int(pos.numel()) > shafa.fields.outlier_capacity(5000)
    back = shafa.restore_field(planes, noise.dtype, noise.shape, (1,), shafa.fields._params("test", 1e-30, k)[0], pos, bits)
    nz = noise != 0
    assert torch.equal(_bits(back)[nz], _bits(noise)[nz])


@pytest.mark.parametrize("k", (4, 8))
def test_compress_fields_round_trip_and_it_pays(shafa, k, capsys):
    import torch
    f = _field(k)
    t = torch.from_numpy(f).to(_dev())
    keep = t.clone()
    nan = torch.isnan(keep)
    assert int(nan.sum()) == 3
    lossless = shafa.compress_grids(t)[0].nbytes
    for err in (1e-1, 1e-2):
        items = shafa.compress_fields(t, err)
        again = shafa.compress_fields(t, err)
        it = items[0]
        assert type(it) is shafa.CompressedField and it.dtype == t.dtype and it.shape == tuple(t.shape) and it.lags == (1, 64, 4096)
        assert it.abs_error == err and (it.step, it.bound) == shafa.fields._params("test", err, k) and it.bound <= err
        pos = it.outlier_pos.cpu().tolist()
        assert pos == sorted(pos) and set(torch.nonzero(nan.reshape(-1)).reshape(-1).tolist()) <= set(pos)
        planes_bytes = sum(sum(int(x.numel()) for x in p.values()) if isinstance(p, dict) else int(p.numel()) for p in it.planes)
        assert it.nbytes == planes_bytes + (8 + k) * len(pos)
        # the items are equal on a second run
        other = again[0]
        assert other.nbytes == it.nbytes and torch.equal(other.outlier_pos, it.outlier_pos) and torch.equal(other.outlier_bits, it.outlier_bits)
        for p, q in zip(it.planes, other.planes):
            assert type(p) is type(q)
            if isinstance(p, dict):
                assert sorted(p) == sorted(q) and all(torch.equal(p[key], q[key]) for key in p)
            else:
                assert torch.equal(p, q)
        back = shafa.decompress_fields(items)[0]
        assert back.dtype == t.dtype and back.shape == t.shape and torch.equal(_bits(t), _bits(keep))
        assert torch.equal(_bits(back)[nan], _bits(keep)[nan])            # the NaNs bit for bit
        W = torch.float64
        diff = (back[~nan].to(W) - keep[~nan].to(W)).abs()
        assert float(diff.max()) <= it.bound <= err, (k, err, float(diff.max()))
        with capsys.disabled():
            print(f"\n[fields] float{8 * k} [32, 64, 64] abs_error {err}: compress_fields {it.nbytes} B, compress_grids {lossless} B, "
                  f"raw {t.numel() * k} B, outliers {len(pos)}")
        assert it.nbytes < lossless


def test_noise_falls_back_and_mixed_lists(shafa):
    import torch
    dev = _dev()
    rng = np.random.default_rng(5)
    noise = torch.from_numpy(rng.standard_normal((64, 300)).astype(np.float32)).to(dev)
    it = shafa.compress_fields(noise, 1e-30)[0]
    assert it.step == 0.0 and it.outlier_pos.numel() == 0 and it.lags == (1, 300)
    ref = shafa.compress_grids(noise)[0]
    assert it.nbytes == ref.nbytes
    for p, q in zip(it.planes, ref.planes):
        assert type(p) is type(q) and (isinstance(p, dict) or torch.equal(p, q))
    assert torch.equal(_bits(shafa.decompress_fields(it)[0]), _bits(noise))
    # a mixed list with one abs_error each: a lossless one among quantised ones, an empty and a 0-dimensional tensor
    f4, f8 = torch.from_numpy(_field(4)[:3]).to(dev), torch.from_numpy(_field(8)[:2]).to(dev)
    ts = [f4, noise, f8, torch.empty((0, 4), dtype=torch.float32, device=dev), torch.tensor(2.5, dtype=torch.float64, device=dev),
          f4.reshape(-1)[1:4001]]
    errs = [1e-2, 1e-30, 1e-5, 1.0, 0.5, 1e-1]
    items = shafa.compress_fields(ts, errs)
    assert [it.step == 0.0 for it in items] == [False, True, False, False, False, False]
    assert [it.lags for it in items] == [(1, 64, 4096), (1, 300), (1, 64, 4096), (1,), (1,), (1,)]
    backs = shafa.decompress_fields(items)
    for t, it, e, b in zip(ts, items, errs, backs):
        assert b.dtype == t.dtype and b.shape == t.shape
        if it.step == 0.0:
            assert torch.equal(_bits(b), _bits(t))
            continue
        nan = torch.isnan(t)
        assert torch.equal(_bits(b)[nan], _bits(t)[nan])
        if t.numel():
            assert float((b[~nan].double() - t[~nan].double()).abs().max()) <= it.bound <= e
    assert abs(float(backs[4]) - 2.5) <= 0.5 and backs[3].numel() == 0
    # an item alone, explicit lags
    it = shafa.compress_fields(f4, 1e-2, lags=(1, 64))[0]
    assert it.lags == (1, 64)
    b = shafa.decompress_fields(it)[0]
    nan = torch.isnan(f4)
    assert float((b[~nan].double() - f4[~nan].double()).abs().max()) <= it.bound

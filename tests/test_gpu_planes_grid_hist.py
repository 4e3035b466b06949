"""shafa_hipd_hist_planes_grid_dev (csrc/planes_lag.hip) and grid_histograms / grid_sizes / choose_lags on top against numpy on the
host: the counts are np.bincount over the planes that tests/test_gpu_planes_grid.py's numpy expectation (_z_planes) gives for the
block's raw bytes and row of lags — for the row of zeros, over the bytes as they lie —, the sizes are those of
tests/test_planes_grid_hist_cpu.py's model with the host's Module T.  Device code is compared with device code in one test only,
whose other side is hist256 over the split entries' planes.

The shapes are the borders of the kernel: a lane has 16 elements, a tile T = PLANES_TILE, a workgroup a run of PLANES_HIST_RUN
tiles of the capacities.  d_freq arrives filled with 0xA5 between guard words that must survive, and every comparison is of the
whole buffer."""
import functools

import numpy as np
import pytest

from test_gpu_planes_grid import _stream, _z_planes
from test_gpu_planes_lag import ELEMS, FILL, UINT, _fill, _img, _random, _same, _sizes, _to
from test_gpu_unpack import _dev
from test_planes_grid_hist_cpu import model_sizes, plane_histograms, three_tensors

pytestmark = pytest.mark.gpu

GUARD = 32                                                                 # int64 words on either side of the counts
A5 = int.from_bytes(bytes([FILL] * 8), "little")


def _counts(raw, k, lags):
    """[k, 256] counts of the planes of the block's raw bytes at this row of lags; (): the bytes as they lie"""
    n = len(raw) // k
    planes = _z_planes(raw, k, lags) if any(lags) else np.frombuffer(raw, np.uint8).reshape(n, k).T
    return np.stack([np.bincount(planes[j], minlength=256) for j in range(k)]).astype(np.uint64)


class _Blocks:
    """blocks (raw bytes, row of lags, element side `a` ELEMENTS behind a multiple of 64 bytes) of k-byte elements: `el` the host
    image of the element side, FILL where no data lies, and `want` the whole count buffer, guards included"""

    def __init__(self, k, blocks):
        self.k, self.nb = k, len(blocks)
        self.n, self.lags, self.off = [len(b[0]) // k for b in blocks], [tuple(b[1]) for b in blocks], []
        pos = 0
        for raw, _, a in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + a * k
            self.off.append(pos)
            pos += len(raw)
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.want = np.full(2 * GUARD + self.nb * k * 256, A5, np.uint64)
        for b, (raw, lags, _) in enumerate(blocks):
            self.el[self.off[b]:self.off[b] + len(raw)] = np.frombuffer(raw, np.uint8)
            self.want[GUARD + b * k * 256:GUARD + (b + 1) * k * 256] = _counts(raw, k, lags).reshape(-1)

    def zero(self, b):
        self.want[GUARD + b * self.k * 256:GUARD + (b + 1) * self.k * 256] = 0


def _freq(nhist):
    """the count buffer: (the whole tensor, 0xA5 everywhere; the view the entry gets)"""
    whole = _fill((2 * GUARD + nhist * 256) * 8).view(_torch().int64)
    return whole, whole[GUARD:GUARD + nhist * 256]


def _torch():
    import torch
    return torch


def _u64img(t):
    return t.cpu().numpy().view(np.uint64)


def _run(shafa, B, cap, dn=None, want_codes=None):
    """one launch over the blocks of B, one finish; the whole count buffer and the element side against the host images"""
    st = _stream()
    bt = shafa.Batch(B.nb, 1 << 20)
    try:
        d_n = _sizes(B.n if dn is None else dn)
        d_el = _to(B.el)
        whole, d_freq = _freq(B.nb * B.k)
        assert d_el.data_ptr() % 16 == 0
        bt.hist_planes_grid_dev(st, B.k, B.lags, d_el, B.off, cap, d_n, d_freq)
        if want_codes is None:
            assert bt.finish(st, B.nb) == (0, [0] * B.nb)
        else:
            assert bt.finish(st, B.nb, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want_codes)
        got = _u64img(whole)
        bad = [(b, B.n[b], B.lags[b]) for b in range(B.nb)
               if got[GUARD + b * B.k * 256:GUARD + (b + 1) * B.k * 256].tobytes()
               != B.want[GUARD + b * B.k * 256:GUARD + (b + 1) * B.k * 256].tobytes()]
        assert not bad, bad[:8]
        assert got.tobytes() == B.want.tobytes()
        assert _img(d_el) == B.el.tobytes()
        return got
    finally:
        bt.close()


# ---------------------------------------------------------------- 1. by hand
def test_eight_elements_worked_out_by_hand(shafa):
    """k = 1, x = 10 12 15 19 24 30 37 45: (): the bytes themselves; (1, 3): z = 20 4 6 11 6 6 6 6; (2, 3, 5): z = 20 24 10 5 5 7 11 2
    (tests/test_gpu_planes_grid.py works them out).  k = 4, x = 1, 2^8, 2^16, 2^24, 0, 0, 0, 2^32 - 1: () counts byte j of each; (1, 3)
    against numpy."""
    raw = bytes([10, 12, 15, 19, 24, 30, 37, 45])
    by_hand = {(): list(raw), (1, 3): [20, 4, 6, 11, 6, 6, 6, 6], (2, 3, 5): [20, 24, 10, 5, 5, 7, 11, 2]}
    for lags, z in by_hand.items():
        want = np.bincount(z, minlength=256)
        assert _counts(raw, 1, lags).tolist() == [want.tolist()], lags
    B = _Blocks(1, [(raw, lags, 1) for lags in by_hand])
    got = _run(shafa, B, [8] * 3)
    assert got[GUARD + 256 + 6] == 5 and got[GUARD + 256 + 20] == 1 and got[GUARD + 10] == 1
    raw4 = np.array([1, 1 << 8, 1 << 16, 1 << 24, 0, 0, 0, (1 << 32) - 1], np.uint32).tobytes()
    plain = _counts(raw4, 4, ())
    for j in range(4):
        assert plain[j, 0] == 6 and plain[j, 1] == 1 and plain[j, 255] == 1 and plain[j].sum() == 8
    _run(shafa, _Blocks(4, [(raw4, (), 0), (raw4, (1, 3), 3), (raw4, (2, 3, 5), 1)]), [8, 9, 13])


# ---------------------------------------------------------------- 2. the kernel: one launch over all the shapes
def _shapes(shafa):
    T = shafa.PLANES_TILE
    out = []
    for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3):
        for lags in ((), (1,), (1, n - 1), (1, n), (1, n + 1), (n - 2, n - 1), (3, 7, 11)):
            if all(g >= 1 for g in lags) and all(a < b for a, b in zip(lags, lags[1:])):
                out += [(n, lags, a) for a in (0, 1, 3)]
    return out


@pytest.mark.parametrize("k", ELEMS)
def test_one_launch_against_numpy(shafa, k):
    rng = np.random.default_rng(400 + k)
    shapes = _shapes(shafa)
    assert len(shapes) > 150
    B = _Blocks(k, [(_random(n, k, rng), lags, a) for n, lags, a in shapes])
    got = _run(shafa, B, [n + 5 for n in B.n])
    sums = got[GUARD:-GUARD].reshape(B.nb, k, 256).sum(2)
    assert (sums == np.array(B.n, np.uint64)[:, None]).all()               # every plane's counts sum to n


# ---------------------------------------------------------------- 3. runs: block borders inside a run, run ends inside a block
@pytest.mark.parametrize("k", (1, 2))
def test_runs_and_hot_bins(shafa, k):
    """capacities n + 5, so the large blocks' tiles number 9, 9, 9 and 18 with 1 .. 3 tiles of a small block in front of each:
    every large block starts inside a run of PLANES_HIST_RUN tiles and has a run end inside it.  Then a block of zeros and one of the single value 0x80...: every lane
    hits one bin of every plane, with and without differences."""
    R, T = shafa.PLANES_HIST_RUN, shafa.PLANES_TILE
    rng = np.random.default_rng(500 + k)
    U = UINT[k]
    big = [R * T - 1, R * T, R * T + 1, 2 * R * T + T + 3]
    small = [17, T + 1, 3, 2 * T + 9]
    rows = [(), (1,), (1, 64), (3, 7, 11)]
    blocks = []
    for i, n in enumerate(big):
        blocks += [(_random(small[i], k, rng), rows[(i + 1) % 4], 1), (_random(n, k, rng), rows[i], (0, 1, 3)[i % 3])]
    smooth = (np.arange(R * T + 77, dtype=np.uint64) // 3).astype(U).tobytes()              # differences of 0 and 1
    blocks += [(smooth, (1,), 0), (smooth, (), 3)]
    hot = U(1) << U(8 * k - 1)
    for v in (U(0), hot):
        const = np.full(R * T + T + 5, v, U).tobytes()
        blocks += [(const, (), 0), (const, (1,), 1), (const, (1, 64), 3)]
    B = _Blocks(k, blocks)
    got = _run(shafa, B, [n + 5 for n in B.n])
    c = got[GUARD:-GUARD].reshape(B.nb, k, 256)
    assert c[-3, k - 1, 0x80] == R * T + T + 5 and c[-6].sum(0)[0] == k * (R * T + T + 5)


# ---------------------------------------------------------------- 4. many blocks in one launch
@pytest.mark.parametrize("k", ELEMS)
def test_nine_blocks_one_launch_one_past_its_capacity(shafa, k):
    """two empty blocks, one past its capacity (OUTSIDE_MODULE, its counts 0), six of mixed sizes, offsets and rows"""
    T = shafa.PLANES_TILE
    rng = np.random.default_rng(30 + k)
    ns = [17, 0, T + 1, 15, 3 * T + 5, 4100, 0, 1024, 2 * T]
    lags = [(1, 3), (), (1, 256), (1, 1 << 40), (1, 5, 300), (), (7, 8, 9), (64,), (3, 257, 8000)]
    B = _Blocks(k, [(_random(n, k, rng), s, (0, 1, 3)[b % 3]) for b, (n, s) in enumerate(zip(ns, lags))])
    bad = 4
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    _run(shafa, B, cap)
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    B.zero(bad)
    _run(shafa, B, cap, dn, [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)])


# ---------------------------------------------------------------- 5. the chooser's shape: candidates on ONE region
CANDS = [(), (1,), (64,), (4096,), (1, 64), (1, 4096), (64, 4096), (1, 64, 4096)]


@pytest.mark.parametrize("k", (2, 4))
def test_eight_candidates_on_one_region(shafa, k):
    rng = np.random.default_rng(600 + k)
    n = 3 * shafa.PLANES_TILE + 21
    raw = _random(n, k, rng)
    B = _Blocks(k, [(raw, CANDS[0], 3)])
    B.nb, B.n, B.lags, B.off = 8, [n] * 8, CANDS, B.off * 8
    B.want = np.full(2 * GUARD + 8 * k * 256, A5, np.uint64)
    B.want[GUARD:-GUARD] = np.concatenate([_counts(raw, k, c).reshape(-1) for c in CANDS])
    _run(shafa, B, [n] * 8)


# ---------------------------------------------------------------- 6. device against device; mixed with other entries; a busy stream
@pytest.mark.parametrize("k", ELEMS)
def test_equals_hist256_over_the_split_entries_planes(shafa, k):
    """split_planes_grid_dev and split_planes_dev into planes, hist256 over them, and the fused entry for the same rows, all on
    one batch behind a large torch kernel, the sizes from a kernel on the stream too: one finish"""
    torch = _torch()
    dev = _dev()
    T = shafa.PLANES_TILE
    rng = np.random.default_rng(700 + k)
    ns = [5 * T + 3, 1000, T, 40000]
    rows = [(1, 64), (3,), (1, 2, 3), (1, 100, 10000)]
    B = _Blocks(k, [(_random(n, k, rng), s, (0, 1, 3)[b % 3]) for b, (n, s) in enumerate(zip(ns, rows))])
    P = _Blocks(k, [(_random(n, k, rng), (), (0, 1, 3)[b % 3]) for b, n in enumerate(ns)])
    al = lambda x: (x + 15) // 16 * 16
    poff, pn, pos = [], [], 0
    for n in ns:
        for _ in range(k):
            poff.append(pos)
            pn.append(n)
            pos += al(n) + 16
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(4 * k, 1 << 20)
    try:
        d_el, d_pel = _to(B.el), _to(P.el)
        d_pl, d_ppl = _fill(pos + 16), _fill(pos + 16)
        half = torch.tensor([[n // 2, n - n // 2] for n in ns], dtype=torch.int64, device=dev)
        wholes = [_freq(4 * k) for _ in range(4)]
        (fg, fg2), (fp, fp2) = [(w[1], x[1]) for w, x in (wholes[:2], wholes[2:])]
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(st):
            busy = torch.empty(1 << 26, dtype=torch.float32, device=dev)
            busy.normal_()                                                 # 256 MiB written
            d_n = half.sum(dim=1)                                          # the sizes exist only behind it
            bt.split_planes_grid_dev(st, k, rows, d_el, B.off, ns, d_n, d_pl, poff)
            bt.hist_planes_grid_dev(st, k, rows, d_el, B.off, ns, d_n, fg)
            bt.hist256(st, d_pl, poff, pn, fg2)
            bt.split_planes_dev(st, k, d_pel, P.off, ns, d_n, d_ppl, poff)
            bt.hist256(st, d_ppl, poff, pn, fp2)
            bt.hist_planes_grid_dev(st, k, [()] * 4, d_pel, P.off, ns, d_n, fp)
            assert bt.finish(st, 4 * k) == (0, [0] * 4 * k)
        assert _u64img(wholes[0][0]).tobytes() == _u64img(wholes[1][0]).tobytes() == B.want.tobytes()
        assert _u64img(wholes[2][0]).tobytes() == _u64img(wholes[3][0]).tobytes() == P.want.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. the drivers
@functools.lru_cache(maxsize=None)
def _reference(shafa):
    """the three tensors of the CPU test and numpy's lists for their default candidates, made once"""
    grids = shafa.grids
    out = []
    for a in three_tensors():
        x = a.reshape(-1).view(UINT[a.dtype.itemsize])
        out.append((a, model_sizes(shafa, x, grids._default_candidates("test", a.shape, None))))
    return out


def test_grid_histograms_equals_the_entry_and_numpy(shafa):
    torch = _torch()
    a = _reference(shafa)[1][0]                                            # the int16 column walk
    t = torch.from_numpy(a).to(_dev())
    sets = [(), (64,), (1, 64), (1,), (5, 64, 4096)]
    got = shafa.grid_histograms(t, sets)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, 2, 256) and got.device == t.device
    x = a.reshape(-1).view(np.uint16)
    want = np.stack([plane_histograms(x, c) for c in sets])
    assert got.cpu().numpy().astype(np.uint64).tobytes() == want.tobytes()
    st = _stream()
    bt = shafa.Batch(5, 1 << 20)
    try:
        whole, d_freq = _freq(5 * 2)
        bt.hist_planes_grid_dev(st, 2, sets, t, [0] * 5, [t.numel()] * 5, _sizes([t.numel()] * 5), d_freq)
        assert bt.finish(st, 5) == (0, [0] * 5)
        assert torch.equal(d_freq.view(5, 2, 256), got)
    finally:
        bt.close()
    assert tuple(shafa.grid_histograms(t, []).shape) == (0, 2, 256)
    e = shafa.grid_histograms(t[:0], [(), (1,)])
    assert tuple(e.shape) == (2, 2, 256) and int(e.abs().sum()) == 0


def test_grid_sizes_and_choose_lags_equal_the_model(shafa):
    """integer for integer, ties included, on the field, the column walk and the noise, in one call and alone"""
    torch = _torch()
    ref = _reference(shafa)
    ts = [torch.from_numpy(a).to(_dev()) for a, _ in ref]
    got = shafa.grid_sizes(ts)
    assert got == [want for _, want in ref]
    assert shafa.choose_lags(ts) == [(1, 4096), (64,), ()]
    assert shafa.grid_sizes(ts[1]) == [ref[1][1]] and shafa.choose_lags(ts[0]) == [(1, 4096)]
    # explicit candidates: one list for all, one list per tensor; explicit axes
    x = [a.reshape(-1).view(UINT[a.dtype.itemsize]) for a, _ in ref]
    cands = [(2, 3), (), (64,)]
    assert shafa.grid_sizes(ts, candidates=cands) == [model_sizes(shafa, v, cands) for v in x]
    per = [[(1, 64, 4096)], [(), (1,)], [(7,), (1, 300), (300,)]]
    assert shafa.grid_sizes(ts, candidates=per) == [model_sizes(shafa, v, c) for v, c in zip(x, per)]
    assert shafa.grid_sizes(ts[0], axes=(0, 2)) == [model_sizes(shafa, x[0], [(), (1,), (4096,), (1, 4096)])]
    # empty and 0-dimensional tensors
    odd = [ts[1][:0], torch.zeros((), dtype=torch.int32, device=_dev()), ts[1], torch.zeros(0, 4, dtype=torch.float64, device=_dev())]
    assert shafa.grid_sizes(odd) == [[((), 0)], [((), 0)], ref[1][1], [((), 0)]]
    assert shafa.choose_lags(odd) == [(), (), (64,), ()]
    assert shafa.grid_sizes(odd[:2]) == [[((), 0)]] * 2 and shafa.grid_sizes([]) == []


DTYPES = ("bfloat16", "float16", "float32", "float64", "int8", "int16", "int32", "int64")


def test_grid_sizes_on_eight_dtypes_in_one_call(shafa):
    """a field smooth along both axes cast to every dtype, as slices at odd element offsets: the sizes against the model on the
    tensors' own bytes"""
    torch = _torch()
    rng = np.random.default_rng(800)
    walk = np.cumsum(np.cumsum(rng.integers(-2, 3, (50, 64)), axis=0), axis=1)
    ts = []
    for i, d in enumerate(DTYPES):
        whole = torch.from_numpy(walk).to(_dev()).to(getattr(torch, d)).reshape(-1)
        buf = torch.zeros(whole.numel() + 8, dtype=whole.dtype, device=_dev())
        buf[1 + i % 3:1 + i % 3 + whole.numel()] = whole
        ts.append(buf[1 + i % 3:1 + i % 3 + whole.numel()].view(50, 64))
    got = shafa.grid_sizes(ts)
    picks = shafa.choose_lags(ts)
    for d, t, g, p in zip(DTYPES, ts, got, picks):
        k = t.element_size()
        x = np.frombuffer(t.contiguous().view(torch.uint8).cpu().numpy().tobytes(), UINT[k])
        want = model_sizes(shafa, x, [(), (1,), (64,), (1, 64)])
        assert g == want and p == want[0][0], d


def test_histogram_drivers_past_one_launch(shafa, monkeypatch):
    """HIST_GROUP candidates go into one launch, and no other test passes more than that: with a group of 3 seven entries take
    launches of 3, 3 and 1 blocks on a batch of 3 — the slices of the lag sets, of the parameters, of freq and of the outliers'
    counts, and d_n used again.  grid_histograms, field_histograms and rounded_histograms then give, bit for bit, what one launch
    gives, which the tests of each tie to numpy.  Seven different lag sets, bounds and keeps on 8200 floats, just past two tiles,
    with NaNs and with denormals of one low bit each at different places, so that every entry has its own counts and, under the
    rounding, its own number of outliers: a slice handed to the wrong entry shows."""
    torch = _torch()
    grids = shafa.grids
    rng = np.random.default_rng(4096)
    a = np.cumsum(rng.normal(0, 1, 5 * 40 * 41)).astype(np.float32)
    a[[7, 4095, 4096, 8199]] = np.nan
    low = (0, 3, 7, 11, 15, 19, 22)                                        # a keep of 23 - d drops the bits below d
    a.view(np.uint32)[[100 + 1000 * i for i in range(7)]] = [1 << p for p in low]
    t = torch.from_numpy(a.reshape(5, 40, 41)).to(_dev())
    sets = [(1, 1640), (1,), (41,), (1640,), (1, 41), (41, 1640), (1, 41, 1640)]
    errs = [0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 0.0003]
    keeps = [23, 20, 16, 12, 8, 4, 1]

    def run():
        return (shafa.grid_histograms(t, [()] + sets[1:]), *shafa.field_histograms(t, errs, sets),
                *shafa.rounded_histograms(t, keeps, [()] + sets[1:]))

    assert grids.HIST_GROUP >= 7
    one = run()
    monkeypatch.setattr(grids, "HIST_GROUP", 3)
    three = run()
    assert [tuple(x.shape) for x in one] == [(7, 4, 256), (7, 4, 256), (7,), (7, 4, 256), (7,)]
    for x, y in zip(one, three):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    for freq in (one[0], one[1], one[3]):
        assert len({freq[i].cpu().numpy().tobytes() for i in range(7)}) > 1
    print(f"past one launch: outliers under the bounds {one[2].tolist()}, under the keeps {one[4].tolist()}")
    assert len(set(one[4].tolist())) > 1


# ---------------------------------------------------------------- 8. what the chooser is worth
def test_it_pays(shafa):
    """DESIGN 7.28's field: the chooser's pick compresses below every single axis and below plain planes, the model's margins are
    2.5 x or more; only < is asserted.  The default of all three axes is printed next to it."""
    torch = _torch()
    a = _reference(shafa)[0][0]
    t = torch.from_numpy(a).to(_dev())
    pick = shafa.choose_lags(t)[0]
    assert pick == _reference(shafa)[0][1][0][0]
    chosen = shafa.compress_grids(t, lags=[pick])[0]
    default = shafa.compress_grids(t)[0]
    plain = shafa.compress_tensors(t)[0].nbytes
    single = [shafa.compress_strided(t, axis=ax)[0].nbytes for ax in (0, 1, 2)]
    print(f"it pays: raw {a.nbytes}, plain planes {plain}, one axis (0, 1, 2) {single}, all axes {default.nbytes}, "
          f"choose_lags' {pick} {chosen.nbytes}")
    assert all(chosen.nbytes < s for s in single) and chosen.nbytes < plain
    assert _same(shafa.decompress_grids(chosen)[0], t)

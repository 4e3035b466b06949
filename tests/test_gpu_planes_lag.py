"""shafa_hipd_split_planes_lag_dev / shafa_hipd_merge_planes_lag_dev (csrc/planes_lag.hip) and the strided drivers on top against
numpy on the host.  With x the block's elements as unsigned little-endian integers of k bytes and L the block's lag, the planes
are those of z = fold(x[i] - x[i-L]), x[i] = 0 for i < 0 (include/shafa_hip.h: "Byte planes of lagged differences"), here a
shifted subtraction on the raw bytes; merge's expectation is the padded reshape(R, L).cumsum(0) of the unfolded z, on RANDOM planes
as well as on split's.  Nothing is compared with device code but for the lag-1 test, whose other side is the _diff_dev entries.

The shapes are the borders of the kernels: a lane has 16 elements, a wave 1024, a pass of the workgroup 4096, a tile
T = PLANES_TILE; merge cuts a block of lag L into chunks of G rows (_geom, the header's rule from the module's PLANES_LAG_*
constants), whose borders are multiples of G L elements, and the forms change at L = PLANES_LAG_STRIP and wherever
PLANES_LAG_STRIP // L does.  Every buffer holds 0xA5 where no data lies, and every comparison is of whole images."""
import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
FILL = 0xA5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _al16(x):
    return (x + 15) // 16 * 16


def _geom(shafa, cap, lag):
    """the header's form of a block: (lag clamped, W, S, m, G, chunks of the capacity)"""
    strip, rows_lane, items = shafa.PLANES_LAG_STRIP, shafa.PLANES_LAG_ROWS, shafa.PLANES_LAG_ITEMS
    L = min(lag, max(cap, 1))
    W = min(L, strip)
    S = strip // W
    NS = -(-L // W)
    g0 = rows_lane * S
    rows = -(-cap // L)
    m = max(1, NS * -(-rows // g0) // items)
    G = g0 * m
    return L, W, S, m, G, -(-rows // G)


def _fold(d, U, k):
    return (d << U(1)) ^ (U(0) - (d >> U(8 * k - 1)))


def _unfold(z, U):
    return (z >> U(1)) ^ (U(0) - (z & U(1)))


def _z_planes(raw, k, lag):
    """split's expectation: [k, n] bytes, row j byte j of the folded differences at distance lag"""
    U = UINT[k]
    x = np.frombuffer(raw, U)
    d = x.copy()
    if lag < x.size:
        d[lag:] -= x[:-lag]                                                # wraps mod M
    return _fold(d, U, k).view(np.uint8).reshape(-1, k).T


def _x_bytes(planes, k, lag):
    """merge's expectation from the planes [k, n]: the prefix sums down the columns of the rows of `lag` elements"""
    U = UINT[k]
    z = np.ascontiguousarray(planes.T).view(U).reshape(-1)
    n = z.size
    L = min(lag, max(n, 1))
    R = -(-n // L)
    d = np.zeros(R * L, U)
    d[:n] = _unfold(z, U)
    return np.cumsum(d.reshape(R, L), axis=0, dtype=U).reshape(-1)[:n].tobytes()


def _random(n, k, rng):
    U = UINT[k]
    x = np.frombuffer(rng.integers(0, 256, n * k, dtype=np.uint8).tobytes(), U).copy()
    if n:
        x[0] |= U(int(np.iinfo(U).max) // 2 + 1)
    return x.tobytes()


class _Layout:
    """blocks (n elements, lag, element side `a` ELEMENTS behind a multiple of 64 bytes) of k-byte elements in host images:
    `el` the element side and `pl` numpy's planes of its folded differences; `zpl` random planes and `zel` numpy's merge of
    them.  All FILL where no data lies, 16 guard bytes or more around every region."""

    def __init__(self, k, blocks, seed, a_out=None):
        rng = np.random.default_rng(seed)
        self.k, self.n, self.lag = k, [b[0] for b in blocks], [b[1] for b in blocks]
        self.off, self.poff = [], []
        pos, ppos = 0, 16
        for n, _, a in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + (a if a_out is None else a_out) * k
            self.off.append(pos)
            pos += n * k
            for _ in range(k):
                self.poff.append(ppos)
                ppos += _al16(n) + 32
        self.raw = [_random(n, k, rng) for n in self.n]
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.pl = np.full(ppos + 16, FILL, np.uint8)
        self.zel, self.zpl = self.el.copy(), self.pl.copy()
        for b, (n, lag) in enumerate(zip(self.n, self.lag)):
            self.el[self.off[b]:self.off[b] + n * k] = np.frombuffer(self.raw[b], np.uint8)
            planes = _z_planes(self.raw[b], k, lag)
            assert _x_bytes(planes, k, lag) == self.raw[b]                 # numpy's inverse of numpy's transform
            zp = rng.integers(0, 256, (k, n), dtype=np.uint8)
            self.zel[self.off[b]:self.off[b] + n * k] = np.frombuffer(_x_bytes(zp, k, lag), np.uint8)
            for j in range(k):
                self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = planes[j]
                self.zpl[self.poff[b * k + j]:self.poff[b * k + j] + n] = zp[j]

    def blank(self, b):
        """block b leaves no trace in any image"""
        n, k = self.n[b], self.k
        for img in (self.el, self.zel):
            img[self.off[b]:self.off[b] + n * k] = FILL
        for j in range(k):
            for img in (self.pl, self.zpl):
                img[self.poff[b * k + j]:self.poff[b * k + j] + n] = FILL


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(_dev())


def _fill(n):
    import torch
    return torch.full((n,), FILL, dtype=torch.uint8, device=_dev())


def _img(t):
    return t.cpu().numpy().tobytes()


def _sizes(ns):
    import torch
    return torch.tensor(ns, dtype=torch.int64, device=_dev())


def test_six_bytes_worked_out_by_hand(shafa):
    """k = 1, M = 256: the planes of six bytes at lags 2, 6 and 2^40 written out by hand, against the entries in both directions
    and against this file's numpy expectation, which every other test leans on"""
    import torch
    raw = bytes([200, 10, 201, 8, 0, 9])
    # lag 2: d = 200, 10, 1, 254 (-2), 55, 1;  z = (d << 1) ^ (255 if d >= 128).  A lag at or past the size: the fold of x
    by_hand = {2: [144 ^ 255, 20, 2, 252 ^ 255, 110, 2]}
    by_hand[6] = by_hand[1 << 40] = [144 ^ 255, 20, 146 ^ 255, 16, 0, 18]
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes([6])
        for lag, z in by_hand.items():
            assert _z_planes(raw, 1, lag).tolist() == [z] and _x_bytes(np.array([z], np.uint8), 1, lag) == raw, lag
            el = np.full(64, FILL, np.uint8)
            el[16:22] = np.frombuffer(raw, np.uint8)
            d_el, d_pl, d_out = _to(el), _fill(64), _fill(64)
            bt.split_planes_lag_dev(st, 1, [lag], d_el, [16], [6], d_n, d_pl, [32])
            bt.merge_planes_lag_dev(st, 1, [lag], d_pl, [32], [6], d_n, d_out, [19])
            assert bt.finish(st, 1) == (0, [0])
            assert _img(d_pl) == bytes([FILL] * 32 + z + [FILL] * 26), lag
            assert _img(d_out) == bytes([FILL] * 19) + raw + bytes([FILL] * 39), lag
    finally:
        bt.close()
    assert _x_bytes(_z_planes(raw, 1, 5), 1, 5) == raw and _x_bytes(_z_planes(raw, 1, 7), 1, 7) == raw


def _blocks(shafa):
    """(n, lag, offset in elements): the issue's lags and the forms' thresholds against the unit, wave, pass, tile and chunk
    borders"""
    T, strip = shafa.PLANES_TILE, shafa.PLANES_LAG_STRIP
    counts = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, T - 1, T, T + 1, 3 * T + 5)
    lags = [1, 2, 3, 5, 16, 17, 64, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 40000, 1 << 40]
    lags += [strip - 1, strip, strip + 1]                                  # a strip of the block's own width -> 256 columns
    lags += [strip // 3, strip // 3 + 1, strip // 2 - 1, strip // 2, strip // 2 + 1]       # 3 -> 2 -> 1 segments of rows
    out = []
    for i, lag in enumerate(dict.fromkeys(lags)):
        ns = [counts[(4 * i + j) % len(counts)] for j in range(4)]
        L, W, S, m, G, _ = _geom(shafa, 1 << 20, lag)
        assert m == 1
        chunk = G * L                                                      # elements of a chunk of whole rows
        if chunk <= 3 * T:
            ns += [chunk - 1, chunk, chunk + 1, chunk + L, 2 * chunk + L + 1, 3 * chunk + 7]
        elif chunk <= 300000:
            ns += [chunk + 1, 2 * chunk + L + 1]
        elif lag < 1 << 20:
            ns += [chunk + L + 1]
        out += [(n, lag) for n in ns]
    for n in (17, 4097, T + 1, 3 * T + 5):
        out += [(n, n - 1), (n, n), (n, n + 1)]
    out += [(0, 1 << 40), (1, 1 << 40), (3 * T + 5, (1 << 64) - 1)]
    return [(n, lag, (0, 1, 3)[b % 3]) for b, (n, lag) in enumerate(out)]


# ---------------------------------------------------------------- 1. the kernels: one launch each way over all the shapes
@pytest.mark.parametrize("k", ELEMS)
def test_one_launch_each_way_against_numpy(shafa, k):
    import torch
    blocks = _blocks(shafa)
    L = _Layout(k, blocks, 100 + k)
    nb = len(blocks)
    cap = [n + 5 for n in L.n]
    assert any(_geom(shafa, c, g)[5] > 2 for c, g in zip(cap, L.lag)) and any(_geom(shafa, c, g)[2] > 1 for c, g in zip(cap, L.lag))
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_n = _sizes(L.n)
        d_el, d_pl = _to(L.el), _fill(L.pl.size)
        assert d_el.data_ptr() % 16 == 0 and d_pl.data_ptr() % 16 == 0
        bt.split_planes_lag_dev(st, k, L.lag, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb)
        got, want = d_pl.cpu().numpy(), L.pl
        bad = [(L.n[b], L.lag[b]) for b in range(nb)
               if any(got[o:o + L.n[b]].tobytes() != want[o:o + L.n[b]].tobytes() for o in L.poff[b * k:b * k + k])]
        assert not bad, bad[:8]
        assert got.tobytes() == want.tobytes()
        assert _img(d_el) == L.el.tobytes()
        # merge: numpy's planes of the data, then random planes
        for pl, el in ((L.pl, L.el), (L.zpl, L.zel)):
            d_pl, d_out = _to(pl), _fill(el.size)
            bt.merge_planes_lag_dev(st, k, L.lag, d_pl, L.poff, cap, d_n, d_out, L.off)
            assert bt.finish(st, nb) == (0, [0] * nb)
            got = d_out.cpu().numpy()
            bad = [(L.n[b], L.lag[b]) for b in range(nb)
                   if got[L.off[b]:L.off[b] + L.n[b] * k].tobytes() != el[L.off[b]:L.off[b] + L.n[b] * k].tobytes()]
            assert not bad, bad[:8]
            assert got.tobytes() == el.tobytes()
            assert _img(d_pl) == pl.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("k", ELEMS)
def test_lag_1_is_the_diff_entries_and_a_round_trip(shafa, k):
    """lag 1 against split_planes_diff_dev / merge_planes_diff_dev byte for byte, and split -> merge back to back on the stream
    into another offset, at mixed lags"""
    import torch
    T = shafa.PLANES_TILE
    ns = [0, 1, 17, 1025, 4097, T + 1, 3 * T + 5]
    L = _Layout(k, [(n, 1, (0, 1, 3)[b % 3]) for b, n in enumerate(ns)], 200 + k)
    nb = len(ns)
    cap = [n + 5 for n in ns]
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = _sizes(ns)
        d_el, d_a, d_b = _to(L.el), _fill(L.pl.size), _fill(L.pl.size)
        bt.split_planes_lag_dev(st, k, [1] * nb, d_el, L.off, cap, d_n, d_a, L.poff)
        bt.split_planes_diff_dev(st, k, d_el, L.off, cap, d_n, d_b, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_a) == _img(d_b) == L.pl.tobytes()
        d_pl, d_a, d_b = _to(L.zpl), _fill(L.el.size), _fill(L.el.size)
        bt.merge_planes_lag_dev(st, k, [1] * nb, d_pl, L.poff, cap, d_n, d_a, L.off)
        bt.merge_planes_diff_dev(st, k, d_pl, L.poff, cap, d_n, d_b, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_a) == _img(d_b) == L.zel.tobytes()
        # the round trip into another offset
        lags = [1, 1, 5, 300, 4097, 64, 8193]
        blocks = [(n, g, (0, 1, 3)[b % 3]) for b, (n, g) in enumerate(zip(ns, lags))]
        L1, L2 = _Layout(k, blocks, 210 + k), _Layout(k, blocks, 210 + k, a_out=2)
        assert L1.raw == L2.raw and L1.off != L2.off
        d_el, d_mid, d_back = _to(L1.el), _fill(L1.pl.size), _fill(L2.el.size)
        bt.split_planes_lag_dev(st, k, lags, d_el, L1.off, cap, d_n, d_mid, L1.poff)
        bt.merge_planes_lag_dev(st, k, lags, d_mid, L1.poff, cap, d_n, d_back, L2.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_mid) == L1.pl.tobytes()
        assert _img(d_back) == L2.el.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("lag", (1, 3, 300, 100003))
@pytest.mark.parametrize("k", (1, 8))
def test_a_block_of_many_chunks(shafa, k, lag):
    """257 T + 3 elements: every form has many chunks (but lag 100 003, whose 22 rows are one), and the scan of lag 300, eight
    chunks a lane and eight lanes a column, takes several rounds"""
    import torch
    n = 257 * shafa.PLANES_TILE + 3
    L = _Layout(k, [(n, lag, 3)], 60 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes([n])
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_lag_dev(st, k, [lag], d_el, L.off, [n + 5], d_n, d_pl, L.poff)
        assert bt.finish(st, 1) == (0, [0])
        assert _img(d_pl) == L.pl.tobytes()
        d_pl = _to(L.zpl)
        bt.merge_planes_lag_dev(st, k, [lag], d_pl, L.poff, [n + 5], d_n, d_out, L.off)
        assert bt.finish(st, 1) == (0, [0])
        assert _img(d_out) == L.zel.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. many blocks in one launch
@pytest.mark.parametrize("k", ELEMS)
def test_nine_blocks_one_launch_one_past_its_capacity(shafa, k):
    """two empty blocks, one past its capacity (OUTSIDE_MODULE, no byte of it touched, the others right), six of mixed sizes,
    offsets and lags"""
    import torch
    T = shafa.PLANES_TILE
    ns = [17, 0, T + 1, 15, 3 * T + 5, 4100, 0, 1024, 2 * T]
    lags = [3, 1, 256, 1 << 40, 5, 4100, 7, 64, 257]
    L = _Layout(k, [(n, g, (0, 1, 3)[b % 3]) for b, (n, g) in enumerate(zip(ns, lags))], 30 + k)
    bad = 4
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    want = [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)]
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = _sizes(dn)
        full_pl, full_el, full_zpl, full_zel = L.pl.copy(), L.el.copy(), L.zpl.copy(), L.zel.copy()
        L.blank(bad)
        d_el, d_pl = _to(full_el), _fill(L.pl.size)
        bt.split_planes_lag_dev(st, k, lags, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_pl) == L.pl.tobytes()
        assert _img(d_el) == full_el.tobytes()
        d_pl, d_out = _to(full_zpl), _fill(L.el.size)
        bt.merge_planes_lag_dev(st, k, lags, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_out) == L.zel.tobytes()
        assert _img(d_pl) == full_zpl.tobytes()
        # all nine within their capacities
        d_n = _sizes(ns)
        d_pl, d_out = _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_lag_dev(st, k, lags, d_el, L.off, cap, d_n, d_pl, L.poff)
        bt.merge_planes_lag_dev(st, k, lags, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9) == (0, [0] * 9)
        assert _img(d_pl) == full_pl.tobytes() and _img(d_out) == full_el.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("k,lag", ((1, 1), (4, 300), (2, 5000)))
def test_runs_of_tiles_per_workgroup_and_grown_chunks(shafa, k, lag):
    """32775 tiles in the capacities with small sizes: three tiles a workgroup, runs that start in one block and end in the next.
    The form is the capacity's: the middle block's 2^28 elements make more than PLANES_LAG_ITEMS items, so its chunks are m > 1
    rounds long, and its size is three of them and a bit"""
    import torch
    T = shafa.PLANES_TILE
    _, W, S, m, G, _ = _geom(shafa, 1 << 28, lag)
    assert m > 1
    mid = 3 * G * lag + lag + 7
    ns = [3 * T + 5, mid, 20000]
    cap = [3 * T + 5, 1 << 28, 20000]
    lags = [3, lag, 129]
    L = _Layout(k, [(n, g, a) for n, g, a in zip(ns, lags, (1, 3, 0))], 50 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes(ns)
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_lag_dev(st, k, lags, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 3) == (0, [0, 0, 0])
        assert _img(d_pl) == L.pl.tobytes()
        d_pl = _to(L.zpl)
        bt.merge_planes_lag_dev(st, k, lags, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 3) == (0, [0, 0, 0])
        assert _img(d_out) == L.zel.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("k,lag", ((2, 1), (1, 256)))
def test_the_capacity_at_which_chunks_grow(shafa, k, lag):
    """two blocks in one launch whose capacities make 2 PLANES_LAG_ITEMS - 1 items (chunks of one round) and 2 PLANES_LAG_ITEMS
    (of two), each with three chunks of data and a bit"""
    import torch
    items = shafa.PLANES_LAG_ITEMS
    round_ = _geom(shafa, 1 << 20, lag)[4] * lag                           # elements of a round of whole rows, all strips
    cap = [(2 * items - 1) * round_, 2 * items * round_]
    gs = [_geom(shafa, c, lag) for c in cap]
    assert [g[3] for g in gs] == [1, 2]
    ns = [3 * g[4] * lag + lag + 7 for g in gs]
    L = _Layout(k, [(n, lag, a) for n, a in zip(ns, (1, 3))], 90 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes(ns)
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_lag_dev(st, k, [lag, lag], d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 2) == (0, [0, 0])
        assert _img(d_pl) == L.pl.tobytes()
        d_pl = _to(L.zpl)
        bt.merge_planes_lag_dev(st, k, [lag, lag], d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 2) == (0, [0, 0])
        assert _img(d_out) == L.zel.tobytes()
    finally:
        bt.close()


def test_behind_a_busy_stream_one_finish(shafa):
    """2^20 + 3 elements of 2 bytes at lag 64 and 2^19 + 1 of 8 at lag 4097, split and merged back behind a large torch kernel on
    the same stream; the sizes come from a kernel on that stream too.  Nothing is synchronised in between: one finish."""
    import torch
    dev = _dev()
    cases = [(2, (1 << 20) + 3, 64, 3), (8, (1 << 19) + 1, 4097, 1)]
    Ls = [_Layout(k, [(n, g, a)], 77 + k) for k, n, g, a in cases]
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_el = [_to(L.el) for L in Ls]
        d_pl = [_fill(L.pl.size) for L in Ls]
        d_out = [_fill(L.el.size) for L in Ls]
        half = torch.tensor([[c[1] // 2, c[1] - c[1] // 2] for c in cases], dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(st):
            busy = torch.empty(1 << 26, dtype=torch.float32, device=dev)
            busy.normal_()                                                 # 256 MiB written
            d_n = half.sum(dim=1)                                          # the sizes exist only behind it
            for i, (k, n, g, a) in enumerate(cases):
                bt.split_planes_lag_dev(st, k, [g], d_el[i], Ls[i].off, [n], d_n[i:i + 1], d_pl[i], Ls[i].poff)
            for i, (k, n, g, a) in enumerate(cases):
                bt.merge_planes_lag_dev(st, k, [g], d_pl[i], Ls[i].poff, [n], d_n[i:i + 1], d_out[i], Ls[i].off)
            assert bt.finish(st, 1) == (0, [0])
        for i, L in enumerate(Ls):
            assert _img(d_pl[i]) == L.pl.tobytes(), cases[i]
            assert _img(d_out[i]) == L.el.tobytes(), cases[i]
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. compress_strided -> decompress_strided
SHAPES = ((1000,), (125, 8), (17, 5, 3), (0, 4))
DTYPES = ("int64", "int32", "int16", "uint8", "bfloat16", "float32", "float64")


def _bits(t):
    return t.reshape(-1).view(__import__("torch").uint8)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(_bits(a), _bits(b))


def _tensor(dtype, shape, seed, lead=0):
    """a tensor of `dtype` and `shape` of random bit patterns — every NaN payload, both zeros, the denormals — as a slice `lead`
    elements into its storage, and its raw bytes"""
    import torch
    dt = getattr(torch, dtype)
    k = torch.empty((), dtype=dt).element_size()
    n = int(np.prod(shape))
    raw = _random(n, k, np.random.default_rng(seed))
    whole = torch.empty((lead + n + 3) * k, dtype=torch.uint8, device=_dev()).view(dt)
    t = whole[lead:lead + n].view(shape)
    _bits(t).copy_(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()))
    assert t.is_contiguous() and t.storage_offset() == lead
    return t, raw


def _check_item(shafa, t, ct, raw, lag):
    """the item's type and fields, and every plane — a coded one decoded alone — against numpy's plane of z"""
    import torch
    k, n = t.element_size(), t.numel()
    assert type(ct) is shafa.CompressedStrided and ct.lag == lag
    assert ct.dtype == t.dtype and tuple(ct.shape) == tuple(t.shape) and len(ct.planes) == k
    want = _z_planes(raw, k, lag)
    total = 0
    for j, p in enumerate(ct.planes):
        if isinstance(p, dict):
            total += sum(int(f.numel()) for f in p.values())
            got = shafa.decompress_files(**shafa.plane_files(p))
        else:
            assert isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and int(p.numel()) == n
            total += n
            got = p
        assert got.cpu().numpy().tobytes() == want[j].tobytes(), j
    assert ct.nbytes == total


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip_is_bit_exact_at_every_axis(shafa, dtype):
    made, axes, lags = [], [], []
    for i, shape in enumerate(SHAPES):
        for ax in range(len(shape)):
            made.append(_tensor(dtype, shape, 11 * i + ax + len(dtype), lead=(1, 3, 5)[(i + ax) % 3]))
            axes.append(ax if (i + ax) % 2 else ax - len(shape))
            lags.append(int(np.prod(shape[ax + 1:])) if np.prod(shape) else 1)
    ts = [m[0] for m in made]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_strided(ts, axis=axes)
    assert len(cts) == len(ts)
    for t, ct, (_, raw), g in zip(ts, cts, made, lags):
        _check_item(shafa, t, ct, raw, g)
    back = shafa.decompress_strided(cts)
    for b, k, t in zip(back, keep, ts):
        assert _same(b, k) and _same(t, k), (dtype, tuple(t.shape))
    # one axis for all, one item alone, an explicit lag on a flat buffer, and the single-tensor calls
    cts = shafa.compress_strided(ts[1:3], axis=0)
    assert [c.lag for c in cts] == [8, 8]
    assert _same(shafa.decompress_strided(cts[0])[0], keep[1])
    flat = ts[3].reshape(-1)
    ct = shafa.compress_strided(flat, lag=15)[0]
    _check_item(shafa, flat, ct, made[3][1], 15)
    assert _same(shafa.decompress_strided([ct])[0], keep[3].reshape(-1))
    planes = shafa.split_strided(ts[4], 3)
    assert planes.cpu().numpy().tobytes() == _z_planes(made[4][1], ts[4].element_size(), 3).tobytes()
    assert _same(shafa.merge_strided(planes, ts[4].dtype, ts[4].shape, 3), keep[4])


def test_eleven_tensors_with_different_lags_in_one_call(shafa):
    spec = [("float32", (50, 100), 0), ("float16", (0,), 0), ("int64", (4096,), 0), ("bfloat16", (16, 64, 64), 1), ("int32", (), 0),
            ("uint8", (4099, 1), 0), ("int16", (10, 100), -1), ("float64", (3, 1000), 0), ("int64", (32, 32), -2), ("int16", (2049,), -1),
            ("int32", (7, 11, 15), 0)]
    lags = [100, 1, 1, 64, 1, 1, 1, 1000, 32, 1, 165]
    made = [_tensor(d, s, 300 + i, lead=i % 4) for i, (d, s, _) in enumerate(spec)]
    ts = [m[0] for m in made]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_strided(ts, axis=[a for _, _, a in spec], block_size=65536)
    assert [c.lag for c in cts] == lags
    for t, ct, (_, raw), g in zip(ts, cts, made, lags):
        _check_item(shafa, t, ct, raw, g)
    for i, (b, k) in enumerate(zip(shafa.decompress_strided(cts), keep)):
        assert _same(b, k), spec[i]
    order = [10, 3, 2, 3, 0]                                               # another order, one item twice
    for i, b in zip(order, shafa.decompress_strided([cts[i] for i in order])):
        assert _same(b, keep[i]), spec[i]


def test_the_last_axis_is_compress_sequences(shafa):
    t, raw = _tensor("int32", (5000,), 7, lead=1)
    a, b = shafa.compress_strided(t, axis=-1)[0], shafa.compress_sequences(t)[0]
    assert a.lag == 1 and a.nbytes == b.nbytes
    for p, q in zip(a.planes, b.planes):
        assert type(p) is type(q)
        if isinstance(p, dict):
            assert sorted(p) == sorted(q) and all(_img(p[f]) == _img(q[f]) for f in p)
        else:
            assert _img(p) == _img(q)


# ---------------------------------------------------------------- 4. what the lag is worth
def _walks(rng, rows, cols, step, dtype, offsets=None):
    x = np.cumsum(rng.integers(-step, step + 1, (rows, cols)), axis=0)
    if offsets is not None:
        x = x + offsets
    return x.astype(dtype)


def test_it_pays(shafa):
    """The first three tensors of the table in DESIGN 7.26, from a fixed seed: per channel random walks as int16 [4096, 64] and as
    int32 [65536, 3] (far-apart offsets), and a uint8 [256, 256, 3] image of gradients plus two bits of noise, along H and along
    W.  The entropy model puts the lagged planes at 0.37 to 0.61 of the better of the other two; only < is asserted."""
    import torch
    rng = np.random.default_rng(2026)
    yy, xx = np.mgrid[0:256, 0:256]
    img = (np.stack([yy + xx // 2, 255 - xx, (yy * 3 + xx) // 4], axis=2) + rng.integers(0, 4, (256, 256, 3))).astype(np.uint8)
    cases = [("int16 [4096, 64]", _walks(rng, 4096, 64, 300, np.int16), 0),
             ("int32 [65536, 3]", _walks(rng, 65536, 3, 1000, np.int32, np.array([0, 1 << 24, -(1 << 28)])), 0),
             ("uint8 [256, 256, 3] along W", img, 1), ("uint8 [256, 256, 3] along H", img, 0)]
    for name, x, axis in cases:
        t = torch.from_numpy(x).to(_dev())
        lagged = shafa.compress_strided(t, axis=axis)[0]
        plain, flat = shafa.compress_tensors(t)[0], shafa.compress_sequences(t)[0]
        print(f"it pays: {name}: raw {x.nbytes}, plain planes {plain.nbytes}, lag 1 {flat.nbytes}, lag {lagged.lag} {lagged.nbytes}")
        assert lagged.nbytes < plain.nbytes and lagged.nbytes < flat.nbytes, name
        assert _same(shafa.decompress_strided(lagged)[0], t)


# ---------------------------------------------------------------- 5. errors
def test_corruption_is_reported_and_the_next_call_succeeds(shafa):
    import torch
    rng = np.random.default_rng(5)
    t = torch.from_numpy(_walks(rng, 8192, 8, 300, np.int32)).to(_dev())
    ct = shafa.compress_strided(t)[0]
    CS = shafa.CompressedStrided
    coded = [j for j, p in enumerate(ct.planes) if isinstance(p, dict)]
    assert coded and ct.lag == 8
    j = coded[0]
    # a truncated .shaf
    entry = dict(ct.planes[j])
    key = ".rle.shaf" if ".rle.shaf" in entry else ".shaf"
    entry[key] = entry[key][:-1]
    planes = list(ct.planes)
    planes[j] = entry
    with pytest.raises(shafa.ShafaError):
        shafa.decompress_strided(CS(ct.dtype, ct.shape, ct.lag, planes, ct.nbytes - 1))
    assert _same(shafa.decompress_strided(ct)[0], t)
    # a plane of another length
    planes[j] = torch.zeros(t.numel() - 16, dtype=torch.uint8, device=_dev())
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_strided(CS(ct.dtype, ct.shape, ct.lag, planes, 0))
    assert e.value.code == shafa.FILE_UNRECOGNIZABLE
    assert _same(shafa.decompress_strided(ct)[0], t)

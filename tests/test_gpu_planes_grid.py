"""shafa_hipd_split_planes_grid_dev / shafa_hipd_merge_planes_grid_dev (csrc/planes_lag.hip) and the grid drivers on top against
numpy on the host.  With x the block's elements as unsigned little-endian integers of k bytes and L1 < L2 < L3 the block's lags,
the planes are those of z = fold((1 - S^L1)(1 - S^L2)(1 - S^L3) x), x[i] = 0 for i < 0 (include/shafa_hip.h: "Byte planes of
Lorenzo differences"), here successive shifted subtractions on the raw bytes (test_planes_grid_cpu.grid_diff); merge's
expectation is one padded reshape(R, L).cumsum(0) per lag of the unfolded z (grid_sum), on RANDOM planes as well as on split's.
Nothing is compared with device code but for the test of one lag a block, whose other sides are the _lag_dev and _diff_dev entries,
and the two driver comparisons with compress_sequences and compress_strided.

The shapes are the borders of the kernels: a lane has 16 elements, a tile T = PLANES_TILE; every pass of merge cuts a block into
chunks of G rows of its lag (test_gpu_planes_lag._geom), whose borders are multiples of G L elements.  Every buffer holds 0xA5
where no data lies, and every comparison is of whole images."""
import numpy as np
import pytest

from test_gpu_planes_lag import (ELEMS, FILL, UINT, _al16, _fill, _fold, _geom, _img, _random, _same, _sizes, _tensor, _to,
                                 _unfold)
from test_gpu_unpack import _dev
from test_planes_grid_cpu import grid_diff, grid_sum

pytestmark = pytest.mark.gpu

TOP = (1 << 64) - 1


def _z_planes(raw, k, lags):
    """split's expectation: [k, n] bytes, row j byte j of the folded differences along `lags`"""
    U = UINT[k]
    with np.errstate(over="ignore"):
        d = grid_diff(np.frombuffer(raw, U).copy(), [g for g in lags if g])
    return _fold(d, U, k).view(np.uint8).reshape(-1, k).T


def _x_bytes(planes, k, lags):
    """merge's expectation from the planes [k, n]: per lag the prefix sums down the columns of the rows of that many elements"""
    U = UINT[k]
    z = np.ascontiguousarray(planes.T).view(U).reshape(-1)
    with np.errstate(over="ignore"):
        return grid_sum(_unfold(z, U), [g for g in lags if g]).tobytes()


class _Layout:
    """blocks (n elements, tuple of lags, element side `a` ELEMENTS behind a multiple of 64 bytes) of k-byte elements in host
    images: `el` the element side and `pl` numpy's planes of its folded differences; `zpl` random planes and `zel` numpy's merge
    of them.  All FILL where no data lies, 16 guard bytes or more around every region."""

    def __init__(self, k, blocks, seed, a_out=None):
        rng = np.random.default_rng(seed)
        self.k, self.n, self.lags = k, [b[0] for b in blocks], [tuple(b[1]) for b in blocks]
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
        for b, (n, lags) in enumerate(zip(self.n, self.lags)):
            self.el[self.off[b]:self.off[b] + n * k] = np.frombuffer(self.raw[b], np.uint8)
            planes = _z_planes(self.raw[b], k, lags)
            assert _x_bytes(planes, k, lags) == self.raw[b]                # numpy's inverse of numpy's transform
            zp = rng.integers(0, 256, (k, n), dtype=np.uint8)
            self.zel[self.off[b]:self.off[b] + n * k] = np.frombuffer(_x_bytes(zp, k, lags), np.uint8)
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


def _stream():
    import torch
    return torch.cuda.Stream(device=_dev())


# ---------------------------------------------------------------- 1. by hand
def test_eight_bytes_worked_out_by_hand(shafa):
    """k = 1, x = 10 12 15 19 24 30 37 45 (second differences of 1).
    Lags (1, 3): (1 - S) x = 10 2 3 4 5 6 7 8, then (1 - S^3): d = 10 2 3 -6 3 3 3 3, z = 2 d or -2 d - 1: 20 4 6 11 6 6 6 6.
    Lags (2, 3, 5): (1 - S^2) x = 10 12 5 7 9 11 13 15; (1 - S^3): 10 12 5 -3 -3 6 6 6; (1 - S^5): d = 10 12 5 -3 -3 -4 -6 1,
    z = 20 24 10 5 5 7 11 2.  Against the entries both ways and against this file's numpy expectation, which every other test
    leans on."""
    raw = bytes([10, 12, 15, 19, 24, 30, 37, 45])
    by_hand = {(1, 3): [20, 4, 6, 11, 6, 6, 6, 6], (2, 3, 5): [20, 24, 10, 5, 5, 7, 11, 2]}
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes([8])
        for lags, z in by_hand.items():
            assert _z_planes(raw, 1, lags).tolist() == [z] and _x_bytes(np.array([z], np.uint8), 1, lags) == raw, lags
            el = np.full(64, FILL, np.uint8)
            el[16:24] = np.frombuffer(raw, np.uint8)
            d_el, d_pl, d_out = _to(el), _fill(64), _fill(64)
            bt.split_planes_grid_dev(st, 1, [lags], d_el, [16], [8], d_n, d_pl, [32])
            bt.merge_planes_grid_dev(st, 1, [lags], d_pl, [32], [8], d_n, d_out, [19])
            assert bt.finish(st, 1) == (0, [0])
            assert _img(d_pl) == bytes([FILL] * 32 + z + [FILL] * 24), lags
            assert _img(d_out) == bytes([FILL] * 19) + raw + bytes([FILL] * 37), lags
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. the kernels: one launch each way over all the shapes
def _blocks(shafa):
    """(n, lags, offset in elements): every lag set at every count, the sets that depend on the count at theirs, and for each
    second and third lag its chunk borders"""
    T = shafa.PLANES_TILE
    counts = (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5)
    sets = [(1, 2), (1, 3), (2, 3), (3, 5, 15), (1, 16), (1, 17), (15, 16, 17), (1, 255), (1, 256), (1, 257), (255, 256, 257),
            (1, 17, 153), (1, 64, 4096), (16, 4096, 8192), (3, 768), (1, 1 << 40), (1 << 63, TOP)]
    out = [(n, s) for s in sets for n in counts]
    for n in counts:
        out += [(n, s) for s in ((1, n - 1), (1, n), (1, n + 1), (n - 2, n - 1)) if 1 <= s[0] < s[1]]
    for s in sets:
        for lag in s[1:]:
            if lag >= 1 << 20:
                continue
            _, _, _, m, G, _ = _geom(shafa, 1 << 20, lag)
            assert m == 1
            chunk = G * lag                                                # elements of a chunk of whole rows
            out += [(n, s) for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + lag + 1, 3 * chunk + 7)]
    return [(n, s, (0, 1, 3)[b % 3]) for b, (n, s) in enumerate(out)]


@pytest.mark.parametrize("k", ELEMS)
def test_one_launch_each_way_against_numpy(shafa, k):
    blocks = _blocks(shafa)
    L = _Layout(k, blocks, 100 + k)
    nb = len(blocks)
    cap = [n + 5 for n in L.n]
    chunks = [_geom(shafa, c, g)[5] for c, s in zip(cap, L.lags) for g in s[1:] if g < c]
    assert max(chunks) > 2 and 1 in chunks and 2 in chunks
    st = _stream()
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_n = _sizes(L.n)
        d_el, d_pl = _to(L.el), _fill(L.pl.size)
        assert d_el.data_ptr() % 16 == 0 and d_pl.data_ptr() % 16 == 0
        bt.split_planes_grid_dev(st, k, L.lags, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb)
        got, want = d_pl.cpu().numpy(), L.pl
        bad = [(L.n[b], L.lags[b]) for b in range(nb)
               if any(got[o:o + L.n[b]].tobytes() != want[o:o + L.n[b]].tobytes() for o in L.poff[b * k:b * k + k])]
        assert not bad, bad[:8]
        assert got.tobytes() == want.tobytes()
        assert _img(d_el) == L.el.tobytes()
        # merge: numpy's planes of the data, then random planes
        for pl, el in ((L.pl, L.el), (L.zpl, L.zel)):
            d_pl, d_out = _to(pl), _fill(el.size)
            bt.merge_planes_grid_dev(st, k, L.lags, d_pl, L.poff, cap, d_n, d_out, L.off)
            assert bt.finish(st, nb) == (0, [0] * nb)
            got = d_out.cpu().numpy()
            bad = [(L.n[b], L.lags[b]) for b in range(nb)
                   if got[L.off[b]:L.off[b] + L.n[b] * k].tobytes() != el[L.off[b]:L.off[b] + L.n[b] * k].tobytes()]
            assert not bad, bad[:8]
            assert got.tobytes() == el.tobytes()
            assert _img(d_pl) == pl.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. one lag a block; mixed widths
@pytest.mark.parametrize("k", ELEMS)
def test_one_lag_is_the_lag_entries_and_1_0_0_the_diff_entries(shafa, k):
    T = shafa.PLANES_TILE
    ns = [0, 1, 17, 1025, 4097, T + 1, 3 * T + 5]
    lags = [1, 1, 5, 300, 4097, 64, 8193]
    nb = len(ns)
    cap = [n + 5 for n in ns]
    L = _Layout(k, [(n, (g,), (0, 1, 3)[b % 3]) for b, (n, g) in enumerate(zip(ns, lags))], 200 + k)
    L1 = _Layout(k, [(n, (1, 0, 0), (0, 1, 3)[b % 3]) for b, n in enumerate(ns)], 210 + k)
    st = _stream()
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = _sizes(ns)
        # nlags = 1 against the _lag_dev entries
        d_el, d_a, d_b = _to(L.el), _fill(L.pl.size), _fill(L.pl.size)
        bt.split_planes_grid_dev(st, k, [(g,) for g in lags], d_el, L.off, cap, d_n, d_a, L.poff)
        bt.split_planes_lag_dev(st, k, lags, d_el, L.off, cap, d_n, d_b, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_a) == _img(d_b) == L.pl.tobytes()
        d_pl, d_a, d_b = _to(L.zpl), _fill(L.el.size), _fill(L.el.size)
        bt.merge_planes_grid_dev(st, k, [(g,) for g in lags], d_pl, L.poff, cap, d_n, d_a, L.off)
        bt.merge_planes_lag_dev(st, k, lags, d_pl, L.poff, cap, d_n, d_b, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_a) == _img(d_b) == L.zel.tobytes()
        # (1, 0, 0) against the _diff_dev entries
        d_el, d_a, d_b = _to(L1.el), _fill(L1.pl.size), _fill(L1.pl.size)
        bt.split_planes_grid_dev(st, k, [(1, 0, 0)] * nb, d_el, L1.off, cap, d_n, d_a, L1.poff)
        bt.split_planes_diff_dev(st, k, d_el, L1.off, cap, d_n, d_b, L1.poff)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_a) == _img(d_b) == L1.pl.tobytes()
        d_pl, d_a, d_b = _to(L1.zpl), _fill(L1.el.size), _fill(L1.el.size)
        bt.merge_planes_grid_dev(st, k, [(1, 0, 0)] * nb, d_pl, L1.poff, cap, d_n, d_a, L1.off)
        bt.merge_planes_diff_dev(st, k, d_pl, L1.poff, cap, d_n, d_b, L1.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_a) == _img(d_b) == L1.zel.tobytes()
        # mixed widths in one launch: the binding pads (7,) to (7, 0, 0)
        mixed = [(7,), (1, 7, 49), (1,), (7, 49), (1, 7), (300,), (1, 300, 100003)]
        L2 = _Layout(k, [(n, s, (0, 1, 3)[b % 3]) for b, (n, s) in enumerate(zip(ns, mixed))], 220 + k)
        d_el, d_pl, d_out = _to(L2.el), _fill(L2.pl.size), _fill(L2.el.size)
        bt.split_planes_grid_dev(st, k, mixed, d_el, L2.off, cap, d_n, d_pl, L2.poff)
        bt.merge_planes_grid_dev(st, k, mixed, d_pl, L2.poff, cap, d_n, d_out, L2.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_pl) == L2.pl.tobytes() and _img(d_out) == L2.el.tobytes()
        d_pl, d_out = _to(L2.zpl), _fill(L2.el.size)
        bt.merge_planes_grid_dev(st, k, mixed, d_pl, L2.poff, cap, d_n, d_out, L2.off)
        assert bt.finish(st, nb) == (0, [0] * nb)
        assert _img(d_out) == L2.zel.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. many blocks in one launch
@pytest.mark.parametrize("k", ELEMS)
def test_nine_blocks_one_launch_one_past_its_capacity(shafa, k):
    """two empty blocks, one past its capacity (OUTSIDE_MODULE; its element region and planes stay FILL after all passes of the
    merge, the others right), six of mixed sizes, offsets and lags"""
    T = shafa.PLANES_TILE
    ns = [17, 0, T + 1, 15, 3 * T + 5, 4100, 0, 1024, 2 * T]
    lags = [(1, 3), (1, 2), (1, 256), (1, 1 << 40), (1, 5, 300), (2, 4100), (7, 8, 9), (64,), (3, 257, 8000)]
    L = _Layout(k, [(n, s, (0, 1, 3)[b % 3]) for b, (n, s) in enumerate(zip(ns, lags))], 30 + k)
    bad = 4
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    want = [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)]
    st = _stream()
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = _sizes(dn)
        full_pl, full_el, full_zpl = L.pl.copy(), L.el.copy(), L.zpl.copy()
        L.blank(bad)
        d_el, d_pl = _to(full_el), _fill(L.pl.size)
        bt.split_planes_grid_dev(st, k, lags, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_pl) == L.pl.tobytes()
        assert _img(d_el) == full_el.tobytes()
        d_pl, d_out = _to(full_zpl), _fill(L.el.size)
        bt.merge_planes_grid_dev(st, k, lags, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_out) == L.zel.tobytes()
        assert _img(d_pl) == full_zpl.tobytes()
        # all nine within their capacities
        d_n = _sizes(ns)
        d_pl, d_out = _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_grid_dev(st, k, lags, d_el, L.off, cap, d_n, d_pl, L.poff)
        bt.merge_planes_grid_dev(st, k, lags, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9) == (0, [0] * 9)
        assert _img(d_pl) == full_pl.tobytes() and _img(d_out) == full_el.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. a block of many chunks
@pytest.mark.parametrize("k", (1, 8))
def test_a_block_of_many_chunks_and_a_round_trip(shafa, k):
    """257 T + 3 elements at lags (1, 300, 100003): the merge of differences, a pass in place of 220 chunks (two strips of 256
    columns; its scan takes several rounds) and one of a single chunk; split -> merge back to back into another offset, then
    random planes"""
    n = 257 * shafa.PLANES_TILE + 3
    lags = (1, 300, 100003)
    L, L2 = _Layout(k, [(n, lags, 3)], 60 + k), _Layout(k, [(n, lags, 3)], 60 + k, a_out=2)
    assert L.raw == L2.raw and L.off != L2.off
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = _sizes([n])
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L2.el.size)
        bt.split_planes_grid_dev(st, k, [lags], d_el, L.off, [n + 5], d_n, d_pl, L.poff)
        bt.merge_planes_grid_dev(st, k, [lags], d_pl, L.poff, [n + 5], d_n, d_out, L2.off)
        assert bt.finish(st, 1) == (0, [0])
        assert _img(d_pl) == L.pl.tobytes()
        assert _img(d_out) == L2.el.tobytes()
        d_pl, d_out = _to(L.zpl), _fill(L.el.size)
        bt.merge_planes_grid_dev(st, k, [lags], d_pl, L.poff, [n + 5], d_n, d_out, L.off)
        assert bt.finish(st, 1) == (0, [0])
        assert _img(d_out) == L.zel.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 6. behind a busy stream
def test_behind_a_busy_stream_one_finish(shafa):
    """2^20 + 3 elements of 2 bytes at lags (1, 64, 4096) and 2^19 + 1 of 8 at (3, 4097), split and merged back behind a large torch
    kernel on the same stream; the sizes come from a kernel on that stream too.  Nothing is synchronised in between: one finish."""
    import torch
    dev = _dev()
    cases = [(2, (1 << 20) + 3, (1, 64, 4096), 3), (8, (1 << 19) + 1, (3, 4097), 1)]
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
                bt.split_planes_grid_dev(st, k, [g], d_el[i], Ls[i].off, [n], d_n[i:i + 1], d_pl[i], Ls[i].poff)
            for i, (k, n, g, a) in enumerate(cases):
                bt.merge_planes_grid_dev(st, k, [g], d_pl[i], Ls[i].poff, [n], d_n[i:i + 1], d_out[i], Ls[i].off)
            assert bt.finish(st, 1) == (0, [0])
        for i, L in enumerate(Ls):
            assert _img(d_pl[i]) == L.pl.tobytes(), cases[i]
            assert _img(d_out[i]) == L.el.tobytes(), cases[i]
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. compress_grids -> decompress_grids
SHAPES = ((1000,), (37, 41), (5, 7, 11), (3, 1, 9), (2, 3, 4, 5), (), (0, 4))
DEFAULT = ((1,), (1, 41), (1, 11, 77), (1, 9), (1, 5, 20), (1,), (1,))
EXPLICIT = (((0,), (1,)), ((0,), (41,)), ((2, 0), (1, 77)), ((-1, -3), (1, 9)), ((0, 1, 3), (1, 20, 60)), ((0,), (1,)),
            ((1, 0), (1,)))
DTYPES = ("bfloat16", "float16", "float32", "float64", "int8", "int16", "int32", "int64")


def _check_item(shafa, t, ct, raw, lags):
    """the item's type and fields, and every plane — a coded one decoded alone — against numpy's plane of z"""
    import torch
    k, n = t.element_size(), t.numel()
    assert type(ct) is shafa.CompressedGrid and ct.lags == lags
    assert ct.dtype == t.dtype and tuple(ct.shape) == tuple(t.shape) and len(ct.planes) == k
    want = _z_planes(raw, k, lags)
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
def test_round_trip_is_bit_exact(shafa, dtype):
    """random bit patterns (every NaN payload, both zeros, the denormals) as slices at odd element offsets"""
    made = [_tensor(dtype, shape, 11 * i + len(dtype), lead=(1, 3, 5)[i % 3]) for i, shape in enumerate(SHAPES)]
    ts = [m[0] for m in made]
    keep = [t.clone() for t in ts]
    for axes, lags in ((None, DEFAULT), ([e[0] for e in EXPLICIT], [e[1] for e in EXPLICIT])):
        cts = shafa.compress_grids(ts, axes=axes)
        assert len(cts) == len(ts)
        for t, ct, (_, raw), g in zip(ts, cts, made, lags):
            _check_item(shafa, t, ct, raw, g)
        for b, k, t in zip(shafa.decompress_grids(cts), keep, ts):
            assert _same(b, k) and _same(t, k), (dtype, tuple(t.shape))
    # one tuple of axes for all, one item alone, explicit lags on a flat buffer, and the single-tensor calls
    cts = shafa.compress_grids(ts[1:3], axes=(0, -1))
    assert [c.lags for c in cts] == [(1, 41), (1, 77)]
    assert _same(shafa.decompress_grids(cts[0])[0], keep[1])
    flat = ts[2].reshape(-1)
    ct = shafa.compress_grids(flat, lags=(2, 15, 100))[0]
    _check_item(shafa, flat, ct, made[2][1], (2, 15, 100))
    assert _same(shafa.decompress_grids([ct])[0], keep[2].reshape(-1))
    planes = shafa.split_grid(ts[1], (3, 41))
    assert planes.cpu().numpy().tobytes() == _z_planes(made[1][1], ts[1].element_size(), (3, 41)).tobytes()
    assert _same(shafa.merge_grid(planes, ts[1].dtype, ts[1].shape, (3, 41)), keep[1])


# ---------------------------------------------------------------- 8. many tensors in one call
def _same_planes(a, b):
    assert a.nbytes == b.nbytes and len(a.planes) == len(b.planes)
    for p, q in zip(a.planes, b.planes):
        assert type(p) is type(q)
        if isinstance(p, dict):
            assert sorted(p) == sorted(q) and all(_img(p[f]) == _img(q[f]) for f in p)
        else:
            assert _img(p) == _img(q)


def test_eleven_tensors_of_mixed_rank_in_one_call(shafa):
    spec = [("float32", (50, 100)), ("float16", (0,)), ("int64", (4096,)), ("bfloat16", (16, 64, 64)), ("int32", ()),
            ("uint8", (4099, 1)), ("int16", (10, 100)), ("float64", (3, 1000)), ("int64", (2, 32, 32)), ("int16", (2049,)),
            ("int32", (3, 7, 11, 15))]
    lags = [(1, 100), (1,), (1,), (1, 64, 4096), (1,), (1,), (1, 100), (1, 1000), (1, 32, 1024), (1,), (1, 15, 165)]
    made = [_tensor(d, s, 300 + i, lead=i % 4) for i, (d, s) in enumerate(spec)]
    ts = [m[0] for m in made]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_grids(ts, block_size=65536)
    assert [c.lags for c in cts] == lags
    for t, ct, (_, raw), g in zip(ts, cts, made, lags):
        _check_item(shafa, t, ct, raw, g)
    for i, (b, k) in enumerate(zip(shafa.decompress_grids(cts), keep)):
        assert _same(b, k), spec[i]
    order = [10, 3, 2, 3, 0]                                               # another order, one item twice
    for i, b in zip(order, shafa.decompress_grids([cts[i] for i in order])):
        assert _same(b, keep[i]), spec[i]
    # one axis: the last is compress_sequences' transform, the first compress_strided's
    for t in (ts[0], ts[3], ts[9]):
        _same_planes(shafa.compress_grids(t, axes=(-1,))[0], shafa.compress_sequences(t)[0])
        _same_planes(shafa.compress_grids(t, axes=(0,))[0], shafa.compress_strided(t, axis=0)[0])


# ---------------------------------------------------------------- 9. what the grid is worth
def test_it_pays(shafa):
    """int32 [32, 64, 64], f[z, y, x] = 3 x^2 + 5 x y + 7 y z + 11 z^2 + 13 x z + ((i * 2654435761) >> 13 & 7), i the flat index:
    the entropy model puts all axes at 3.2 bits an element against 9.2 for the best single axis and 15.7 plain; only
    < is asserted"""
    import torch
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.int64)
    i = (z * 64 + y) * 64 + x
    f = (3 * x * x + 5 * x * y + 7 * y * z + 11 * z * z + 13 * x * z + ((i * 2654435761) >> 13 & 7)).astype(np.int32)
    t = torch.from_numpy(f).to(_dev())
    grid = shafa.compress_grids(t)[0]
    assert grid.lags == (1, 64, 4096)
    plain = shafa.compress_tensors(t)[0].nbytes
    single = [shafa.compress_strided(t, axis=a)[0].nbytes for a in (0, 1, 2)]
    print(f"it pays: raw {f.nbytes}, plain planes {plain}, one axis (0, 1, 2) {single}, all axes {grid.nbytes}")
    assert all(grid.nbytes < s for s in single) and grid.nbytes < plain
    assert _same(shafa.decompress_grids(grid)[0], t)


# ---------------------------------------------------------------- 10. errors
def test_corruption_is_reported_and_the_next_call_succeeds(shafa):
    import torch
    rng = np.random.default_rng(5)
    walk = np.cumsum(np.cumsum(rng.integers(-30, 31, (512, 128)), axis=0), axis=1).astype(np.int32)
    t = torch.from_numpy(walk).to(_dev())
    ct = shafa.compress_grids(t)[0]
    CG = shafa.CompressedGrid
    coded = [j for j, p in enumerate(ct.planes) if isinstance(p, dict)]
    assert coded and ct.lags == (1, 128)
    j = coded[0]
    # a truncated .shaf
    entry = dict(ct.planes[j])
    key = ".rle.shaf" if ".rle.shaf" in entry else ".shaf"
    entry[key] = entry[key][:-1]
    planes = list(ct.planes)
    planes[j] = entry
    with pytest.raises(shafa.ShafaError):
        shafa.decompress_grids(CG(ct.dtype, ct.shape, ct.lags, planes, ct.nbytes - 1))
    assert _same(shafa.decompress_grids(ct)[0], t)
    # a plane of another length
    planes[j] = torch.zeros(t.numel() - 16, dtype=torch.uint8, device=_dev())
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_grids(CG(ct.dtype, ct.shape, ct.lags, planes, 0))
    assert e.value.code == shafa.FILE_UNRECOGNIZABLE
    assert _same(shafa.decompress_grids(ct)[0], t)

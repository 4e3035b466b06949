"""shafa_hipd_split_planes_diff_dev / shafa_hipd_merge_planes_diff_dev (csrc/planes.hip) and the sequence drivers on top against
numpy on the host.  With x the block's elements as unsigned little-endian integers of k bytes, the planes are those of
z = fold(x[i] - x[i-1]), x[-1] = 0 (include/shafa_hip.h: "Byte planes of differences"), here np.diff on the raw bytes; merge's
expectation is np.cumsum of the unfolded z.  Nothing is compared with device code.

The shapes are the borders of the kernels: a lane has 16 elements, a wave 1024, a pass of the workgroup 4096, a tile
T = PLANES_TILE, and merge's scan kernel takes a block's tiles 256 at a time.  The data is uniformly random bit patterns whose
first element is M / 2 or more: every difference wraps, and one wrong carry spoils everything behind it.  Every buffer holds 0xA5
where no data lies, every region has 16 guard bytes or more around it, and every comparison is of whole images.  The full
range of alignments, 0 .. 15 against every end of the region mod 16, is test_gpu_every_alignment.py's."""
import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
ALIGN = (0, 1, 3, 8, 15)
FILL = 0xA5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _counts(shafa):
    T = shafa.PLANES_TILE
    return (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, T - 1, T, T + 1, 3 * T + 5)


def _al16(x):
    return (x + 15) // 16 * 16


def _z_planes(raw, k):
    """split's expectation: [k, n] bytes, row j byte j of the folded differences"""
    U = UINT[k]
    x = np.frombuffer(raw, U)
    one, top = U(1), U(8 * k - 1)
    d = np.diff(x, prepend=U(0))                                           # wraps mod M
    z = (d << one) ^ (U(0) - (d >> top))
    return z.view(np.uint8).reshape(-1, k).T


def _x_bytes(planes, k):
    """merge's expectation from the planes [k, n]"""
    U = UINT[k]
    one = U(1)
    z = np.ascontiguousarray(planes.T).view(U).reshape(-1)
    return np.cumsum((z >> one) ^ (U(0) - (z & one)), dtype=U).tobytes()


def _data(kind, n, k, rng):
    """n elements of k bytes as raw bytes; every kind begins with an element of M / 2 or more (a prefix carried across a block
    border, or a first element taken for a difference, shows)"""
    U = UINT[k]
    M1 = int(np.iinfo(U).max)
    if kind == "random":
        x = np.frombuffer(rng.integers(0, 256, n * k, dtype=np.uint8).tobytes(), U).copy()
        if n:
            x[0] |= U(M1 // 2 + 1)
    elif kind == "alternate":                                              # M - 1, 0, M - 1, ... and 0, M - 1, 0, ... behind it
        x = np.where(np.arange(n) % 2 == 0, U(M1), U(0)).astype(U)
    elif kind == "alternate0":                                             # the issue's 0, M - 1, 0, ...
        x = np.where(np.arange(n) % 2 == 1, U(M1), U(0)).astype(U)
    elif kind == "constant":
        x = np.full(n, U(M1 - 2), U)
    else:                                                                  # sorted, from M / 2 on
        x = np.sort(rng.integers(M1 // 2 + 1, M1, n, dtype=np.uint64, endpoint=True).astype(U))
    return x.tobytes()


class _Layout:
    """blocks (n elements of `kind`, element side at alignment a) of k-byte elements in two host images: `el` the element side
    and `pl` numpy's planes of the folded differences, both FILL where no data lies; 16 guard bytes or more around every
    region.  raw: the blocks' bytes, where the caller brings data of its own instead of a kind's."""

    def __init__(self, k, blocks, seed, a_out=None, raw=None):
        rng = np.random.default_rng(seed)
        self.k, self.n = k, [b[0] for b in blocks]
        self.off, self.poff = [], []
        pos, ppos = 0, 16
        for n, a, *_ in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + (a if a_out is None else a_out)
            self.off.append(pos)
            pos += n * k
            for _ in range(k):
                self.poff.append(ppos)
                ppos += _al16(n) + 32
        self.raw = [_data(b[2] if len(b) > 2 else "random", b[0], k, rng) for b in blocks] if raw is None else list(raw)
        assert [len(r) for r in self.raw] == [n * k for n in self.n]
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.pl = np.full(ppos + 16, FILL, np.uint8)
        for b, n in enumerate(self.n):
            self.el[self.off[b]:self.off[b] + n * k] = np.frombuffer(self.raw[b], np.uint8)
            planes = _z_planes(self.raw[b], k)
            assert _x_bytes(planes, k) == self.raw[b]                      # numpy's inverse of numpy's transform
            for j in range(k):
                self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = planes[j]

    def blank(self, b):
        """block b leaves no trace in either image"""
        n, k = self.n[b], self.k
        self.el[self.off[b]:self.off[b] + n * k] = FILL
        for j in range(k):
            self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = FILL


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(_dev())


def _fill(n):
    import torch
    return torch.full((n,), FILL, dtype=torch.uint8, device=_dev())


def _img(t):
    return t.cpu().numpy().tobytes()


def test_numpy_side():
    """the expectation itself, on values worked out by hand (k = 1, M = 256)"""
    raw = bytes([200, 201, 199, 199, 0, 255])
    # d = 200, 1, 254 (-2), 0, 57, 255 (-1);  z = (d << 1) ^ (255 if d >= 128): 144 ^ 255, 2, 252 ^ 255, 0, 114, 254 ^ 255
    assert _z_planes(raw, 1).tolist() == [[111, 2, 3, 0, 114, 1]]
    assert _x_bytes(_z_planes(raw, 1), 1) == raw
    assert _z_planes(np.array([0x8000, 0x7FFF], np.uint16).tobytes(), 2).tolist() == [[0xFF, 0x01], [0xFF, 0x00]]


# ---------------------------------------------------------------- 1. the kernels, block by block
@pytest.mark.parametrize("a", ALIGN)
@pytest.mark.parametrize("k", ELEMS)
def test_split_against_numpy(shafa, k, a):
    import torch
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, n in enumerate(_counts(shafa)):
            L = _Layout(k, [(n, a)], 1000 * k + 100 * a + i)
            d_el, d_pl = _to(L.el), _fill(L.pl.size)
            assert (d_el.data_ptr() + L.off[0]) % 16 == a and d_pl.data_ptr() % 16 == 0
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            bt.split_planes_diff_dev(st, k, d_el, L.off, [n + 5], d_n, d_pl, L.poff)
            assert bt.finish(st, 1) == (0, [0]), (k, a, n)
            assert _img(d_pl) == L.pl.tobytes(), (k, a, n)
            assert _img(d_el) == L.el.tobytes(), (k, a, n)
    finally:
        bt.close()


@pytest.mark.parametrize("a", ALIGN)
@pytest.mark.parametrize("k", ELEMS)
def test_merge_against_numpy_and_round_trip(shafa, k, a):
    import torch
    a2 = ALIGN[(ALIGN.index(a) + 2) % len(ALIGN)]                          # another alignment
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, n in enumerate(_counts(shafa)):
            seed = 2000 * k + 100 * a + i
            L = _Layout(k, [(n, a)], seed)
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            # the planes numpy made -> the elements
            d_pl, d_out = _to(L.pl), _fill(L.el.size)
            assert (d_out.data_ptr() + L.off[0]) % 16 == a
            bt.merge_planes_diff_dev(st, k, d_pl, L.poff, [n + 5], d_n, d_out, L.off)
            assert bt.finish(st, 1) == (0, [0]), (k, a, n)
            assert _img(d_out) == L.el.tobytes(), (k, a, n)
            assert _img(d_pl) == L.pl.tobytes(), (k, a, n)
            # split -> merge back to back on the stream, into another alignment
            L2 = _Layout(k, [(n, a)], seed, a_out=a2)                      # the same bytes
            assert L2.raw == L.raw
            d_el, d_mid, d_back = _to(L.el), _fill(L.pl.size), _fill(L2.el.size)
            assert (d_back.data_ptr() + L2.off[0]) % 16 == a2
            bt.split_planes_diff_dev(st, k, d_el, L.off, [n + 5], d_n, d_mid, L.poff)
            bt.merge_planes_diff_dev(st, k, d_mid, L.poff, [n + 5], d_n, d_back, L2.off)
            assert bt.finish(st, 1) == (0, [0]), (k, a, n)
            assert _img(d_back) == L2.el.tobytes(), (k, a, n)
            assert _img(d_mid) == L.pl.tobytes(), (k, a, n)
    finally:
        bt.close()


@pytest.mark.parametrize("kind", ("alternate0", "alternate", "constant", "sorted"))
@pytest.mark.parametrize("k", ELEMS)
def test_patterns(shafa, k, kind):
    """0, M - 1, 0, ... (every difference is + 1 or - 1 mod M, the two smallest non-zero z), a constant (z = 0 behind the first
    element) and a sorted array, across the unit, wave, pass and tile borders"""
    import torch
    T = shafa.PLANES_TILE
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, (n, a) in enumerate(((17, 3), (1025, 0), (4097, 8), (T + 1, 0), (3 * T + 5, 15))):
            L = _Layout(k, [(n, a, kind)], 3000 * k + i)
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
            bt.split_planes_diff_dev(st, k, d_el, L.off, [n + 5], d_n, d_pl, L.poff)
            bt.merge_planes_diff_dev(st, k, d_pl, L.poff, [n + 5], d_n, d_out, L.off)
            assert bt.finish(st, 1) == (0, [0]), (k, kind, n)
            assert _img(d_pl) == L.pl.tobytes(), (k, kind, n)
            assert _img(d_out) == L.el.tobytes(), (k, kind, n)
            # and from numpy's planes alone
            d_pl, d_out = _to(L.pl), _fill(L.el.size)
            bt.merge_planes_diff_dev(st, k, d_pl, L.poff, [n + 5], d_n, d_out, L.off)
            assert bt.finish(st, 1) == (0, [0]), (k, kind, n)
            assert _img(d_out) == L.el.tobytes(), (k, kind, n)
    finally:
        bt.close()


@pytest.mark.parametrize("k", (1, 8))
def test_a_block_longer_than_one_round_of_the_scan(shafa, k):
    """257 T + 3 elements: 258 tiles, so the scan kernel carries a total from its first 256 sums into the next round"""
    import torch
    n = 257 * shafa.PLANES_TILE + 3
    L = _Layout(k, [(n, 3)], 60 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_diff_dev(st, k, d_el, L.off, [n + 5], d_n, d_pl, L.poff)
        assert bt.finish(st, 1) == (0, [0])
        assert _img(d_pl) == L.pl.tobytes()
        d_pl = _to(L.pl)
        bt.merge_planes_diff_dev(st, k, d_pl, L.poff, [n + 5], d_n, d_out, L.off)
        assert bt.finish(st, 1) == (0, [0])
        assert _img(d_out) == L.el.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. many blocks in one launch
@pytest.mark.parametrize("k", ELEMS)
def test_nine_blocks_one_launch_one_past_its_capacity(shafa, k):
    """two empty blocks, one past its capacity (OUTSIDE_MODULE, no byte of it touched, the others right), six of mixed sizes
    and alignments; every block's data begins with a large element, so a prefix carried across a block border shows"""
    import torch
    T = shafa.PLANES_TILE
    ns = [17, 0, T + 1, 15, 3 * T + 5, 4100, 0, 1024, 2 * T]
    al = [3, 0, 0, 15, 1, 0, 8, 1, 4]
    L = _Layout(k, list(zip(ns, al)), 30 + k)
    bad = 4
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    want = [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)]
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = torch.tensor(dn, dtype=torch.int64, device=_dev())
        full_pl, full_el = L.pl.copy(), L.el.copy()
        L.blank(bad)
        d_el, d_pl = _to(full_el), _fill(L.pl.size)
        bt.split_planes_diff_dev(st, k, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_pl) == L.pl.tobytes()
        assert _img(d_el) == full_el.tobytes()
        d_pl, d_out = _to(full_pl), _fill(L.el.size)
        bt.merge_planes_diff_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_out) == L.el.tobytes()
        assert _img(d_pl) == full_pl.tobytes()
        # all nine within their capacities
        d_n = torch.tensor(ns, dtype=torch.int64, device=_dev())
        d_pl, d_out = _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_diff_dev(st, k, d_el, L.off, cap, d_n, d_pl, L.poff)
        bt.merge_planes_diff_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9) == (0, [0] * 9)
        assert _img(d_pl) == full_pl.tobytes() and _img(d_out) == full_el.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("k", (1, 4))
def test_runs_of_tiles_per_workgroup(shafa, k):
    """32775 tiles in the capacities with small sizes: three tiles a workgroup, runs that start in one block and end in the
    next, most tiles behind their block's real size (and their sums never written nor read)"""
    import torch
    T = shafa.PLANES_TILE
    ns = [3 * T + 5, T + 1, 20000]
    cap = [3 * T + 5, 1 << 28, 20000]
    L = _Layout(k, list(zip(ns, (1, 3, 0))), 50 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = torch.tensor(ns, dtype=torch.int64, device=_dev())
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_diff_dev(st, k, d_el, L.off, cap, d_n, d_pl, L.poff)
        bt.merge_planes_diff_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 3) == (0, [0, 0, 0])
        assert _img(d_pl) == L.pl.tobytes()
        assert _img(d_out) == L.el.tobytes()
    finally:
        bt.close()


def test_behind_a_busy_stream_one_finish(shafa):
    """2^20 + 3 elements of 2 bytes and 2^19 + 1 of 8, split and merged back behind a large torch kernel on the same stream;
    the sizes come from a kernel on that stream too.  Nothing is synchronised in between: one finish."""
    import torch
    dev = _dev()
    cases = [(2, (1 << 20) + 3, 3), (8, (1 << 19) + 1, 15)]
    Ls = [_Layout(k, [(n, a)], 77 + k) for k, n, a in cases]
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
            for i, (k, n, a) in enumerate(cases):
                bt.split_planes_diff_dev(st, k, d_el[i], Ls[i].off, [n], d_n[i:i + 1], d_pl[i], Ls[i].poff)
            for i, (k, n, a) in enumerate(cases):
                bt.merge_planes_diff_dev(st, k, d_pl[i], Ls[i].poff, [n], d_n[i:i + 1], d_out[i], Ls[i].off)
            assert bt.finish(st, 1) == (0, [0])
        for i, L in enumerate(Ls):
            assert _img(d_pl[i]) == L.pl.tobytes(), cases[i]
            assert _img(d_out[i]) == L.el.tobytes(), cases[i]
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. compress_sequences -> decompress_sequences
NUMELS = (0, 1, 17, 1000, 4096, 1 << 16)
DTYPES = ("int64", "int32", "int16", "uint8", "bfloat16", "float16", "float32", "float64")


def _bits(t):
    return t.reshape(-1).view(__import__("torch").uint8)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(_bits(a), _bits(b))


def _tensor(dtype, n, seed, lead=0, kind="walk"):
    """n elements of `dtype`, a slice `lead` elements into its storage, and its raw bytes.  walk: a large first element, then
    steps in +-300 (mod M): the high planes of the differences code, the low ones mostly do not; random: random bit patterns —
    every NaN payload, both zeros and the denormals at the float dtypes"""
    import torch
    dt = getattr(torch, dtype)
    k = torch.empty((), dtype=dt).element_size()
    U = UINT[k]
    rng = np.random.default_rng(seed)
    if kind == "walk":
        steps = rng.integers(-300, 301, n).astype(np.int64).astype(np.uint64)
        if n:
            steps[0] = np.uint64((int(np.iinfo(U).max) - 1000) % (1 << 64))
        raw = np.cumsum(steps, dtype=np.uint64).astype(U).tobytes()
    else:
        raw = _data("random", n, k, rng)
    whole = torch.empty((lead + n + 3) * k, dtype=torch.uint8, device=_dev()).view(dt)
    t = whole[lead:lead + n]
    _bits(t).copy_(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()))
    assert t.is_contiguous() and t.storage_offset() == lead
    return t, raw


def _check_item(shafa, t, ct, raw):
    """the item's type and fields, and every plane — a coded one decoded alone — against numpy's plane of z"""
    import torch
    k, n = t.element_size(), t.numel()
    assert type(ct) is shafa.CompressedSequence
    assert ct.dtype == t.dtype and tuple(ct.shape) == tuple(t.shape) and len(ct.planes) == k
    want = _z_planes(raw, k)
    total = 0
    for j, p in enumerate(ct.planes):
        if isinstance(p, dict):
            assert n >= 1024 and sum(int(f.numel()) for f in p.values()) < n
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
    kinds = ("walk", "random", "walk", "random", "walk", "walk")
    made = [_tensor(dtype, n, 7 * i + len(dtype), lead=(0, 3, 1, 0, 5, 1)[i], kind=kinds[i]) for i, n in enumerate(NUMELS)]
    made.append(_tensor(dtype, 1 << 16, 99, lead=3, kind="random"))
    ts = [m[0] for m in made]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_sequences(ts)
    assert len(cts) == len(ts)
    for t, ct, (_, raw) in zip(ts, cts, made):
        _check_item(shafa, t, ct, raw)
    if dtype != "uint8":
        assert any(isinstance(p, dict) for p in cts[5].planes)             # the walk's high planes are file sets
    back = shafa.decompress_sequences(cts)
    assert len(back) == len(ts)
    for b, k, t in zip(back, keep, ts):
        assert _same(b, k) and _same(t, k), (dtype, t.numel())
    # one item alone, and a shape
    one = shafa.compress_sequences(ts[3].view(8, 125))
    assert len(one) == 1 and one[0].shape == (8, 125)
    assert _same(shafa.decompress_sequences(one[0])[0], keep[3].view(8, 125))


def test_eleven_tensors_in_one_call(shafa):
    spec = [("float32", 5000), ("float16", 0), ("int64", 4096), ("bfloat16", 65536), ("int32", 1), ("uint8", 4099),
            ("int16", 1000), ("float64", 3000), ("int64", 1024), ("int16", 2049), ("int32", 1155)]
    made = [_tensor(d, n, 300 + i, lead=i % 4, kind=("walk", "random")[i % 3 == 0]) for i, (d, n) in enumerate(spec)]
    ts = [m[0] for m in made]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_sequences(ts, block_size=65536)
    assert len(cts) == 11
    for t, ct, (_, raw) in zip(ts, cts, made):
        _check_item(shafa, t, ct, raw)
    back = shafa.decompress_sequences(cts)
    for i, (b, k) in enumerate(zip(back, keep)):
        assert _same(b, k), spec[i]
    order = [10, 3, 2, 3, 0]                                               # another order, one item twice
    for i, b in zip(order, shafa.decompress_sequences([cts[i] for i in order])):
        assert _same(b, keep[i]), spec[i]
    # the other decoders refuse the items, and this one theirs
    with pytest.raises(ValueError, match="decompress_sequences"):
        shafa.decompress_tensors(cts)
    with pytest.raises(ValueError, match="decompress_sequences"):
        shafa.decompress_deltas(cts, [None] * 11)
    with pytest.raises(ValueError, match="decompress_sequences: a CompressedSequence"):
        shafa.decompress_sequences(shafa.compress_tensors(ts[0]))


# ---------------------------------------------------------------- 4. what the differences are worth
def test_it_pays(shafa):
    """The two relations the entropy model of the planes gives (order-0 entropy of each plane plus 600 bytes of overhead a
    plane, RLE ignored, 2^18 elements): sorted uniform uint64 below 2^40 — 772 337 bytes for the planes of the differences
    against 1 312 520 for the plain planes, a ratio of 0.59; arange as int32 — four planes that are constant behind their first
    byte against 591 024 bytes, more than 30 x.  The factor 10 below is a third of the model's."""
    import torch
    n = 1 << 18
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64).sort().values.to(_dev())
    seq, plain = shafa.compress_sequences(ids)[0], shafa.compress_tensors(ids)[0]
    print(f"it pays: sorted int64 below 2^40: differences {seq.nbytes} bytes, plain planes {plain.nbytes} bytes, raw {8 * n}")
    assert seq.nbytes < plain.nbytes
    assert _same(shafa.decompress_sequences(seq)[0], ids)
    pos = torch.arange(n, dtype=torch.int32, device=_dev())
    seq, plain = shafa.compress_sequences(pos)[0], shafa.compress_tensors(pos)[0]
    print(f"it pays: arange int32: differences {seq.nbytes} bytes, plain planes {plain.nbytes} bytes, raw {4 * n}")
    assert 10 * seq.nbytes < plain.nbytes
    assert _same(shafa.decompress_sequences(seq)[0], pos)


# ---------------------------------------------------------------- 5. errors
def test_corruption_is_reported_and_the_next_call_succeeds(shafa):
    t, raw = _tensor("int32", 1 << 16, 5, lead=1)
    ct = shafa.compress_sequences(t)[0]
    CS = shafa.CompressedSequence
    coded = [j for j, p in enumerate(ct.planes) if isinstance(p, dict)]
    assert coded
    j = coded[0]
    # a truncated .shaf
    entry = dict(ct.planes[j])
    key = ".rle.shaf" if ".rle.shaf" in entry else ".shaf"
    entry[key] = entry[key][:-1]
    planes = list(ct.planes)
    planes[j] = entry
    with pytest.raises(shafa.ShafaError):
        shafa.decompress_sequences(CS(ct.dtype, ct.shape, planes, ct.nbytes - 1))
    assert _same(shafa.decompress_sequences(ct)[0], t)
    # a plane of another length
    import torch
    planes[j] = torch.zeros(t.numel() - 16, dtype=torch.uint8, device=_dev())
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_sequences(CS(ct.dtype, ct.shape, planes, 0))
    assert e.value.code == shafa.FILE_UNRECOGNIZABLE
    assert _same(shafa.decompress_sequences(ct)[0], t)
    # a plane entry that is an error
    planes[j] = shafa.ShafaError(shafa.FILE_TOO_SMALL, "planted")
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_sequences(CS(ct.dtype, ct.shape, planes, 0))
    assert e.value.code == shafa.FILE_TOO_SMALL
    assert _same(shafa.decompress_sequences(ct)[0], t)

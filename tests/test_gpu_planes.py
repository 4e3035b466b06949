"""shafa_hipd_split_planes_dev / shafa_hipd_merge_planes_dev (csrc/planes.hip) and the tensor drivers on top against numpy on
the host: the planes of n elements of k bytes are np.frombuffer(raw, np.uint8).reshape(n, k).T, nothing is compared with device
code.

The shapes are the smallest at which the kernels can go wrong: a lane transposes 16 elements, a tile is T = PLANES_TILE
elements, the element side lies at the byte alignments 0, 1, 3, 8, 15.  Every buffer is 0xA5 where no data lies and is compared
whole, so a byte written in front of a region, behind a plane's d_n bytes or into a guard shows up.  The tiles are numbered
from the capacities: a capacity of 2^28 elements with few real ones gives every workgroup a run of several tiles without the
memory.  The full range of alignments, 0 .. 15 against every end of the region mod 16, is test_gpu_every_alignment.py's.

A compressed plane is compress_many's dict with the files' names as keys; shafa.plane_files(entry) names the two of them that
decompress_files takes (the issue's `decompress_files(**entry)` with the keyword names filled in)."""
import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
ALIGN = (0, 1, 3, 8, 15)
FILL = 0xA5


def _counts(shafa):
    T = shafa.PLANES_TILE
    return (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5)


def _al16(x):
    return (x + 15) // 16 * 16


def _planes_of(raw, n, k):
    return np.frombuffer(raw, np.uint8).reshape(n, k).T


class _Layout:
    """blocks (n elements each, element side at alignment a) of k-byte elements in two host images: `el` the element side,
    `pl` the plane side, both FILL where no data lies; every region has 16 guard bytes or more on both sides"""

    def __init__(self, k, blocks, seed):
        rng = np.random.default_rng(seed)
        self.k, self.n = k, [n for n, _ in blocks]
        self.off, self.poff, pos, ppos = [], [], 0, 16
        for n, a in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + a
            self.off.append(pos)
            pos += n * k
            for _ in range(k):
                self.poff.append(ppos)
                ppos += _al16(n) + 32
        self.raw = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in self.n]
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.pl = np.full(ppos + 16, FILL, np.uint8)
        for b, raw in enumerate(self.raw):
            self.put(b, raw)

    def put(self, b, raw):
        n, k = self.n[b], self.k
        self.el[self.off[b]:self.off[b] + n * k] = np.frombuffer(raw, np.uint8)
        for j in range(k):
            self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = _planes_of(raw, n, k)[j]

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


# ---------------------------------------------------------------- 1. the two kernels, block by block
@pytest.mark.parametrize("a", ALIGN)
@pytest.mark.parametrize("k", ELEMS)
def test_split_against_numpy(shafa, k, a):
    import torch
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, n in enumerate(_counts(shafa)):
            L = _Layout(k, [(n, a)], 1000 * k + 10 * a + i)
            d_el, d_pl = _to(L.el), _fill(L.pl.size)
            assert (d_el.data_ptr() + L.off[0]) % 16 == a
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            bt.split_planes_dev(st, k, d_el, L.off, [n + 5], d_n, d_pl, L.poff)
            assert bt.finish(st, 1) == (0, [0]), (k, a, n)
            assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes(), (k, a, n)
            assert d_el.cpu().numpy().tobytes() == L.el.tobytes(), (k, a, n)
    finally:
        bt.close()


@pytest.mark.parametrize("a", ALIGN)
@pytest.mark.parametrize("k", ELEMS)
def test_merge_against_numpy_and_round_trip(shafa, k, a):
    import torch
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, n in enumerate(_counts(shafa)):
            L = _Layout(k, [(n, a)], 2000 * k + 10 * a + i)
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            # the planes numpy made -> the elements
            d_pl, d_out = _to(L.pl), _fill(L.el.size)
            bt.merge_planes_dev(st, k, d_pl, L.poff, [n + 5], d_n, d_out, L.off)
            assert bt.finish(st, 1) == (0, [0]), (k, a, n)
            assert d_out.cpu().numpy().tobytes() == L.el.tobytes(), (k, a, n)
            assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes(), (k, a, n)
            # split -> merge, back to back on the stream, into another alignment
            a2 = ALIGN[(ALIGN.index(a) + 2) % len(ALIGN)]
            L2 = _Layout(k, [(n, a2)], 2000 * k + 10 * a + i)             # the same bytes
            assert L2.raw == L.raw
            d_el, d_mid, d_back = _to(L.el), _fill(L.pl.size), _fill(L2.el.size)
            bt.split_planes_dev(st, k, d_el, L.off, [n], d_n, d_mid, L.poff)
            bt.merge_planes_dev(st, k, d_mid, L.poff, [n], d_n, d_back, L2.off)
            assert bt.finish(st, 1) == (0, [0]), (k, a, n)
            assert d_back.cpu().numpy().tobytes() == L2.el.tobytes(), (k, a, n)
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. many blocks in one launch
@pytest.mark.parametrize("k", ELEMS)
def test_nine_blocks_one_launch_one_past_its_capacity(shafa, k):
    import torch
    T = shafa.PLANES_TILE
    ns = [17, 0, T + 1, 15, 3 * T + 5, 0, T - 1, 16, T]
    L = _Layout(k, [(n, ALIGN[b % len(ALIGN)]) for b, n in enumerate(ns)], 30 + k)
    bad = 4
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = torch.tensor(dn, dtype=torch.int64, device=_dev())
        want = [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)]
        # split: the bad block's planes stay as they were
        d_el, d_pl = _to(L.el), _fill(L.pl.size)
        bt.split_planes_dev(st, k, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        full_pl, full_el = L.pl.copy(), L.el.copy()
        L.blank(bad)
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes()
        assert d_el.cpu().numpy().tobytes() == full_el.tobytes()
        # merge: the bad block's region stays as it was
        d_pl, d_out = _to(full_pl), _fill(L.el.size)
        bt.merge_planes_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert d_out.cpu().numpy().tobytes() == L.el.tobytes()
        # a capacity of 0 has no tile: its block is still reported, alone and next to others
        d_n1 = torch.tensor([1, 16], dtype=torch.int64, device=_dev())
        d_pl = _fill(L.pl.size)
        bt.split_planes_dev(st, k, d_el, L.off[:1], [0], d_n1, d_pl, L.poff[:k])
        assert bt.finish(st, 1, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [shafa.OUTSIDE_MODULE])
        bt.split_planes_dev(st, k, d_el, [L.off[0], L.off[7]], [0, 16], d_n1, d_pl, L.poff[:k] + L.poff[7 * k:8 * k])
        assert bt.finish(st, 2, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [shafa.OUTSIDE_MODULE, 0])
        only7 = np.full(L.pl.size, FILL, np.uint8)
        for j in range(k):
            o = L.poff[7 * k + j]
            only7[o:o + 16] = full_pl[o:o + 16]
        assert d_pl.cpu().numpy().tobytes() == only7.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. large blocks, a busy stream, runs of tiles per workgroup
def test_large_blocks_behind_a_busy_stream_one_finish(shafa):
    """2^22 + 3 elements of 2 bytes and 2^20 + 1 of 8, split and merged back behind a large torch kernel on the same stream; the
    sizes come from a kernel on that stream too.  One finish."""
    import torch
    dev = _dev()
    cases = [(2, (1 << 22) + 3, 3), (8, (1 << 20) + 1, 15)]
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
            busy = torch.empty(1 << 28, dtype=torch.float32, device=dev)
            busy.normal_()                                                 # 1 GiB written: a few hundred microseconds
            d_n = half.sum(dim=1)                                          # the sizes exist only behind it
            for i, (k, n, a) in enumerate(cases):
                bt.split_planes_dev(st, k, d_el[i], Ls[i].off, [n], d_n[i:i + 1], d_pl[i], Ls[i].poff)
            for i, (k, n, a) in enumerate(cases):
                bt.merge_planes_dev(st, k, d_pl[i], Ls[i].poff, [n], d_n[i:i + 1], d_out[i], Ls[i].off)
            assert bt.finish(st, 1) == (0, [0])
        for i, L in enumerate(Ls):
            assert d_pl[i].cpu().numpy().tobytes() == L.pl.tobytes(), cases[i]
            assert d_out[i].cpu().numpy().tobytes() == L.el.tobytes(), cases[i]
    finally:
        bt.close()


@pytest.mark.parametrize("k", (1, 4))
def test_runs_of_tiles_per_workgroup(shafa, k):
    """32775 tiles in the capacities: three tiles a workgroup, runs that start in one block and end in the next, and most
    tiles behind their block's real size"""
    import torch
    T = shafa.PLANES_TILE
    ns = [3 * T + 5, T + 1, 20000]
    cap = [3 * T + 5, 1 << 28, 20000]
    L = _Layout(k, [(n, ALIGN[(b + 1) % len(ALIGN)]) for b, n in enumerate(ns)], 50 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = torch.tensor(ns, dtype=torch.int64, device=_dev())
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_dev(st, k, d_el, L.off, cap, d_n, d_pl, L.poff)
        bt.merge_planes_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 3) == (0, [0, 0, 0])
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes()
        assert d_out.cpu().numpy().tobytes() == L.el.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. split_planes / merge_planes
@pytest.mark.parametrize("dtype,n", [("float32", 1000), ("bfloat16", 4096), ("int64", 17), ("uint8", 33), ("float64", 0)])
def test_split_planes_and_merge_planes(shafa, dtype, n):
    import torch
    dt = getattr(torch, dtype)
    k = torch.empty((), dtype=dt).element_size()
    raw = np.random.default_rng(n).integers(0, 256, n * k, dtype=np.uint8)
    t = _to(raw).view(dt) if n else torch.empty(0, dtype=dt, device=_dev())
    planes = shafa.split_planes(t)
    assert planes.dtype == torch.uint8 and tuple(planes.shape) == (k, n)
    assert planes.cpu().numpy().tobytes() == _planes_of(raw.tobytes(), n, k).tobytes()
    for p in (planes, planes.contiguous(), planes.clone()[:, :n]):
        back = shafa.merge_planes(p, dt, (n,))
        assert back.dtype == dt and tuple(back.shape) == (n,)
        assert back.view(torch.uint8).cpu().numpy().tobytes() == raw.tobytes()
    if n == 4096:
        assert tuple(shafa.merge_planes(planes, dt, (4, 16, 64)).shape) == (4, 16, 64)
        with pytest.raises(ValueError):
            shafa.merge_planes(planes, dt, (4095,))
        with pytest.raises(ValueError):
            shafa.merge_planes(planes, torch.float32, (4096,))
        with pytest.raises(ValueError):
            shafa.compress_tensors(t.view(64, 64).t())
        with pytest.raises(ValueError):
            shafa.compress_tensors([t, t.cpu()])
        with pytest.raises(ValueError):
            shafa.compress_tensors(_to(np.zeros(64, np.complex128)))


# ---------------------------------------------------------------- 5. compress_tensors -> decompress_tensors
def _bits(t):
    return t.reshape(-1).view(__import__("torch").uint8)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(_bits(a), _bits(b))


def _tensor(name):
    import torch
    g = torch.Generator().manual_seed(len(name) * 131 + sum(name.encode()))
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    make = {
        "bf16-patterns": lambda: pat.view(torch.bfloat16),
        "fp16-patterns": lambda: pat.view(torch.float16),
        "fp32-randn": lambda: torch.randn(5000, generator=g),
        "fp64-randn": lambda: torch.randn(3000, generator=g, dtype=torch.float64),
        "int8": lambda: torch.randint(-128, 128, (4099,), generator=g, dtype=torch.int8),
        "int32": lambda: torch.randint(-1000, 1000, (3001,), generator=g, dtype=torch.int32),
        "int64-token-ids": lambda: torch.randint(0, 50000, (4096,), generator=g, dtype=torch.int64),
        "complex64": lambda: torch.complex(torch.randn(2000, generator=g), torch.randn(2000, generator=g)),
        "numel-1": lambda: torch.tensor(-0.0, dtype=torch.float32),
        "numel-0": lambda: torch.empty((3, 0, 2), dtype=torch.float16),
        "numel-1000": lambda: (torch.randn(1000, generator=g) * 0.02).to(torch.bfloat16),
        "numel-1023": lambda: (torch.randn(1023, generator=g) * 0.02).to(torch.bfloat16),
        "numel-1024": lambda: (torch.randn(1024, generator=g) * 0.02).to(torch.bfloat16),
        "shape-3-5-7-11": lambda: torch.randn((3, 5, 7, 11), generator=g),
    }
    return make[name]().to(_dev())


SINGLE = ("bf16-patterns", "fp16-patterns", "fp32-randn", "fp64-randn", "int8", "int32", "int64-token-ids", "complex64",
          "numel-1", "numel-0", "numel-1000", "numel-1023", "numel-1024", "shape-3-5-7-11")


def _check_item(shafa, t, ct):
    import torch
    k, n = t.element_size(), t.numel()
    assert isinstance(ct, shafa.CompressedTensor) and ct.dtype == t.dtype and tuple(ct.shape) == tuple(t.shape)
    assert len(ct.planes) == k
    total = 0
    for p in ct.planes:
        if isinstance(p, dict):
            assert n >= 1024 and sum(int(f.numel()) for f in p.values()) < n
            total += sum(int(f.numel()) for f in p.values())
        else:
            assert isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and int(p.numel()) == n
            total += n
    assert ct.nbytes == total
    if n < 1024:
        assert all(isinstance(p, torch.Tensor) for p in ct.planes)


@pytest.mark.parametrize("name", SINGLE)
def test_round_trip_is_bit_exact(shafa, name):
    import torch
    t = _tensor(name)
    keep = t.clone()
    ct = shafa.compress_tensors(t)
    assert len(ct) == 1
    _check_item(shafa, t, ct[0])
    back = shafa.decompress_tensors(ct)
    assert len(back) == 1 and _same(back[0], keep) and _same(t, keep), name
    assert _same(shafa.decompress_tensors(ct[0])[0], keep)                 # a single item, not in a list
    # the raw planes are the numpy planes
    raw = _bits(keep).cpu().numpy().tobytes()
    for j, p in enumerate(ct[0].planes):
        if isinstance(p, torch.Tensor):
            assert p.cpu().numpy().tobytes() == _planes_of(raw, t.numel(), t.element_size())[j].tobytes(), (name, j)
    if name == "int64-token-ids":                                          # six constant planes: single-symbol blocks of size 0
        assert all(isinstance(p, dict) for p in ct[0].planes[2:])
        assert ct[0].nbytes < 3 * t.numel()


def test_eleven_tensors_in_one_call(shafa):
    names = ("fp32-randn", "numel-0", "int64-token-ids", "bf16-patterns", "numel-1", "int8", "numel-1000", "complex64",
             "fp64-randn", "numel-1024", "shape-3-5-7-11")
    ts = [_tensor(n) for n in names]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_tensors(ts, block_size=65536)
    assert len(cts) == 11
    for t, ct in zip(ts, cts):
        _check_item(shafa, t, ct)
    back = shafa.decompress_tensors(cts)
    assert len(back) == 11
    for name, b, k in zip(names, back, keep):
        assert _same(b, k), name
    # the same items in another order and one of them twice
    order = [10, 3, 3, 0, 9]
    for i, b in zip(order, shafa.decompress_tensors([cts[i] for i in order])):
        assert _same(b, keep[i]), names[i]


# ---------------------------------------------------------------- 6. what a plane is, and what the split is worth
def _small_weights(n):
    import torch
    return (torch.randn(n, generator=torch.Generator().manual_seed(1)) * 0.02).to(torch.bfloat16).to(_dev())


def test_planes_are_ordinary_file_sets(shafa):
    import torch
    t = _small_weights(1 << 16)
    raw = _bits(t).cpu().numpy().tobytes()
    ct = shafa.compress_tensors(t, block_size=65536)[0]
    coded = [j for j, p in enumerate(ct.planes) if isinstance(p, dict)]
    assert coded
    for j in coded:
        plane = _planes_of(raw, t.numel(), 2)[j].tobytes()
        assert shafa.decompress_files(**shafa.plane_files(ct.planes[j])).cpu().numpy().tobytes() == plane
        alone = shafa.compress_many(_to(np.frombuffer(plane, np.uint8)), [len(plane)], block_size=65536)[0]
        assert sorted(alone) == sorted(ct.planes[j])
        for key in alone:
            assert alone[key].cpu().numpy().tobytes() == ct.planes[j][key].cpu().numpy().tobytes(), (j, key)


def test_it_pays(shafa):
    """bf16 weights of standard deviation 0.02, 2^20 of them: the mantissa plane is kept raw, the sign and exponent plane is a
    file set, and the whole is smaller than the file set of the unsplit bytes at the same block size.  Measured on an MI355X:
    1 404 471 bytes by plane against 1 644 499 unsplit, of 2 097 152."""
    import torch
    t = _small_weights(1 << 20)
    ct = shafa.compress_tensors(t)[0]
    assert isinstance(ct.planes[0], torch.Tensor) and isinstance(ct.planes[1], dict)
    unsplit = shafa.compress_many(_bits(t), [2 * t.numel()], block_size=8 << 20)[0]
    whole = sum(int(f.numel()) for f in unsplit.values())
    print(f"it pays: by plane {ct.nbytes} bytes, unsplit {whole} bytes, raw {2 * t.numel()} bytes")
    assert ct.nbytes < whole
    assert _same(shafa.decompress_tensors(ct)[0], t)


def test_corruption_is_reported(shafa):
    t = _small_weights(1 << 16)
    ct = shafa.compress_tensors(t)[0]
    j = [j for j, p in enumerate(ct.planes) if isinstance(p, dict)][0]
    entry = dict(ct.planes[j])
    key = ".rle.shaf" if ".rle.shaf" in entry else ".shaf"
    entry[key] = entry[key][:-1]
    planes = list(ct.planes)
    planes[j] = entry
    with pytest.raises(shafa.ShafaError):
        shafa.decompress_tensors(shafa.CompressedTensor(ct.dtype, ct.shape, planes, ct.nbytes - 1))
    # a plane of another length, a plane entry that is an error
    planes[j] = ct.planes[1 - j][:-16] if not isinstance(ct.planes[1 - j], dict) else ct.planes[j]
    if planes[j] is not ct.planes[j]:
        with pytest.raises(shafa.ShafaError) as e:
            shafa.decompress_tensors(shafa.CompressedTensor(ct.dtype, ct.shape, planes, 0))
        assert e.value.code == shafa.FILE_UNRECOGNIZABLE
    planes[j] = shafa.ShafaError(shafa.FILE_TOO_SMALL, "planted")
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_tensors(shafa.CompressedTensor(ct.dtype, ct.shape, planes, 0))
    assert e.value.code == shafa.FILE_TOO_SMALL
    assert _same(shafa.decompress_tensors(ct)[0], t)

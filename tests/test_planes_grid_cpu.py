"""CPU-side checks of the byte-plane transposes of Lorenzo differences (shafa_hipd_split_planes_grid_dev /
shafa_hipd_merge_planes_grid_dev, csrc/planes_lag.hip) and of the drivers on top (shafa-cd_amd/grids.py): declared, exported, bound
in Python, the ABI version, the submodule's names re-exported and its own, the __slots__, every argument error of the lag entries
refused before HIP is touched and in their order, the refusals of these entries' own (nlags; malformed rows of lags), how axes
become a tuple of lags, the drivers' ValueErrors before a device is touched, the refusals across the item classes, and a numpy
check of the reference the GPU tests lean on (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64
from test_planes_lag_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAMES = ("shafa_hipd_split_planes_grid_dev", "shafa_hipd_merge_planes_grid_dev")
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def grids(shafa):
    return pkgload.load_submodule("grids")


def test_declared_exported_and_bound(shafa, grids):
    declared = declared_symbols(HEADER)
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_grid_dev", "merge_planes_grid_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("split_grid", "merge_grid", "compress_grids", "decompress_grids"):
        assert callable(getattr(grids, name, None)), name
        assert getattr(shafa, name) is getattr(grids, name), name          # re-exported, and the submodule's own
        assert getattr(grids, name).__module__ == grids.__name__
    assert isinstance(grids.CompressedGrid, type) and shafa.CompressedGrid is grids.CompressedGrid
    assert grids.CompressedGrid.__module__ == grids.__name__
    assert grids.CompressedGrid.__slots__ == ("dtype", "shape", "lags", "planes", "nbytes")
    assert not issubclass(grids.CompressedGrid, shafa.CompressedTensor)
    with open(HEADER) as f:
        text = f.read()
    assert text.index("Byte planes of lagged differences") < text.index("Byte planes of Lorenzo differences") < text.index("Byte columns")
    assert f"#define SHAFA_PLANES_GRID_LAGS {shafa.PLANES_GRID_LAGS}\n" in text and shafa.PLANES_GRID_LAGS == 3


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    """the lag entries' checks in the lag entries' order (tests/test_planes_lag_cpu.py), on the stand-in batch, with nlags next to
    elem and the rows of lags where those entries check their lags"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE
    TOP = (1 << 64) - 1

    def poffs(elem):
        return _u64(*[16 * i for i in range(3 * elem)])

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=2, nl=3, lags=_u64(1, 0, 0, 1, 7, TOP, 1 << 63, TOP, 0), d_el=A.p, off=_u64(0, 6, (1 << 40) + 2),
                 cap=_u64(5, 100, 70000), d_n=A.p, d_planes=A.p, poff=_u64(0, 16, 32, 1 << 40, 4096, 4096 + 112))
        a.update(kw)
        if merge:
            return L.shafa_hipd_merge_planes_grid_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["d_planes"], a["poff"],
                                                      a["cap"], a["d_n"], a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_grid_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["d_el"], a["off"], a["cap"],
                                                  a["d_n"], a["d_planes"], a["poff"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed, with the rows (1, 0, 0), (1, 7, 2^64 - 1) and (2^63, 2^64 - 1, 0): HIP refuses the stand-in batch
    assert reached_hip(call())
    assert reached_hip(call(nl=2, lags=_u64(1, 0, 1 << 63, TOP, 3, 5))) and reached_hip(call(nl=1, lags=_u64(1, 7, TOP)))
    for elem in (1, 2, 4, 8):
        assert reached_hip(call(elem=elem, off=_u64(0, 8, (1 << 40) + 24), poff=poffs(elem))), elem
    # 1. the device pointers, the element size and nlags, in front of nblocks
    for k in ("b", "d_el", "d_planes", "d_n"):
        for nb in (3, 0, -1, 0x7FFFFFFF):
            assert call(**{k: None}, nb=nb) == OM, (k, nb)
    for elem in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    for nl in (0, 4, 0xFFFFFFFF):
        assert call(nl=nl) == OM and call(nl=nl, nb=0) == OM and call(nl=nl, nb=-1) == OM and call(nl=nl, nb=0x7FFFFFFF) == OM, nl
        assert call(nl=nl, lags=None, cap=None) == OM
    # 2. no block: success, the host arrays — the lags too — are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, poff=None, lags=None) == OK
    assert call(nb=0, d_el=A.odd, lags=_u64(*[0] * 9)) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, poff=None, lags=None) == LM
    # 4. the capacities, in front of the other host arrays, of the alignment rules and of the lags
    assert call(cap=None) == OM
    assert call(cap=None, off=None, poff=None, lags=None) == OM
    for elem in (1, 2, 4, 8):
        kw = dict(elem=elem, off=_u64(0, 8, 16), poff=poffs(elem))
        if elem > 1:
            assert call(cap=_u64(5, (1 << 64) // elem, 7), **kw) == LM, elem
        assert call(cap=_u64(TOP, 0, 0), **kw) == LM, elem
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, elem
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), elem
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big, off=None, poff=None) == LM                         # LACK_OF_MEMORY in front of a NULL host array,
    assert call(cap=big, d_planes=C.c_void_p(A.p.value + 8)) == LM          # of the plane side's alignment,
    assert call(cap=big, d_el=A.odd) == LM and call(cap=big, off=_u64(1, 3, 5)) == LM      # of the element side's alignment
    # 5. the other host arrays and the plane side's alignment
    for k in ("off", "poff"):
        assert call(**{k: None}) == OM, k
    for d in (1, 4, 8, 15):
        assert call(d_planes=C.c_void_p(A.p.value + d)) == OM, d
    for i in range(6):
        v = [0, 16, 32, 1 << 40, 4096, 4096 + 112]
        v[i] += 8
        assert call(poff=_u64(*v)) == OM, i
    # 5a. the rows of lags: NULL or malformed, in any block of the call — behind LACK_OF_MEMORY
    assert call(lags=None) == OM and call(cap=big, lags=None) == LM
    good = [(1, 0, 0), (1, 7, TOP), (1 << 63, TOP, 0)]
    for row in ((0, 1, 0), (0, 1, 2), (0, 0, 0), (3, 3, 0), (3, 3, 4), (5, 2, 0), (5, 6, 6), (5, 7, 6), (1, 0, 7), (TOP, TOP, 0)):
        for i in range(3):
            rows = list(good)
            rows[i] = row
            flat = _u64(*[g for r in rows for g in r])
            assert call(lags=flat) == OM, (row, i)
            assert call(cap=big, lags=flat) == LM, (row, i)
    for row in ((0, 1), (3, 3), (5, 2)):
        assert call(nl=2, lags=_u64(1, 2, *row, 4, 5)) == OM, row
    assert call(nl=1, lags=_u64(1, 0, 3)) == OM
    assert reached_hip(call(nb=2, lags=_u64(1, 0, 0, 1, 7, TOP, 5, 2, 0)))  # only the call's blocks are looked at
    assert reached_hip(call(nb=2, nl=2, lags=_u64(1, 2, 3, 4, 0, 1)))
    # 5b. the element side at multiples of the element: the address, and every offset
    for elem in (2, 4, 8):
        ok = [0, 8 * elem, (1 << 40) + 3 * elem]
        kw = dict(elem=elem, poff=poffs(elem))
        assert reached_hip(call(off=_u64(*ok), **kw)), elem
        for d in (1, elem - 1, elem // 2):
            assert call(d_el=C.c_void_p(A.p.value + d), off=_u64(*ok), **kw) == OM, (elem, d)
        assert reached_hip(call(d_el=C.c_void_p(A.p.value + elem), off=_u64(*ok), **kw)), elem
        for i in range(3):
            v = list(ok)
            v[i] += 1
            assert call(off=_u64(*v), **kw) == OM, (elem, i)
        assert reached_hip(call(nb=2, off=_u64(ok[0], ok[1], ok[2] + 1), **kw)), elem      # only the call's blocks
    for d in (0, 1, 5, 15):                                                 # elem 1 takes any address and any offsets
        assert reached_hip(call(elem=1, d_el=C.c_void_p(A.p.value + d), off=_u64(1, 3, (1 << 40) + 15), poff=poffs(1))), d


def test_the_binding_pads_the_rows(shafa):
    nl, lg = shafa._grid_lags("test", [(7,), (1, 7, 49), [2, 3]], 3)
    assert nl == 3 and lg.dtype == np.uint64 and lg.tolist() == [7, 0, 0, 1, 7, 49, 2, 3, 0]
    nl, lg = shafa._grid_lags("test", [(1 << 63, (1 << 64) - 1)], 1)
    assert nl == 2 and lg.tolist() == [1 << 63, (1 << 64) - 1]
    assert shafa._grid_lags("test", [], 0)[0] == 1
    with pytest.raises(ValueError, match="test: one tuple of lags per block"):
        shafa._grid_lags("test", [(1,)], 2)


def test_axes_to_lags(shafa, grids):
    import torch
    fake = lambda *shape: _FakeCuda(torch.zeros(shape, dtype=torch.int16))
    default = {(5,): (1,), (4, 6): (1, 6), (2, 3, 4): (1, 4, 12), (7, 1, 5): (1, 5), (2, 3, 4, 5): (1, 5, 20), (): (1,), (0, 4): (1,),
               (3, 0, 5): (1,), (3, 1, 9): (1, 9), (1, 1, 1): (1,)}
    for shape, want in default.items():
        assert grids._axes_lags("test", shape, None) == want, shape
        assert grids._lags("test", [fake(*shape)], None, None) == [want], shape
    # explicit axes: any order, negative ones from the back, duplicates dropped
    assert grids._axes_lags("test", (2, 3, 4), (0,)) == (12,) and grids._axes_lags("test", (2, 3, 4), (2, 0)) == (1, 12)
    assert grids._axes_lags("test", (2, 3, 4), (-1, -3)) == (1, 12) and grids._axes_lags("test", (2, 3, 4), (1, -2, 1)) == (4,)
    assert grids._axes_lags("test", (2, 3, 4, 5), (0, 1, 3)) == (1, 20, 60)
    assert grids._axes_lags("test", (2, 1, 4, 5), (0, 1, 2, 3)) == (1, 5, 20)           # an axis of dimension 1 repeats a lag
    with pytest.raises(ValueError, match="test: axes .* make 4 distinct lags, more than 3"):
        grids._axes_lags("test", (2, 3, 4, 5), (0, 1, 2, 3))
    for ax in (3, -4, 100):
        with pytest.raises(ValueError, match=f"test: axis {ax} of a tensor of 3 dimensions"):
            grids._axes_lags("test", (2, 3, 4), (0, ax))
    for ax in (1.0, "0", None, True):
        with pytest.raises(ValueError, match="test: an axis is an int"):
            grids._axes_lags("test", (2, 3, 4), (ax,))
    for axes in ((), [], 1, "01", 1.5):
        with pytest.raises(ValueError, match="test: axes are a tuple of ints"):
            grids._axes_lags("test", (2, 3, 4), axes)
    # one tuple for all tensors, or a list with one per tensor
    ts = [fake(5), fake(4, 6), fake(2, 3, 4)]
    assert grids._lags("test", ts, None, None) == [(1,), (1, 6), (1, 4, 12)]
    assert grids._lags("test", ts, (0,), None) == [(1,), (6,), (12,)]
    assert grids._lags("test", ts, (-1,), None) == [(1,), (1,), (1,)]
    assert grids._lags("test", ts, [(0,), (0, 1), None], None) == [(1,), (1, 6), (1, 4, 12)]
    for axes in ([], [(0,)], [0, 1, 2], [(0,), (0,), (0,), (0,)]):
        with pytest.raises(ValueError, match="test: axes is a tuple of ints or a list with one tuple per tensor"):
            grids._lags("test", ts, axes, None)
    # lags override axes
    assert grids._lags("test", ts, "ignored", (3, 5)) == [(3, 5)] * 3
    assert grids._lags("test", ts, None, [(1,), [2, 1 << 40], (1, 2, (1 << 64) - 1)]) == [(1,), (2, 1 << 40), (1, 2, (1 << 64) - 1)]
    for bad in ((), (1, 2, 3, 4), 3, "12", None):
        with pytest.raises(ValueError, match="test: lags are a tuple of 1 .. 3 ints"):
            grids._lag_tuple("test", bad)
    for bad in ((0,), (1, -1), (1, 1 << 64), (2.0,), ("3",), (True,), (1, None)):
        with pytest.raises(ValueError, match="test: a lag is an int of 1 .. 2\\^64 - 1 elements"):
            grids._lag_tuple("test", bad)
    for bad in ((3, 3), (5, 2), (1, 7, 7), (1, 9, 8)):
        with pytest.raises(ValueError, match="test: lags are strictly increasing"):
            grids._lag_tuple("test", bad)
    for bad in ([], [(1,)], [1, 2, 3]):
        with pytest.raises(ValueError, match="test: lags is a tuple of ints or a list with one tuple per tensor"):
            grids._lags("test", ts, None, bad)


def test_drivers_refuse_bad_arguments_before_a_device(shafa, grids, monkeypatch):
    import torch
    # any device work would need a stream or a batch: both refuse to be made here
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(64, dtype=torch.float32)
    meta = lambda *shape, dtype=torch.int16: torch.zeros(*shape, dtype=dtype, device="meta")      # never reaches a device
    # compress_grids: compress_tensors' argument errors, message for message but for the name in front
    for bad in (None, b"abc", 5, cpu, [cpu], [None], [meta(4, dtype=torch.complex64)]):
        with pytest.raises(ValueError) as mine:
            grids.compress_grids(bad)
        with pytest.raises(ValueError) as theirs:
            shafa.compress_tensors(bad)
        assert str(mine.value) == str(theirs.value).replace("compress_tensors", "compress_grids"), bad
        assert str(mine.value).startswith("compress_grids: ")
    assert grids.compress_grids([]) == [] and grids.decompress_grids([]) == []
    for bs in (-1, 1 << 64, 1.5, None, True):
        with pytest.raises(ValueError, match="compress_grids: block_size"):
            grids.compress_grids([], block_size=bs)
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.int16))
    g4 = _FakeCuda(torch.zeros(2, 3, 4, 5, dtype=torch.int16))
    for ax in (2, -3, 100):
        with pytest.raises(ValueError, match=f"compress_grids: axis {ax} of a tensor of 2 dimensions"):
            grids.compress_grids(f, axes=(0, ax))
    with pytest.raises(ValueError, match="compress_grids: an axis is an int"):
        grids.compress_grids(f, axes=(0, 1.0))
    with pytest.raises(ValueError, match="compress_grids: axes are a tuple of ints"):
        grids.compress_grids(f, axes=0)
    with pytest.raises(ValueError, match="compress_grids: axes is a tuple of ints or a list with one tuple per tensor"):
        grids.compress_grids([f], axes=[(0,), (1,)])
    with pytest.raises(ValueError, match="compress_grids: axes .* make 4 distinct lags, more than 3"):
        grids.compress_grids(g4, axes=(0, 1, 2, 3))
    with pytest.raises(ValueError, match="compress_grids: a lag is an int of 1 .. 2\\^64 - 1 elements"):
        grids.compress_grids(f, lags=(0, 6))
    with pytest.raises(ValueError, match="compress_grids: lags are strictly increasing"):
        grids.compress_grids(f, lags=(6, 1))
    with pytest.raises(ValueError, match="compress_grids: lags are a tuple of 1 .. 3 ints"):
        grids.compress_grids(f, lags=(1, 2, 3, 4))
    with pytest.raises(ValueError, match="compress_grids: lags is a tuple of ints or a list with one tuple per tensor"):
        grids.compress_grids([f], lags=[(1,), (6,)])
    # split_grid / merge_grid
    for bad in (None, b"abc", [cpu]):
        with pytest.raises(ValueError, match="split_grid: a contiguous CUDA tensor"):
            grids.split_grid(bad, (1, 3))
    with pytest.raises(ValueError, match="split_grid: contiguous CUDA tensors"):
        grids.split_grid(cpu, (1, 3))
    for g in (3, None, (), (0,), (3, 3), (1, 2, 3, 4), (1.5,)):
        with pytest.raises(ValueError, match="split_grid: (lags are|a lag is)"):
            grids.split_grid(f, g)
    u8 = torch.zeros(2, 64, dtype=torch.uint8)
    for planes, dtype, shape, g in ((None, torch.int16, (64,), (1, 3)), (u8, "int16", (64,), (1, 3)), (u8, torch.int16, 64, (1, 3)),
                                    (u8, torch.int16, (-64,), (1, 3)), (u8, torch.int16, (64,), (0,)), (u8, torch.int16, (64,), None),
                                    (u8, torch.int16, (64,), (3, 1)), (u8, torch.int16, (65,), (1, 3)),
                                    (u8, torch.float32, (32,), (1, 3)), (u8[0], torch.uint8, (64,), (1,)),
                                    (u8.to(torch.int8), torch.int16, (64,), (1, 3)), (u8, torch.complex128, (8,), (1,)),
                                    (u8, torch.int16, (64,), (1, 3))):
        with pytest.raises(ValueError, match="merge_grid: "):
            grids.merge_grid(planes, dtype, shape, g)


def test_items_are_kept_apart(shafa, grids, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    raw = torch.zeros(8, dtype=torch.uint8)
    CG = grids.CompressedGrid
    cg = CG(torch.int16, [2, 4], (1, 4), [raw, raw], 16)
    assert (cg.dtype, cg.shape, cg.lags, cg.nbytes) == (torch.int16, (2, 4), (1, 4), 16) and len(cg.planes) == 2
    assert repr(cg).startswith("CompressedGrid(torch.int16, (2, 4), lags=(1, 4), planes=['raw', 'raw']")
    assert not hasattr(cg, "__dict__")
    # the existing decompressors refuse a CompressedGrid with their present ValueError
    for arg in (cg, [cg]):
        with pytest.raises(ValueError, match="decompress_tensors: a CompressedTensor or a list of them"):
            shafa.decompress_tensors(arg)
    with pytest.raises(ValueError, match="decompress_deltas: a CompressedDelta / CompressedTensor or a list of them"):
        shafa.decompress_deltas([cg], [None])
    with pytest.raises(ValueError, match="decompress_sequences: a CompressedSequence or a list of them"):
        shafa.decompress_sequences([cg])
    with pytest.raises(ValueError, match="decompress_records: a CompressedRecords or a list of them"):
        shafa.decompress_records([cg])
    with pytest.raises(ValueError, match="decompress_strided: a CompressedStrided or a list of them"):
        shafa.decompress_strided([cg])
    # decompress_grids refuses everything else: all five existing item classes
    others = (shafa.CompressedTensor(torch.int16, (8,), [raw, raw], 16), shafa.CompressedDelta(torch.int16, (8,), [raw, raw], 16),
              shafa.CompressedSequence(torch.int16, (8,), [raw, raw], 16),
              shafa.CompressedRecords(torch.int16, (8,), 2, [raw, raw], 16),
              shafa.CompressedStrided(torch.int16, (8,), 1, [raw, raw], 16))
    for bad in others + (None, 5, [None], [raw], {"a": 1}):
        with pytest.raises(ValueError, match="decompress_grids: a CompressedGrid or a list of them"):
            grids.decompress_grids(bad)
    for bad in others:
        with pytest.raises(ValueError, match="decompress_grids: a CompressedGrid or a list of them"):
            grids.decompress_grids([cg, bad])
    # malformed items of its own: the lags, then decompress_tensors' checks under this driver's name
    for g in (0, 4, None, (), (0,), (4, 4), (4, 1), (1, 2, 3, 4), (2.0,), (True,), (1 << 64,)):
        with pytest.raises(ValueError, match="decompress_grids: (lags are|a lag is)"):
            grids.decompress_grids(CG(torch.int16, (2, 4), g, [raw, raw], 16))
    with pytest.raises(ValueError, match="decompress_grids: torch.int16 has 2 planes"):
        grids.decompress_grids(CG(torch.int16, (8,), (1,), [raw], 8))
    with pytest.raises(ValueError, match="decompress_grids: planes are CUDA tensors"):
        grids.decompress_grids([cg])
    with pytest.raises(ValueError, match="decompress_grids: negative dimension"):
        grids.decompress_grids(CG(torch.int16, (-8,), (1,), [raw, raw], 16))
    with pytest.raises(ValueError, match="decompress_grids: torch.complex128 has elements of 16 bytes"):
        grids.decompress_grids(CG(torch.complex128, (1,), (1,), [raw] * 16, 16))


# ---------------------------------------------------------------- the reference of tests/test_gpu_planes_grid.py
def grid_diff(x, lags):
    """d = the product of (1 - S^L) over `lags` applied to the unsigned array x (zero in front of it), mod 2^(8 k): successive
    shifted subtractions"""
    d = x.copy()
    for L in lags:
        if L < d.size:
            prev = d.copy()
            d[L:] -= prev[:-L]                                             # wraps mod M
    return d


def grid_sum(d, lags):
    """grid_diff's inverse: per lag a prefix sum down the columns of the rows of L elements, padded"""
    x = d.copy()
    n = x.size
    for L in lags:
        L = min(L, max(n, 1))
        R = -(-n // L)
        p = np.zeros(R * L, x.dtype)
        p[:n] = x
        x = np.cumsum(p.reshape(R, L), axis=0, dtype=x.dtype).reshape(-1)[:n]
    return x


def _taps(x, lags):
    """the definition written as taps: d[i] = sum over the subsets A of the lags of (-1)^|A| x[i - sum A]"""
    d = np.zeros_like(x)
    for sub in range(1 << len(lags)):
        dist = sum(L for k, L in enumerate(lags) if sub >> k & 1)
        sign = bin(sub).count("1") & 1
        if dist < x.size:
            t = np.zeros_like(x)
            t[dist:] = x[:x.size - dist]
            d = d - t if sign else d + t
    return d


@pytest.mark.parametrize("k", (1, 2, 4, 8))
def test_the_reference_checks_itself(k):
    """taps = successive shifted subtractions = the inverse of the successive prefix sums, mod 2^(8 k)"""
    U = UINT[k]
    rng = np.random.default_rng(k)
    for n, lags in ((40, (1, 7)), (100, (3, 5, 15)), (40, (3, 60)), (200, (1, 8, 32)), (50, (2, 3, 5)), (33, (1, 33)), (33, (1, 32)),
                    (64, (5,)), (0, (1, 2)), (1, (1, 2, 3)), (70, (1, 1 << 40)), (300, (15, 16, 17))):
        x = np.frombuffer(rng.integers(0, 256, n * k, dtype=np.uint8).tobytes(), U).copy()
        with np.errstate(over="ignore"):
            d = grid_diff(x, lags)
            assert d.tobytes() == _taps(x, lags).tobytes(), (n, lags)
            assert grid_sum(d, lags).tobytes() == x.tobytes(), (n, lags)
            assert grid_sum(d, lags[::-1]).tobytes() == x.tobytes(), (n, lags)             # the passes commute
            z = rng.integers(0, 256, n * k, dtype=np.uint8).view(U)                       # and on anything
            assert grid_diff(grid_sum(z, lags), lags).tobytes() == z.tobytes(), (n, lags)

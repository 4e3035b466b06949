"""CPU-side checks of the byte-plane transposes of lagged differences (shafa_hipd_split_planes_lag_dev /
shafa_hipd_merge_planes_lag_dev, csrc/planes_lag.hip) and of the drivers on top (shafa-cd_amd/strided.py): declared, exported,
bound in Python, the ABI version, the submodule's names re-exported and its own, the __slots__, every argument error of the plain
entries refused before HIP is touched and in the plain entries' order, the two refusals of these entries' own (a lag of 0 or no
lags; an element side off the element's alignment), the drivers' ValueErrors before a device is touched, and how an axis becomes
a lag (no GPU needed)."""
import ctypes as C
import os

import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAMES = ("shafa_hipd_split_planes_lag_dev", "shafa_hipd_merge_planes_lag_dev")


@pytest.fixture(scope="module")
def strided(shafa):
    return pkgload.load_submodule("strided")


def test_declared_exported_and_bound(shafa, strided):
    declared = declared_symbols(HEADER)
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_lag_dev", "merge_planes_lag_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("split_strided", "merge_strided", "compress_strided", "decompress_strided"):
        assert callable(getattr(strided, name, None)), name
        assert getattr(shafa, name) is getattr(strided, name), name        # re-exported, and the submodule's own
        assert getattr(strided, name).__module__ == strided.__name__
    assert isinstance(strided.CompressedStrided, type) and shafa.CompressedStrided is strided.CompressedStrided
    assert strided.CompressedStrided.__module__ == strided.__name__
    assert strided.CompressedStrided.__slots__ == ("dtype", "shape", "lag", "planes", "nbytes")
    assert not issubclass(strided.CompressedStrided, shafa.CompressedTensor)
    with open(HEADER) as f:
        text = f.read()
    assert "Byte planes of lagged differences" in text
    assert text.index("Byte planes of differences") < text.index("Byte planes of lagged differences") < text.index("Byte columns")
    for name, v in (("STRIP", shafa.PLANES_LAG_STRIP), ("ROWS", shafa.PLANES_LAG_ROWS), ("ITEMS", shafa.PLANES_LAG_ITEMS)):
        assert f"#define SHAFA_PLANES_LAG_{name} {v}" in text, name
    assert shafa.PLANES_LAG_STRIP * shafa.PLANES_LAG_ROWS == shafa.PLANES_TILE


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    """the plain entries' checks in the plain entries' order (tests/test_planes_cpu.py), on the stand-in batch, with the two
    additions among the other host arrays"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE

    def poffs(elem):
        return _u64(*[16 * i for i in range(3 * elem)])

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=2, lag=_u64(1, 7, (1 << 64) - 1), d_el=A.p, off=_u64(0, 6, (1 << 40) + 2), cap=_u64(5, 100, 70000),
                 d_n=A.p, d_planes=A.p, poff=_u64(0, 16, 32, 1 << 40, 4096, 4096 + 112))
        a.update(kw)
        if merge:
            return L.shafa_hipd_merge_planes_lag_dev(a["b"], None, a["nb"], a["elem"], a["lag"], a["d_planes"], a["poff"], a["cap"],
                                                     a["d_n"], a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_lag_dev(a["b"], None, a["nb"], a["elem"], a["lag"], a["d_el"], a["off"], a["cap"], a["d_n"],
                                                 a["d_planes"], a["poff"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed (lags of 1, past every capacity and 2^64 - 1): HIP refuses the stand-in batch
    assert reached_hip(call())
    for elem in (1, 2, 4, 8):
        assert reached_hip(call(elem=elem, off=_u64(0, 8, (1 << 40) + 24), poff=poffs(elem))), elem
    # 1. the device pointers and the element size, in front of nblocks
    for k in ("b", "d_el", "d_planes", "d_n"):
        assert call(**{k: None}) == OM, k
        assert call(**{k: None}, nb=0) == OM, k
        assert call(**{k: None}, nb=-1) == OM, k
        assert call(**{k: None}, nb=0x7FFFFFFF) == OM, k
    for elem in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    assert call(b=None, elem=3) == OM
    # 2. no block: success, the host arrays — the lags too — are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, poff=None, lag=None) == OK
    assert call(nb=0, d_el=A.odd, lag=_u64(0, 0, 0)) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, poff=None, lag=None) == LM
    # 4. the capacities, in front of the other host arrays, of the alignment rules and of the lags
    assert call(cap=None) == OM
    assert call(cap=None, off=None, poff=None, lag=None) == OM
    for elem in (1, 2, 4, 8):
        kw = dict(elem=elem, off=_u64(0, 8, 16), poff=poffs(elem))
        if elem > 1:
            assert call(cap=_u64(5, (1 << 64) // elem, 7), **kw) == LM, elem
        assert call(cap=_u64((1 << 64) - 1, 0, 0), **kw) == LM, elem
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, elem
        assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1), **kw) == LM, elem
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), elem
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big, off=None, poff=None) == LM                         # LACK_OF_MEMORY in front of a NULL host array,
    assert call(cap=big, d_planes=C.c_void_p(A.p.value + 8)) == LM          # of the plane side's alignment,
    assert call(cap=big, lag=None) == LM and call(cap=big, lag=_u64(0, 0, 0)) == LM        # of the lags
    assert call(cap=big, d_el=A.odd) == LM and call(cap=big, off=_u64(1, 3, 5)) == LM      # and of the element side's alignment
    # 5. the other host arrays and the plane side's alignment
    for k in ("off", "poff"):
        assert call(**{k: None}) == OM, k
    for d in (1, 4, 8, 15):
        assert call(d_planes=C.c_void_p(A.p.value + d)) == OM, d
    for i in range(6):
        v = [0, 16, 32, 1 << 40, 4096, 4096 + 112]
        v[i] += 8
        assert call(poff=_u64(*v)) == OM, i
    # 5a. the lags: NULL, or a 0 in any block of the call
    assert call(lag=None) == OM
    for i in range(3):
        v = [1, 7, 1 << 63]
        v[i] = 0
        assert call(lag=_u64(*v)) == OM, i
    assert reached_hip(call(nb=2, lag=_u64(3, 1, 0)))                       # only the call's blocks are looked at
    # 5b. the element side at multiples of the element: the address, and every offset
    for elem in (2, 4, 8):
        good = [0, 8 * elem, (1 << 40) + 3 * elem]
        kw = dict(elem=elem, poff=poffs(elem))
        assert reached_hip(call(off=_u64(*good), **kw)), elem
        assert call(d_el=C.c_void_p(A.p.value + 1), off=_u64(*good), **kw) == OM, elem
        assert call(d_el=C.c_void_p(A.p.value + elem - 1), off=_u64(*good), **kw) == OM, elem
        assert call(d_el=C.c_void_p(A.p.value + elem // 2), off=_u64(*good), **kw) == OM, elem
        assert reached_hip(call(d_el=C.c_void_p(A.p.value + elem), off=_u64(*good), **kw)), elem
        for i in range(3):
            for d in (1, -1):
                v = list(good)
                v[i] = v[i] + d if v[i] + d >= 0 else elem + 1
                assert call(off=_u64(*v), **kw) == OM, (elem, i, d)
        assert reached_hip(call(nb=2, off=_u64(good[0], good[1], good[2] + 1), **kw)), elem    # only the call's blocks
    # elem 1 takes any address and any offsets
    for d in (0, 1, 5, 15):
        assert reached_hip(call(elem=1, d_el=C.c_void_p(A.p.value + d), off=_u64(1, 3, (1 << 40) + 15), poff=poffs(1))), d


class _FakeCuda:
    """a CPU tensor that says it is a contiguous CUDA tensor: what the checks look at, and nothing a device is needed for"""

    def __new__(cls, t):
        import torch

        class T(torch.Tensor):
            is_cuda = True
            device = torch.device("cuda", 0)

        return t.as_subclass(T)


def test_axis_to_lag(shafa, strided):
    import torch
    want = {(5,): [1], (4, 6): [6, 1], (2, 3, 4): [12, 4, 1]}
    for shape, lags in want.items():
        t = _FakeCuda(torch.zeros(shape, dtype=torch.int16))
        for ax, g in enumerate(lags):
            assert strided._lags("test", [t], ax, None) == [g], (shape, ax)
            assert strided._lags("test", [t], ax - len(shape), None) == [g], (shape, ax)
            assert strided._axis_lag("test", shape, ax) == g
        for ax in (len(shape), -len(shape) - 1, 7):
            with pytest.raises(ValueError, match=f"test: axis {ax} of a tensor of {len(shape)} dimensions"):
                strided._lags("test", [t], ax, None)
    ts = [_FakeCuda(torch.zeros(s, dtype=torch.float32)) for s in ((5,), (4, 6), (2, 3, 4))]
    assert strided._lags("test", ts, 0, None) == [1, 6, 12]
    assert strided._lags("test", ts, -1, None) == [1, 1, 1]
    assert strided._lags("test", ts, [0, 1, -2], None) == [1, 1, 4]
    # 0-dimensional and empty tensors take lag 1
    assert strided._lags("test", [_FakeCuda(torch.zeros(())), _FakeCuda(torch.zeros(0, 4)), _FakeCuda(torch.zeros(3, 0, 5))], 0,
                         None) == [1, 1, 1]
    assert strided._axis_lag("test", (0, 4), 1) == 1 and strided._axis_lag("test", (), -1) == 1
    # lag overrides axis
    assert strided._lags("test", ts, 0, 7) == [7, 7, 7]
    assert strided._lags("test", ts, "ignored", [1, 1 << 40, (1 << 64) - 1]) == [1, 1 << 40, (1 << 64) - 1]


def test_drivers_refuse_bad_arguments_before_a_device(shafa, strided, monkeypatch):
    import torch
    # any device work would need a stream or a batch: both refuse to be made here
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(64, dtype=torch.float32)
    meta = lambda *shape, dtype=torch.int16: torch.zeros(*shape, dtype=dtype, device="meta")      # never reaches a device
    # compress_strided: compress_tensors' argument errors, message for message but for the name in front
    for bad in (None, b"abc", 5, cpu, [cpu], [None], [meta(4, dtype=torch.complex64)]):
        with pytest.raises(ValueError) as mine:
            strided.compress_strided(bad)
        with pytest.raises(ValueError) as theirs:
            shafa.compress_tensors(bad)
        assert str(mine.value) == str(theirs.value).replace("compress_tensors", "compress_strided"), bad
        assert str(mine.value).startswith("compress_strided: ")
    assert strided.compress_strided([]) == [] and strided.decompress_strided([]) == []
    for bs in (-1, 1 << 64, 1.5, None, True):
        with pytest.raises(ValueError, match="compress_strided: block_size"):
            strided.compress_strided([], block_size=bs)
    # the axis and the lag
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.int16))
    for ax in (2, -3, 100):
        with pytest.raises(ValueError, match=f"compress_strided: axis {ax} of a tensor of 2 dimensions"):
            strided.compress_strided(f, axis=ax)
    for ax in (1.0, "0", None, True, [1.0]):
        with pytest.raises(ValueError, match="compress_strided: an axis is an int"):
            strided.compress_strided(f, axis=ax)
    for ax in ([], [0, 1], (0, 0, 0)):
        with pytest.raises(ValueError, match="compress_strided: axis is an int or a list with one int per tensor"):
            strided.compress_strided([f], axis=ax)
    for g in (0, -1, 1 << 64, 2.0, "3", True, [0], [None]):
        with pytest.raises(ValueError, match="compress_strided: a lag is an int of 1 .. 2\\^64 - 1 elements"):
            strided.compress_strided(f, lag=g)
    for g in ([], [3, 3], (1, 2, 3)):
        with pytest.raises(ValueError, match="compress_strided: lag is an int or a list with one int per tensor"):
            strided.compress_strided([f], lag=g)
    # split_strided / merge_strided
    for bad in (None, b"abc", [cpu]):
        with pytest.raises(ValueError, match="split_strided: a contiguous CUDA tensor"):
            strided.split_strided(bad, 3)
    with pytest.raises(ValueError, match="split_strided: contiguous CUDA tensors"):
        strided.split_strided(cpu, 3)
    for g in (0, -2, 1.5, None, True, 1 << 64):
        with pytest.raises(ValueError, match="split_strided: a lag is an int"):
            strided.split_strided(f, g)
    u8 = torch.zeros(2, 64, dtype=torch.uint8)
    for planes, dtype, shape, g in ((None, torch.int16, (64,), 3), (u8, "int16", (64,), 3), (u8, torch.int16, 64, 3),
                                    (u8, torch.int16, (-64,), 3), (u8, torch.int16, (64,), 0), (u8, torch.int16, (64,), None),
                                    (u8, torch.int16, (65,), 3), (u8, torch.float32, (32,), 3), (u8[0], torch.uint8, (64,), 1),
                                    (u8.to(torch.int8), torch.int16, (64,), 3), (u8, torch.complex128, (8,), 1),
                                    (u8, torch.int16, (64,), 3)):
        with pytest.raises(ValueError, match="merge_strided: "):
            strided.merge_strided(planes, dtype, shape, g)


def test_items_are_kept_apart(shafa, strided, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    raw = torch.zeros(8, dtype=torch.uint8)
    CS, CT = strided.CompressedStrided, shafa.CompressedTensor
    cs = CS(torch.int16, [2, 4], 4, [raw, raw], 16)
    assert (cs.dtype, cs.shape, cs.lag, cs.nbytes) == (torch.int16, (2, 4), 4, 16) and len(cs.planes) == 2
    assert repr(cs).startswith("CompressedStrided(torch.int16, (2, 4), lag=4, planes=['raw', 'raw']")
    assert not hasattr(cs, "__dict__")
    # the existing decompressors refuse a CompressedStrided with their present ValueError
    with pytest.raises(ValueError, match="decompress_tensors: a CompressedTensor or a list of them"):
        shafa.decompress_tensors(cs)
    with pytest.raises(ValueError, match="decompress_tensors: a CompressedTensor or a list of them"):
        shafa.decompress_tensors([cs])
    with pytest.raises(ValueError, match="decompress_deltas: a CompressedDelta / CompressedTensor or a list of them"):
        shafa.decompress_deltas([cs], [None])
    with pytest.raises(ValueError, match="decompress_sequences: a CompressedSequence or a list of them"):
        shafa.decompress_sequences([cs])
    with pytest.raises(ValueError, match="decompress_records: a CompressedRecords or a list of them"):
        shafa.decompress_records([cs])
    # decompress_strided refuses everything else
    others = (CT(torch.int16, (8,), [raw, raw], 16), shafa.CompressedDelta(torch.int16, (8,), [raw, raw], 16),
              shafa.CompressedSequence(torch.int16, (8,), [raw, raw], 16), shafa.CompressedRecords(torch.int16, (8,), 2, [raw, raw], 16))
    for bad in others + (None, 5, [None], [raw], {"a": 1}):
        with pytest.raises(ValueError, match="decompress_strided: a CompressedStrided or a list of them"):
            strided.decompress_strided(bad)
    for bad in others:
        with pytest.raises(ValueError, match="decompress_strided: a CompressedStrided or a list of them"):
            strided.decompress_strided([cs, bad])
    # malformed items of its own: the lag, then decompress_tensors' checks under this driver's name
    for g in (0, -4, 2.0, None, "4", True, 1 << 64):
        with pytest.raises(ValueError, match="decompress_strided: a lag is an int"):
            strided.decompress_strided(CS(torch.int16, (2, 4), g, [raw, raw], 16))
    with pytest.raises(ValueError, match="decompress_strided: torch.int16 has 2 planes"):
        strided.decompress_strided(CS(torch.int16, (8,), 1, [raw], 8))
    with pytest.raises(ValueError, match="decompress_strided: planes are CUDA tensors"):
        strided.decompress_strided([cs])
    with pytest.raises(ValueError, match="decompress_strided: negative dimension"):
        strided.decompress_strided(CS(torch.int16, (-8,), 1, [raw, raw], 16))
    with pytest.raises(ValueError, match="decompress_strided: torch.complex128 has elements of 16 bytes"):
        strided.decompress_strided(CS(torch.complex128, (1,), 1, [raw] * 16, 16))

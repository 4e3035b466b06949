"""CPU-side checks of the plane histograms of Lorenzo differences (shafa_hipd_hist_planes_grid_dev, csrc/planes_lag.hip) and of the
choosers on top (grid_histograms / grid_sizes / choose_lags, shafa-cd_amd/grids.py): declared, exported, bound, the ABI version,
the header's section in its place and its define mirrored, every argument error refused before HIP is touched and in the grid
split's order, the rows of lags with the row of zeros allowed, the drivers' ValueErrors before a device is touched, the default
candidates from shapes, and the numpy model of the sizes, which tests/test_gpu_planes_grid_hist.py leans on, checking itself on
three tensors (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64
from test_planes_grid_cpu import grid_diff
from test_planes_lag_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAME = "shafa_hipd_hist_planes_grid_dev"
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def grids(shafa):
    return pkgload.load_submodule("grids")


def test_declared_exported_and_bound(shafa, grids):
    assert NAME in declared_symbols(HEADER)
    assert hasattr(C.CDLL(shafa.LIB_PATH), NAME)
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "hist_planes_grid_dev", None))
    for name in ("grid_histograms", "grid_sizes", "choose_lags"):
        assert callable(getattr(grids, name, None)), name
        assert getattr(shafa, name) is getattr(grids, name), name          # re-exported, and the submodule's own
        assert getattr(grids, name).__module__ == grids.__name__
    with open(HEADER) as f:
        text = f.read()
    assert text.index("Byte planes of Lorenzo differences") < text.index("Plane histograms of Lorenzo differences") \
        < text.index(NAME + "(") < text.index("Byte columns")
    assert text.index("shafa_hipd_merge_planes_grid_dev(") < text.index("Plane histograms of Lorenzo differences")
    assert f"#define SHAFA_PLANES_HIST_RUN {shafa.PLANES_HIST_RUN} " in text and shafa.PLANES_HIST_RUN >= 1


def test_argument_errors_before_hip(shafa):
    """the grid split's checks in the grid split's order (tests/test_planes_grid_cpu.py) on the stand-in batch, d_freq in d_planes'
    place, no plane side, and the row of zeros allowed"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE
    TOP = (1 << 64) - 1

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=2, nl=3, lags=_u64(0, 0, 0, 1, 0, 0, 1, 7, TOP), d_in=A.p, off=_u64(0, 6, (1 << 40) + 2),
                 cap=_u64(5, 100, 70000), d_n=A.p, d_freq=A.p)
        a.update(kw)
        return L.shafa_hipd_hist_planes_grid_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["d_in"], a["off"], a["cap"],
                                                 a["d_n"], a["d_freq"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed, with the rows (0, 0, 0), (1, 0, 0) and (1, 7, 2^64 - 1): HIP refuses the stand-in batch
    assert reached_hip(call())
    assert reached_hip(call(nl=2, lags=_u64(0, 0, 1 << 63, TOP, 3, 5))) and reached_hip(call(nl=1, lags=_u64(0, 7, TOP)))
    for elem in (1, 2, 4, 8):
        assert reached_hip(call(elem=elem, off=_u64(0, 8, (1 << 40) + 24))), elem
    assert reached_hip(call(off=_u64(0, 0, 0), cap=_u64(70000, 70000, 70000)))              # blocks may coincide
    assert reached_hip(call(d_freq=A.odd))                                                  # no alignment rule on the counts here
    # 1. the device pointers, the element size and nlags, in front of nblocks
    for k in ("b", "d_in", "d_n", "d_freq"):
        for nb in (3, 0, -1, 0x7FFFFFFF):
            assert call(**{k: None}, nb=nb) == OM, (k, nb)
    for elem in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    for nl in (0, 4, 0xFFFFFFFF):
        assert call(nl=nl) == OM and call(nl=nl, nb=0) == OM and call(nl=nl, nb=-1) == OM and call(nl=nl, nb=0x7FFFFFFF) == OM, nl
        assert call(nl=nl, lags=None, cap=None) == OM
    # 2. no block: success, no host array is looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, lags=None) == OK
    assert call(nb=0, d_in=A.odd, lags=_u64(0, 1, 0, 3, 3, 0, 5, 2, 0)) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, lags=None) == LM
    # 4. the capacities, in front of the other host arrays, of the alignment rule and of the lags
    assert call(cap=None) == OM
    assert call(cap=None, off=None, lags=None) == OM
    for elem in (1, 2, 4, 8):
        kw = dict(elem=elem, off=_u64(0, 8, 16))
        if elem > 1:
            assert call(cap=_u64(5, (1 << 64) // elem, 7), **kw) == LM, elem
        assert call(cap=_u64(TOP, 0, 0), **kw) == LM, elem
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, elem
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), elem
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big, off=None) == LM and call(cap=big, lags=None) == LM                 # LACK_OF_MEMORY in front of a NULL host array,
    assert call(cap=big, d_in=A.odd) == LM and call(cap=big, off=_u64(1, 3, 5)) == LM       # of the element side's alignment,
    assert call(cap=big, lags=_u64(0, 1, 0, 1, 0, 0, 1, 0, 0)) == LM                        # and of a malformed row
    # 5. the other host arrays
    assert call(off=None) == OM and call(lags=None) == OM
    # 5a. the element side at multiples of the element: the address, and every offset
    for elem in (2, 4, 8):
        ok = [0, 8 * elem, (1 << 40) + 3 * elem]
        assert reached_hip(call(elem=elem, off=_u64(*ok))), elem
        for d in (1, elem - 1, elem // 2):
            assert call(elem=elem, d_in=C.c_void_p(A.p.value + d), off=_u64(*ok)) == OM, (elem, d)
        assert reached_hip(call(elem=elem, d_in=C.c_void_p(A.p.value + elem), off=_u64(*ok))), elem
        for i in range(3):
            v = list(ok)
            v[i] += 1
            assert call(elem=elem, off=_u64(*v)) == OM, (elem, i)
        assert reached_hip(call(elem=elem, nb=2, off=_u64(ok[0], ok[1], ok[2] + 1))), elem  # only the call's blocks
    for d in (0, 1, 5, 15):                                                 # elem 1 takes any address and any offsets
        assert reached_hip(call(elem=1, d_in=C.c_void_p(A.p.value + d), off=_u64(1, 3, (1 << 40) + 15))), d
    # 5b. the rows of lags: malformed in any block of the call; the row of zeros and the grid entries' rows pass
    good = [(0, 0, 0), (1, 0, 0), (1, 7, TOP)]
    for row in ((0, 1, 0), (0, 1, 2), (0, 0, 5), (3, 3, 0), (3, 3, 4), (5, 2, 0), (5, 6, 6), (5, 7, 6), (1, 0, 7), (TOP, TOP, 0)):
        for i in range(3):
            rows = list(good)
            rows[i] = row
            assert call(lags=_u64(*[g for r in rows for g in r])) == OM, (row, i)
    for row in ((0, 1), (3, 3), (5, 2)):
        assert call(nl=2, lags=_u64(1, 2, *row, 0, 0)) == OM, row
    for row in good + [(1 << 63, TOP, 0), (2, 3, 5)]:
        assert reached_hip(call(lags=_u64(*row * 3))), row
    assert reached_hip(call(nb=2, lags=_u64(0, 0, 0, 1, 7, TOP, 5, 2, 0)))  # only the call's blocks are looked at


def test_the_binding_takes_the_empty_tuple(shafa):
    nl, lg = shafa._grid_lags("test", [(), (1, 64), (7,)], 3)
    assert nl == 2 and lg.tolist() == [0, 0, 1, 64, 7, 0]
    nl, lg = shafa._grid_lags("test", [(), ()], 2)
    assert nl == 1 and lg.tolist() == [0, 0]


def test_default_candidates_from_shapes(shafa, grids):
    want = {(5,): [(), (1,)], (4, 6): [(), (1,), (6,), (1, 6)],
            (2, 3, 4): [(), (1,), (4,), (12,), (1, 4), (1, 12), (4, 12), (1, 4, 12)], (1, 7): [(), (1,), (7,), (1, 7)],
            (7, 1): [(), (1,)], (2, 3, 4, 5): [(), (1,), (5,), (20,), (1, 5), (1, 20), (5, 20), (1, 5, 20)]}
    for shape, cands in want.items():
        got = grids._default_candidates("test", shape, None)
        assert got == cands and len(set(got)) == len(got) <= 8, shape
    assert grids._default_candidates("test", (2, 3, 4), (0, -1)) == [(), (1,), (12,), (1, 12)]
    import torch
    ts = [_FakeCuda(torch.zeros(s, dtype=torch.int16)) for s in ((5,), (4, 6))]
    assert grids._candidates("test", ts, None, None) == [want[(5,)], want[(4, 6)]]
    assert grids._candidates("test", ts, (0,), None) == [[(), (1,)], [(), (6,)]]
    assert grids._candidates("test", ts, [(0,), None], None) == [[(), (1,)], want[(4, 6)]]
    assert grids._candidates("test", ts, "ignored", [(), (3, 5)]) == [[(), (3, 5)]] * 2
    assert grids._candidates("test", ts, None, [[()], [(2,), (1, 2, 1 << 40)]]) == [[()], [(2,), (1, 2, 1 << 40)]]


def test_drivers_refuse_bad_arguments_before_a_device(shafa, grids, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(64, dtype=torch.float32)
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.int16))
    for drv in (grids.grid_sizes, grids.choose_lags):
        assert drv([]) == []
        for bad in (None, b"abc", 5, cpu, [cpu], [None]):
            with pytest.raises(ValueError, match="grid_sizes: "):
                drv(bad)
        for cands in ([1], [(1,), 6], [(1,), "6"], [None], [[(1,)], [6]]):                 # a candidate that is no tuple
            with pytest.raises(ValueError, match="grid_sizes: a candidate is a tuple of lags"):
                drv([f, f] if isinstance(cands[0], list) else f, candidates=cands)
        for cands in ([(0,)], [(), (1, -1)], [(2.0,)], [(True,)], [(1 << 64,)]):            # what _lag_tuple refuses
            with pytest.raises(ValueError, match="grid_sizes: a lag is an int of 1 .. 2\\^64 - 1 elements"):
                drv(f, candidates=cands)
        for cands in ([(3, 3)], [(), (5, 2)]):
            with pytest.raises(ValueError, match="grid_sizes: lags are strictly increasing"):
                drv(f, candidates=cands)
        with pytest.raises(ValueError, match="grid_sizes: lags are a tuple of 1 .. 3 ints"):
            drv(f, candidates=[(1, 2, 3, 4)])
        for cands in ([[(1,)]], [[()], [()], [()]]):                                         # a per-tensor list of the wrong length
            with pytest.raises(ValueError, match="grid_sizes: candidates is a list of tuples or a list with one such list per tensor"):
                drv([f, f], candidates=cands)
        for cands in ([], (), ((1,),), "x", 5, [[], [()]]):
            with pytest.raises(ValueError, match="grid_sizes: candidates are a non-empty list of tuples of lags"):
                drv([f, f], candidates=cands)
        with pytest.raises(ValueError, match="grid_sizes: axis 2 of a tensor of 2 dimensions"):
            drv(f, axes=(0, 2))
        with pytest.raises(ValueError, match="grid_sizes: axes is a tuple of ints or a list with one tuple per tensor"):
            drv([f], axes=[(0,), (1,)])
    assert grids._candidate("test", ()) == () and grids._candidate_list("test", [(), (1, 6)]) == [(), (1, 6)]
    for bad in (None, b"abc", [cpu]):
        with pytest.raises(ValueError, match="grid_histograms: a contiguous CUDA tensor"):
            grids.grid_histograms(bad, [()])
    with pytest.raises(ValueError, match="grid_histograms: contiguous CUDA tensors"):
        grids.grid_histograms(cpu, [()])
    for sets in (None, 5, "ab"):
        with pytest.raises(ValueError, match="grid_histograms: lag_sets is a list of tuples of lags"):
            grids.grid_histograms(f, sets)
    for sets in ([1], [[1]], [(), None]):
        with pytest.raises(ValueError, match="grid_histograms: a candidate is a tuple of lags"):
            grids.grid_histograms(f, sets)
    for sets in ([(0,)], [(3, 3)], [(1, 2, 3, 4)]):
        with pytest.raises(ValueError, match="grid_histograms: (lags are|a lag is)"):
            grids.grid_histograms(f, sets)


# ---------------------------------------------------------------- the model, which tests/test_gpu_planes_grid_hist.py leans on
def z_of(x, lags):
    """the unsigned array whose bytes are a candidate's planes: x itself for (), else the zigzag fold of grid_diff"""
    if not lags:
        return x
    bits = 8 * x.dtype.itemsize
    with np.errstate(over="ignore"):
        d = grid_diff(x, lags)
        return (d << x.dtype.type(1)) ^ (x.dtype.type(0) - (d >> x.dtype.type(bits - 1)))


def plane_histograms(x, lags):
    """[k, 256] counts of the bytes of the candidate's planes"""
    k = x.dtype.itemsize
    planes = np.ascontiguousarray(z_of(x, lags)).view(np.uint8).reshape(-1, k)
    return np.stack([np.bincount(planes[:, j], minlength=256) for j in range(k)]).astype(np.uint64)


def sf_bytes(shafa, freq):
    """the Shannon-Fano bytes of a block with this histogram under the table of the histogram: ceil(sum freq len / 8)"""
    tab = shafa.sf_build_codes(np.ascontiguousarray(freq, dtype=np.uint64))
    bits = int((freq.astype(object) * np.frombuffer(bytes(tab.len), np.uint8).astype(object)).sum())
    return -(-bits // 8)


def model_sizes(shafa, x, cands):
    """grid_sizes' list for the flat unsigned array x: (lags, sum over the planes of min(n, SF bytes)), sorted by its rule"""
    out = [(c, sum(min(x.size, sf_bytes(shafa, h)) for h in plane_histograms(x, c))) for c in cands]
    return sorted(out, key=lambda e: (e[1], len(e[0]), e[0]))


def the_field():
    """DESIGN 7.28's int32 [32, 64, 64] (tests/test_gpu_planes_grid.py, test_it_pays)"""
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.int64)
    i = (z * 64 + y) * 64 + x
    return (3 * x * x + 5 * x * y + 7 * y * z + 11 * z * z + 13 * x * z + ((i * 2654435761) >> 13 & 7)).astype(np.int32)


def the_column_walk():
    """int16 [4096, 64]: every column a random walk of its own, smooth down the columns and nowhere else"""
    return np.cumsum(np.random.default_rng(29).integers(-3, 4, (4096, 64)), axis=0).astype(np.int16)


def the_noise():
    return np.random.default_rng(31).integers(0, 1 << 32, (64, 300), dtype=np.uint32)


def three_tensors():
    return [the_field(), the_column_walk(), the_noise()]


def test_the_model_checks_itself(shafa, grids):
    """on the field the sort rule picks a two-lag set below compress_grids' default of all three axes — the table is the one the
    chooser was proposed with —, on the column walk the one axis that is smooth, on noise plain planes, every candidate a tie"""
    field, walk, noise = three_tensors()
    flat = lambda a: a.reshape(-1).view(UINT[a.dtype.itemsize])
    got = model_sizes(shafa, flat(field), grids._default_candidates("test", field.shape, None))
    assert got == [((1, 4096), 58911), ((64, 4096), 60671), ((1, 64), 67789), ((1, 64, 4096), 69524), ((64,), 153327),
                   ((4096,), 175947), ((1,), 179858), ((), 274115)]
    assert len(got[0][0]) == 2 and got[0][1] < dict(got)[(1, 64, 4096)]
    got = model_sizes(shafa, flat(walk), grids._default_candidates("test", walk.shape, None))
    assert got[0][0] == (64,) and got[0][1] < got[1][1] and sorted(c for c, _ in got) == [(), (1,), (1, 64), (64,)]
    got = model_sizes(shafa, flat(noise), grids._default_candidates("test", noise.shape, None))
    assert got == [(c, noise.size * 4) for c in ((), (1,), (300,), (1, 300))]
    # the histograms are those of the planes: every plane's counts sum to n, and () is the bytes as they lie
    h = plane_histograms(flat(field), ())
    assert h.sum(1).tolist() == [field.size] * 4
    assert h[1].tolist() == np.bincount(field.reshape(-1).view(np.uint8)[1::4], minlength=256).tolist()
    assert plane_histograms(np.zeros(0, np.uint16), (1,)).tolist() == [[0] * 256] * 2

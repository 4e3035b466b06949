"""CPU-side checks of the field sizes under an error bound (shafa_hipd_hist_planes_grid_quant_dev, csrc/planes_lag.hip) and of the
drivers on top (field_histograms / field_sizes / choose_field_lags / field_rates / fit_abs_error, shafa-cd_amd/fields.py):
declared, exported, bound, the ABI version, the header's section in its place, the names re-exported and the submodule's own,
every argument error refused before HIP is touched in shafa_hipd_hist_planes_grid_dev's order with the quantising split's steps
and bounds where that checks its lags, the drivers' ValueErrors before a device is touched, and the numpy model of field_sizes,
which tests/test_gpu_field_hist.py leans on, checking itself on DESIGN 7.28's field (no GPU needed)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64
from test_fields_cpu import _f64, model, the_float_field
from test_planes_grid_hist_cpu import plane_histograms, sf_bytes
from test_planes_lag_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAME = "shafa_hipd_hist_planes_grid_quant_dev"
DRIVERS = ("field_histograms", "field_sizes", "choose_field_lags", "field_rates", "fit_abs_error")
UINT = {4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def fields(shafa):
    return pkgload.load_submodule("fields")


def test_declared_exported_and_bound(shafa, fields):
    assert NAME in declared_symbols(HEADER)
    assert hasattr(C.CDLL(shafa.LIB_PATH), NAME)
    fn = getattr(shafa.lib(), NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 14
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "hist_planes_grid_quant_dev", None))
    for name in DRIVERS:
        assert callable(getattr(fields, name, None)), name
        assert getattr(shafa, name) is getattr(fields, name), name          # re-exported, and the submodule's own
        assert getattr(fields, name).__module__ == fields.__name__
    with open(HEADER) as f:
        text = f.read()
    assert text.index("shafa_hipd_merge_planes_grid_quant_dev(") < text.index("Field sizes under an error bound") \
        < text.index(NAME + "(") < text.index("Byte columns")
    assert text.count(NAME + "(") == 1


def test_argument_errors_before_hip(shafa):
    """shafa_hipd_hist_planes_grid_dev's checks in its order (tests/test_planes_grid_hist_cpu.py) on the stand-in batch with elem 4
    or 8 at the elem check and no row of zeros, then, where that entry checks its lags, the quantising split's own
    (tests/test_fields_cpu.py) and d_outl_n"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE
    TOP = (1 << 64) - 1

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=4, nl=3, lags=_u64(1, 0, 0, 1, 7, TOP, 1 << 63, TOP, 0), step=_f64(0.5, 0.25, 3.0),
                 bound=_f64(0.25, 0.125, 2.0), d_in=A.p, off=_u64(0, 8, (1 << 40) + 24), cap=_u64(5, 100, 70000), d_n=A.p,
                 d_freq=A.p, d_outl_n=A.p)
        a.update(kw)
        return getattr(L, NAME)(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["step"], a["bound"], a["d_in"], a["off"],
                                a["cap"], a["d_n"], a["d_freq"], a["d_outl_n"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    assert reached_hip(call()) and reached_hip(call(elem=8))
    assert reached_hip(call(nl=1, lags=_u64(1, 7, TOP)))
    assert reached_hip(call(off=_u64(0, 0, 0), cap=_u64(70000, 70000, 70000)))              # blocks may coincide
    assert reached_hip(call(d_freq=A.odd, d_outl_n=A.odd))                                  # no alignment rule on the counts here
    # 1. the device pointers, nlags and the element size, in front of nblocks
    for k in ("b", "d_in", "d_n", "d_freq"):
        for nb in (3, 0, -1, 0x7FFFFFFF):
            assert call(**{k: None}, nb=nb) == OM, (k, nb)
    for nl in (0, 4, 0xFFFFFFFF):
        assert call(nl=nl) == OM and call(nl=nl, nb=0) == OM and call(nl=nl, nb=0x7FFFFFFF) == OM, nl
    for elem in (0, 1, 2, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):                   # floats and doubles only: 1 and 2 among the refused
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    # 2. no block: success, no host array is looked at — the entry's own neither, nor d_outl_n
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, lags=None, step=None, bound=None, d_outl_n=None) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F)
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF, cap=None, step=None, d_outl_n=None) == LM
    # 4. the capacities, in front of everything behind them
    assert call(cap=None) == OM and call(cap=None, step=None) == OM
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big) == LM and call(cap=_u64(TOP, 0, 0)) == LM and call(elem=8, cap=_u64(5, (1 << 64) // 8, 7)) == LM
    for kw in (dict(step=None), dict(bound=None), dict(step=_f64(0.0, 0.5, 0.5)), dict(bound=_f64(0.5, -1.0, 0.5)), dict(d_outl_n=None),
               dict(lags=None), dict(off=None), dict(lags=_u64(0, 0, 0, 1, 0, 0, 1, 0, 0)), dict(d_in=C.c_void_p(A.p.value + 2))):
        assert call(cap=big, **kw) == LM, kw
    # 5. the other host arrays, the element side at multiples of the element, the rows of lags
    assert call(off=None) == OM and call(lags=None) == OM
    assert call(off=_u64(0, 8, (1 << 40) + 26)) == OM and call(d_in=C.c_void_p(A.p.value + 2)) == OM
    assert call(elem=8, off=_u64(0, 8, (1 << 40) + 28)) == OM and call(elem=8, d_in=C.c_void_p(A.p.value + 4)) == OM
    good = [(1, 0, 0), (1, 7, TOP), (1 << 63, TOP, 0)]
    for row in ((0, 0, 0), (0, 1, 0), (0, 1, 2), (0, 0, 5), (3, 3, 0), (3, 3, 4), (5, 2, 0), (5, 6, 6), (5, 7, 6), (1, 0, 7),
                (TOP, TOP, 0)):                                             # the row of zeros is malformed here, as in the split
        for i in range(3):
            rows = list(good)
            rows[i] = row
            assert call(lags=_u64(*[g for r in rows for g in r])) == OM, (row, i)
    for row in ((0,), (0, 0), (0, 1), (3, 3), (5, 2)):
        assert call(nl=len(row), lags=_u64(*((1,) + (2,) * (len(row) - 1)), *row, *((1,) + (0,) * (len(row) - 1)))) == OM, row
    for row in good + [(2, 3, 5)]:
        assert reached_hip(call(lags=_u64(*row * 3))), row
    assert reached_hip(call(nb=2, lags=_u64(1, 0, 0, 1, 7, TOP, 0, 0, 0)))  # only the call's blocks are looked at
    # 6. the entry's own, where the lags are checked: NULL arrays and d_outl_n
    assert call(step=None) == OM and call(bound=None) == OM and call(d_outl_n=None) == OM
    # 7. a bad step, bound or inverse, in every block's place: the cases tests/test_fields_cpu.py runs for the split
    tiny32, tiny64 = float(np.finfo(np.float32).tiny), float(np.finfo(np.float64).tiny)
    bad = {4: [0.0, -0.5, math.nan, math.inf, -math.inf, 0.1, 1.0 + 2.0 ** -30, 1e-300, tiny32 / 2, 2.0 ** -149, 1e39],
           8: [0.0, -0.5, math.nan, math.inf, -math.inf, 5e-324, tiny64 / 2, tiny64 / 8]}
    ok = {4: [0.5, float(np.float32(0.1)), tiny32, 2.0 ** 100], 8: [0.5, 0.1, tiny64, 1e-300, 1e300]}
    for elem in (4, 8):
        for i in range(3):
            for v in bad[elem]:
                s = [0.5, 0.25, 3.0]
                s[i] = v
                assert call(elem=elem, step=_f64(*s)) == OM, (elem, i, v)
                assert call(elem=elem, bound=_f64(*s)) == OM, (elem, i, v)
            for v in ok[elem]:
                s = [0.5, 0.25, 3.0]
                s[i] = v
                assert reached_hip(call(elem=elem, step=_f64(*s))), (elem, i, v)
                assert reached_hip(call(elem=elem, bound=_f64(*s))), (elem, i, v)
        assert reached_hip(call(elem=elem, nb=2, step=_f64(0.5, 0.25, 0.0), bound=_f64(0.5, 0.25, -1.0)))   # only the call's blocks


def test_drivers_refuse_bad_arguments_before_a_device(shafa, fields, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(64, dtype=torch.float32)
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.float32))
    d = _FakeCuda(torch.zeros(4, 6, dtype=torch.float64))
    bad_bounds = (0, 0.0, -1e-3, math.nan, math.inf, None, "1e-3", True, 1e-46, 1e-40)
    # field_sizes and choose_field_lags: compress_fields' tensors and bounds, grid_sizes' candidates without ()
    for drv in (fields.field_sizes, fields.choose_field_lags):
        assert drv([], 1e-3) == []
        for bad in (None, b"abc", 5, cpu, [cpu], [None]):
            with pytest.raises(ValueError, match="field_sizes: "):
                drv(bad, 1e-3)
        for dt in (torch.int32, torch.bfloat16, torch.float16, torch.int64, torch.uint8):
            with pytest.raises(ValueError, match="field_sizes: float32 and float64 tensors"):
                drv([f, _FakeCuda(torch.zeros(8, dtype=dt))], 1e-3)
        for e in bad_bounds:
            with pytest.raises(ValueError, match="field_sizes: (abs_error is|an abs_error of)"):
                drv(f, e)
            with pytest.raises(ValueError, match="field_sizes: (abs_error is|an abs_error of)"):
                drv([d, f], [1e-3, e])
        for e in (1e-320, 5e-324):
            with pytest.raises(ValueError, match="field_sizes: an abs_error of"):
                drv(d, e)
        for errs in ([], [1e-3], [1e-3] * 3, (1e-3,)):
            with pytest.raises(ValueError, match="field_sizes: abs_error is a float or a list with one float per tensor"):
                drv([f, d], errs)
        for cands in ([()], [(1,), ()], [[(1,)], [()]]):
            with pytest.raises(ValueError, match="field_sizes: a candidate is a non-empty tuple of lags"):
                drv([f, d], 1e-3, candidates=cands)
        for cands in ([1], [(1,), 6], [None]):
            with pytest.raises(ValueError, match="field_sizes: a candidate is a (non-empty )?tuple of lags"):
                drv(f, 1e-3, candidates=cands)
        for cands in ([(0,)], [(2.0,)], [(1 << 64,)], [(3, 3)], [(5, 2)], [(1, 2, 3, 4)]):
            with pytest.raises(ValueError, match="field_sizes: (a lag is|lags are)"):
                drv(f, 1e-3, candidates=cands)
        for cands in ([[(1,)]], [[(1,)]] * 3):
            with pytest.raises(ValueError, match="field_sizes: candidates is a list of tuples or a list with one such list per tensor"):
                drv([f, d], 1e-3, candidates=cands)
        for cands in ([], (), "x", 5):
            with pytest.raises(ValueError, match="field_sizes: candidates are a non-empty list of tuples of lags"):
                drv(f, 1e-3, candidates=cands)
        with pytest.raises(ValueError, match="field_sizes: axis 2 of a tensor of 2 dimensions"):
            drv(f, 1e-3, axes=(0, 2))
    # the default candidates: the non-empty subsets of the axis lags, at most seven
    assert fields._field_candidates("test", [f], None, None) == [[(1,), (6,), (1, 6)]]
    g = _FakeCuda(torch.zeros(2, 3, 4, 5, dtype=torch.float64))
    assert fields._field_candidates("test", [g], None, None) == [[(1,), (5,), (20,), (1, 5), (1, 20), (5, 20), (1, 5, 20)]]
    assert fields._field_candidates("test", [f, g], None, [(2,), (1, 7)]) == [[(2,), (1, 7)]] * 2
    # field_histograms
    for bad in (None, b"abc", [cpu]):
        with pytest.raises(ValueError, match="field_histograms: a contiguous CUDA tensor"):
            fields.field_histograms(bad, 1e-3, [(1,)])
    with pytest.raises(ValueError, match="field_histograms: contiguous CUDA tensors"):
        fields.field_histograms(cpu, 1e-3, [(1,)])
    with pytest.raises(ValueError, match="field_histograms: float32 and float64 tensors"):
        fields.field_histograms(_FakeCuda(torch.zeros(8, dtype=torch.int32)), 1e-3, [(1,)])
    for sets in (None, 5, "ab"):
        with pytest.raises(ValueError, match="field_histograms: lag_sets is a list of tuples of lags"):
            fields.field_histograms(f, 1e-3, sets)
    for sets in ([()], [(1,), ()], [1], [[1]], [None]):
        with pytest.raises(ValueError, match="field_histograms: a candidate is a non-empty tuple of lags"):
            fields.field_histograms(f, 1e-3, sets)
    for sets in ([(0,)], [(3, 3)], [(1, 2, 3, 4)]):
        with pytest.raises(ValueError, match="field_histograms: (lags are|a lag is)"):
            fields.field_histograms(f, 1e-3, sets)
    for e in bad_bounds:
        with pytest.raises(ValueError, match="field_histograms: (abs_error is|an abs_error of)"):
            fields.field_histograms(f, e, [(1,), (6,)])
        with pytest.raises(ValueError, match="field_histograms: (abs_error is|an abs_error of)"):
            fields.field_histograms(f, [1e-3, e], [(1,), (1,)])
    for errs in ([], [1e-3], [1e-3] * 3):
        with pytest.raises(ValueError, match="field_histograms: abs_error is a float or a list with one float per entry"):
            fields.field_histograms(f, errs, [(1,), (6,)])
    # field_rates and fit_abs_error
    for name, drv in (("field_rates", lambda t, e, **kw: fields.field_rates(t, e, **kw)),
                      ("fit_abs_error", lambda t, e, **kw: fields.fit_abs_error(t, 1000, e, **kw))):
        for bad in (None, b"abc", [f]):
            with pytest.raises(ValueError, match=f"{name}: a contiguous CUDA tensor"):
                drv(bad, [1e-3])
        with pytest.raises(ValueError, match=f"{name}: contiguous CUDA tensors"):
            drv(cpu, [1e-3])
        with pytest.raises(ValueError, match=f"{name}: float32 and float64 tensors"):
            drv(_FakeCuda(torch.zeros(8, dtype=torch.int16)), [1e-3])
        for errs in ([], (), None, 1e-3, "ab"):
            with pytest.raises(ValueError, match=f"{name}: abs_errors is a non-empty list of floats"):
                drv(f, errs)
        for e in bad_bounds:
            with pytest.raises(ValueError, match=f"{name}: (abs_error is|an abs_error of)"):
                drv(f, [1e-3, e])
        with pytest.raises(ValueError, match=f"{name}: lags are strictly increasing"):
            drv(f, [1e-3], lags=(6, 1))
        with pytest.raises(ValueError, match=f"{name}: axis 2 of a tensor of 2 dimensions"):
            drv(f, [1e-3], axes=(0, 2))
    for mb in (-1, 1.5, None, "9", True, [5]):
        with pytest.raises(ValueError, match="fit_abs_error: max_bytes is an int >= 0"):
            fields.fit_abs_error(f, mb, [1e-3])
    with pytest.raises(ValueError, match="fit_abs_error: max_bytes is an int >= 0"):
        fields.fit_abs_error(None, -1, [])                                  # in front of everything else


# ---------------------------------------------------------------- the model, which tests/test_gpu_field_hist.py leans on
def field_model(shafa, fields, x, abs_error, lags):
    """field_sizes' model in numpy for the flat float array x: codes -> Lorenzo differences -> fold -> np.bincount -> the host's
    Module T sizes.  Returns (the planes' histograms [k, 256], outliers, nbytes)"""
    k = x.dtype.itemsize
    step, bound = fields._params("test", abs_error, k)
    code, _, good = model(x, step, bound)
    h = plane_histograms(code.view(UINT[k]), lags)
    outliers = int((~good).sum())
    return h, outliers, sum(min(x.size, sf_bytes(shafa, r)) for r in h) + (8 + k) * outliers


def field_model_sizes(shafa, fields, x, abs_error, cands):
    """field_sizes' list for the flat float array x, sorted by its rule"""
    out = [(c,) + field_model(shafa, fields, x, abs_error, c)[:0:-1] for c in cands]
    return sorted(out, key=lambda e: (e[2] > fields.outlier_capacity(x.size), e[1], len(e[0]), e[0]))


def planted(k, value=np.nan):
    """DESIGN 7.28's field as floats with `value` where tests/test_gpu_fields.py plants its three NaNs"""
    x = the_float_field(k).reshape(-1).copy()
    x[[0, 70000, x.size - 1]] = value
    return x


@pytest.mark.parametrize("k", (4, 8))
def test_the_model_checks_itself(shafa, fields, k):
    """on the field at 10^-1 the outliers are the three planted NaNs, far below the capacity; every plane's counts sum to numel;
    a NaN's code is 0, so against the field with 0.0 in the NaNs' places the planes are the same and nbytes grows by exactly
    8 + elem per NaN"""
    x, clean = planted(k), planted(k, 0.0)
    import torch
    shaped = _FakeCuda(torch.zeros(32, 64, 64, dtype=torch.float32 if k == 4 else torch.float64))
    cands = fields._field_candidates("test", [shaped], None, None)[0]       # field_sizes' default: no (), at most seven
    assert cands == [(1,), (64,), (4096,), (1, 64), (1, 4096), (64, 4096), (1, 64, 4096)]
    assert fields.outlier_capacity(x.size) == 16 + 131072 // 64
    got, ref = field_model_sizes(shafa, fields, x, 1e-1, cands), field_model_sizes(shafa, fields, clean, 1e-1, cands)
    assert [e[0] for e in got] == [e[0] for e in ref] and sorted(e[0] for e in got) == sorted(cands)
    for (c, nb, no), (_, nb0, no0) in zip(got, ref):
        assert (no, no0) == (3, 0) and nb == nb0 + 3 * (8 + k), c
        h, _, _ = field_model(shafa, fields, x, 1e-1, c)
        assert h.shape == (k, 256) and h.sum(1).tolist() == [x.size] * k, c
        assert h.tolist() == field_model(shafa, fields, clean, 1e-1, c)[0].tolist()
    assert all(a[1] <= b[1] for a, b in zip(got, got[1:]))                  # no candidate is past the capacity: sorted by nbytes
    assert got[0][1] < x.size * k // 4                                      # and under the bound the field shrinks to a fraction
    # a candidate past the capacity sorts last, whatever its bytes: noise at a bound nothing resolves
    noise = np.random.default_rng(k).standard_normal(6400).astype(x.dtype)
    got = field_model_sizes(shafa, fields, noise, 1e-30, [(1,), (2,)])
    assert [e[2] for e in got] == [6400, 6400] and [e[0] for e in got] == [(1,), (2,)]
    mixed = sorted([((1,), 10, 117), ((2,), 500, 116), ((3,), 20, 0)], key=lambda e: (e[2] > fields.outlier_capacity(6400), e[1]))
    assert [e[0] for e in mixed] == [(3,), (2,), (1,)]

"""CPU-side checks of the error-bounded fields (shafa_hipd_split_planes_grid_quant_dev / shafa_hipd_merge_planes_grid_quant_dev,
csrc/planes_lag.hip) and of the drivers on top (shafa-cd_amd/fields.py): declared, exported, bound, the ABI version, the header's
section in its place, the submodule's names re-exported and its own, every argument error refused before HIP is touched and in
the grid split's order with the entries' own where that checks its lags, the drivers' ValueErrors before a device is touched, and
the numpy model of the transform (include/shafa_hip.h: "Error-bounded fields") on DESIGN 7.28's field: no outliers at |x|max /
abs_error = 10^4 and 10^5, the bound in exact arithmetic, and what is an outlier by rule (no GPU needed)."""
import ctypes as C
import fractions
import math
import os

import numpy as np
import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64
from test_planes_lag_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAMES = ("shafa_hipd_split_planes_grid_quant_dev", "shafa_hipd_merge_planes_grid_quant_dev")
FLOAT = {4: np.float32, 8: np.float64}
INT = {4: np.int32, 8: np.int64}


@pytest.fixture(scope="module")
def fields(shafa):
    return pkgload.load_submodule("fields")


def _f64(*v):
    return (C.c_double * len(v))(*v)


def test_declared_exported_and_bound(shafa, fields):
    declared = declared_symbols(HEADER)
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert getattr(shafa.lib(), name).restype is C.c_int and getattr(shafa.lib(), name).argtypes, name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_grid_quant_dev", "merge_planes_grid_quant_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("quantize_field", "restore_field", "compress_fields", "decompress_fields"):
        assert callable(getattr(fields, name, None)), name
        assert getattr(shafa, name) is getattr(fields, name), name          # re-exported, and the submodule's own
        assert getattr(fields, name).__module__ == fields.__name__
    assert shafa.FIELD_SLACK == fields.FIELD_SLACK == 2.0 ** -7
    assert isinstance(fields.CompressedField, type) and shafa.CompressedField is fields.CompressedField
    assert fields.CompressedField.__module__ == fields.__name__
    assert fields.CompressedField.__slots__ == ("dtype", "shape", "lags", "abs_error", "step", "bound", "planes", "outlier_pos",
                                                "outlier_bits", "nbytes")
    with open(HEADER) as f:
        text = f.read()
    assert text.index("Plane histograms of Lorenzo differences") < text.index("shafa_hipd_hist_planes_grid_dev(") \
        < text.index("Error-bounded fields") < text.index(NAMES[0] + "(") < text.index(NAMES[1] + "(") < text.index("Byte columns")


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    """the grid split's checks in its order (tests/test_planes_grid_cpu.py) on the stand-in batch, then, where that entry checks
    its lags, these entries' own"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE
    TOP = (1 << 64) - 1

    def poffs(elem):
        return _u64(*[16 * i for i in range(3 * elem)])

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=4, nl=3, lags=_u64(1, 0, 0, 1, 7, TOP, 1 << 63, TOP, 0), step=_f64(0.5, 0.25, 3.0),
                 bound=_f64(0.25, 0.125, 2.0), d_el=A.p, off=_u64(0, 8, (1 << 40) + 24), cap=_u64(5, 100, 70000), d_n=A.p,
                 d_planes=A.p, poff=None, d_outl=A.p, ooff=_u64(0, 16, 17), ocnt=_u64(16, 1, 0), d_outl_n=A.p)
        a.update(kw)
        if a["poff"] is None:
            a["poff"] = poffs(a["elem"] if a["elem"] in (1, 2, 4, 8) else 8)
        if merge:
            return L.shafa_hipd_merge_planes_grid_quant_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["step"],
                                                            a["d_planes"], a["poff"], a["cap"], a["d_n"], a["d_outl"], a["ooff"],
                                                            a["ocnt"], a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_grid_quant_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["step"], a["bound"],
                                                        a["d_el"], a["off"], a["cap"], a["d_n"], a["d_planes"], a["poff"],
                                                        a["d_outl"], a["ooff"], a["ocnt"], a["d_outl_n"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    assert reached_hip(call()) and reached_hip(call(elem=8))
    assert reached_hip(call(nl=1, lags=_u64(1, 7, TOP)))
    assert reached_hip(call(d_outl=None, ocnt=_u64(0, 0, 0)))              # no records anywhere: no record buffer needed
    # 1. the device pointers, the element size and nlags, in front of nblocks
    for k in ("b", "d_el", "d_planes", "d_n"):
        for nb in (3, 0, -1, 0x7FFFFFFF):
            assert call(**{k: None}, nb=nb) == OM, (k, nb)
    for elem in (0, 1, 2, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):                   # floats and doubles only
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    for nl in (0, 4, 0xFFFFFFFF):
        assert call(nl=nl) == OM and call(nl=nl, nb=0) == OM and call(nl=nl, nb=0x7FFFFFFF) == OM, nl
    # 2. no block: success, no host array is looked at — these entries' own neither
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, lags=None, step=None, bound=None, ooff=None, ocnt=None, d_outl=None, d_outl_n=None) == OK
    # 3. past max_blocks
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF, cap=None, step=None) == LM
    # 4. the capacities, in front of everything of these entries' own
    assert call(cap=None) == OM and call(cap=None, step=None) == OM
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big) == LM and call(cap=_u64(TOP, 0, 0)) == LM
    for kw in (dict(step=None), dict(bound=None), dict(step=_f64(0.0, 0.5, 0.5)), dict(d_outl_n=None), dict(ooff=None), dict(ocnt=None),
               dict(d_outl=None), dict(lags=None), dict(off=None)):
        assert call(cap=big, **kw) == LM, kw
    # 5. the grid entries' host arrays, alignments and rows of lags
    assert call(off=None) == OM and call(d_planes=C.c_void_p(A.p.value + 8)) == OM
    assert call(off=_u64(0, 8, (1 << 40) + 26)) == OM and call(d_el=C.c_void_p(A.p.value + 2)) == OM
    assert call(lags=None) == OM and call(lags=_u64(1, 0, 0, 0, 1, 0, 1, 2, 3)) == OM and call(lags=_u64(1, 0, 0, 3, 3, 0, 1, 2, 3)) == OM
    # 6. these entries' own: NULL arrays
    assert call(step=None) == OM
    if not merge:
        assert call(bound=None) == OM and call(d_outl_n=None) == OM
    assert call(ooff=None) == OM and call(ocnt=None) == OM
    assert call(d_outl=None) == OM                                          # a block has records
    assert call(d_outl=None, ocnt=_u64(0, 0, 1)) == OM and reached_hip(call(nb=2, d_outl=None, ocnt=_u64(0, 0, 1)))
    # 7. a bad step, bound or inverse, in every block's place
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
                if not merge:
                    assert call(elem=elem, bound=_f64(*s)) == OM, (elem, i, v)
            for v in ok[elem]:
                s = [0.5, 0.25, 3.0]
                s[i] = v
                assert reached_hip(call(elem=elem, step=_f64(*s))), (elem, i, v)
                if not merge:
                    assert reached_hip(call(elem=elem, bound=_f64(*s))), (elem, i, v)
        assert reached_hip(call(elem=elem, nb=2, step=_f64(0.5, 0.25, 0.0), bound=_f64(0.5, 0.25, -1.0)))   # only the call's blocks


def test_drivers_refuse_bad_arguments_before_a_device(shafa, fields, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(64, dtype=torch.float32)
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.float32))
    d = _FakeCuda(torch.zeros(4, 6, dtype=torch.float64))
    for bad in (None, b"abc", 5, cpu, [cpu], [None]):
        with pytest.raises(ValueError, match="compress_fields: "):
            fields.compress_fields(bad, 1e-3)
    for dt in (torch.int32, torch.bfloat16, torch.float16, torch.int64, torch.uint8):
        with pytest.raises(ValueError, match="compress_fields: float32 and float64 tensors"):
            fields.compress_fields([f, _FakeCuda(torch.zeros(8, dtype=dt))], 1e-3)
        with pytest.raises(ValueError, match="quantize_field: float32 and float64 tensors"):
            fields.quantize_field(_FakeCuda(torch.zeros(8, dtype=dt)), 1e-3, (1,))
    for e in (0, 0.0, -1e-3, math.nan, math.inf, None, "1e-3", True, 1e-46, 1e-40):
        with pytest.raises(ValueError, match="compress_fields: (abs_error is|an abs_error of)"):
            fields.compress_fields(f, e)
        with pytest.raises(ValueError, match="compress_fields: (abs_error is|an abs_error of)"):
            fields.compress_fields([d, f], [1e-3, e])
    for e in (0.0, math.nan, 1e-320, 5e-324):
        with pytest.raises(ValueError, match="compress_fields: (abs_error is|an abs_error of)"):
            fields.compress_fields(d, e)
    for errs in ([], [1e-3], [1e-3] * 3, (1e-3,)):
        with pytest.raises(ValueError, match="compress_fields: abs_error is a float or a list with one float per tensor"):
            fields.compress_fields([f, d], errs)
    assert fields.compress_fields([], 1e-3) == [] and fields.decompress_fields([]) == []
    with pytest.raises(ValueError, match="compress_fields: block_size"):
        fields.compress_fields(f, 1e-3, block_size=-1)
    with pytest.raises(ValueError, match="compress_fields: lags are strictly increasing"):
        fields.compress_fields(f, 1e-3, lags=(6, 1))
    with pytest.raises(ValueError, match="compress_fields: axis 2 of a tensor of 2 dimensions"):
        fields.compress_fields(f, 1e-3, axes=(0, 2))
    raw = torch.zeros(24, dtype=torch.uint8)
    none = torch.zeros(0, dtype=torch.int64)
    cg = shafa.CompressedGrid(torch.float32, (4, 6), (1, 6), [raw] * 4, 96)
    for bad in (cg, [cg], None, 5, [None], shafa.CompressedTensor(torch.float32, (24,), [raw] * 4, 96)):
        with pytest.raises(ValueError, match="decompress_fields: a CompressedField or a list of them"):
            fields.decompress_fields(bad)
    CF = fields.CompressedField
    item = CF(torch.float32, (4, 6), (1, 6), 1e-3, 0.5, 0.25, [raw] * 4, none, none, 96)
    assert not hasattr(item, "__dict__") and repr(item).startswith("CompressedField(torch.float32, (4, 6), lags=(1, 6)")
    with pytest.raises(ValueError, match="decompress_grids: a CompressedGrid or a list of them"):
        shafa.decompress_grids([item])
    for step in (0.1, -0.5, math.nan, math.inf, 1e-46):
        with pytest.raises(ValueError, match="decompress_fields: step is"):
            fields.decompress_fields(CF(torch.float32, (4, 6), (1, 6), 1e-3, step, 0.25, [raw] * 4, none, none, 96))
    with pytest.raises(ValueError, match="decompress_fields: (lags are|a lag is)"):
        fields.decompress_fields(CF(torch.float32, (4, 6), (6, 1), 1e-3, 0.5, 0.25, [raw] * 4, none, none, 96))
    with pytest.raises(ValueError, match="decompress_fields: float32 and float64 tensors"):
        fields.decompress_fields(CF(torch.int32, (4, 6), (1, 6), 1e-3, 0.5, 0.25, [raw] * 4, none, none, 96))
    with pytest.raises(ValueError, match="decompress_fields: one position and one bit pattern per outlier"):
        fields.decompress_fields(CF(torch.float32, (4, 6), (1, 6), 1e-3, 0.5, 0.25, [raw] * 4, none, torch.zeros(1, dtype=torch.int64), 96))
    with pytest.raises(ValueError, match="decompress_fields: planes are CUDA tensors"):
        fields.decompress_fields(item)


def test_step_and_bound_of_an_abs_error(fields):
    """step = 2 abs_error (1 - FIELD_SLACK) and bound = abs_error, each the largest value of the element type that is not above"""
    F = fractions.Fraction
    for k in (4, 8):
        T = FLOAT[k]
        for e in (1e-3, 0.1, 1.0, 0.75, 1e-30, 123.456, 2.0 ** -20, 1e30):
            step, bound = fields._params("test", e, k)
            for got, want in ((step, 2 * F(e) * (1 - F(2) ** -7)), (bound, F(e))):
                assert float(T(got)) == got and F(got) <= want < F(float(np.nextafter(T(got), T(np.inf)))), (k, e)
            assert fields._inverse(step, k) == float(T(1.0 / step))
    assert fields.outlier_capacity(0) == 16 and fields.outlier_capacity(6400) == 116


# ---------------------------------------------------------------- the numpy model of the rule
def model(x, step, bound):
    """include/shafa_hip.h, "Error-bounded fields", in numpy: x a float32 or float64 array, step and bound Python floats exactly
    representable in its type -> (codes as signed integers, x' = T(code) * step, good).  Every operation is one numpy operation
    in T, so one IEEE operation rounded to nearest even."""
    k = x.dtype.itemsize
    T = x.dtype.type
    inv = T(1.0 / step)
    with np.errstate(all="ignore"):
        t = x * inv
        inside = np.abs(t) < T(2.0 ** (8 * k - 2))
        code = np.where(inside, np.rint(t), T(0)).astype(INT[k])
        xr = code.astype(T) * T(step)
        if k == 4:
            good = inside & (np.abs(x.astype(np.float64) - xr.astype(np.float64)) <= np.float64(bound))
        else:
            good = inside & (np.abs(x - xr) <= T(bound))
    return code, xr, good


def the_float_field(k):
    """DESIGN 7.28's [32, 64, 64] field as floats: 1000 sin(x / 9) cos(y / 13) sin(z / 7 + 0.3)"""
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.float64)
    return (1000 * np.sin(x / 9) * np.cos(y / 13) * np.sin(z / 7 + 0.3)).astype(FLOAT[k])


@pytest.mark.parametrize("k", (4, 8))
def test_the_model_on_the_field(fields, k):
    x = the_float_field(k).reshape(-1)
    assert x.size == 131072
    top = float(np.abs(x).max())
    rng = np.random.default_rng(k)
    for ratio in (1e4, 1e5):
        step, bound = fields._params("test", top / ratio, k)
        code, xr, good = model(x, step, bound)
        assert int((~good).sum()) == 0, (k, ratio, int((~good).sum()))
        assert np.abs(code).max() > ratio / 4
        # every good element of a sample is within the bound in EXACT arithmetic
        for i in rng.choice(x.size, 4096, replace=False):
            assert abs(fractions.Fraction(float(x[i])) - fractions.Fraction(float(xr[i]))) <= fractions.Fraction(bound), (k, ratio, i)
    # at 10^6 float32's own rounding of x' reaches the bound: outliers appear, fewer with the slack than with step = 2 bound,
    # and few enough for compress_fields' capacity
    if k == 4:
        b = float(np.float32(top / 1e6))
        plain, slack = (int((~model(x, *p)[2]).sum()) for p in ((2 * b, b), fields._params("test", top / 1e6, k)))
        assert slack < plain and slack <= fields.outlier_capacity(x.size), (plain, slack)


@pytest.mark.parametrize("k", (4, 8))
def test_what_is_an_outlier(k):
    T = FLOAT[k]
    step, bound = 0.25, 0.125
    below = float(np.nextafter(T(2.0 ** (8 * k - 2)), T(0)))                 # the largest t inside the code range
    x = np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, -0.0, 0.0, 0.3, below * step, 2.0 ** (8 * k - 4)], T)
    code, xr, good = model(x, step, bound)
    assert good.tolist() == [False] * 5 + [True] * 4 + [False]
    assert code[:5].tolist() == [0] * 5 and code[9] == 0                      # no code: 0 goes into the planes
    assert xr[5] == 0 and not np.signbit(xr[5])                              # -0.0 is good and restores as +0.0
    assert code[7] == 1 and xr[7] == 0.25 and code[8] == int(below) and xr[8] == x[8]
    # a value whose restored value misses the bound is an outlier although it has a code
    code, xr, good = model(np.array([0.3], T), 0.25, 2.0 ** -5)
    assert code.tolist() == [1] and not good[0]

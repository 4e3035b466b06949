"""CPU-side checks of the error statistics (shafa_hipd_error_dev, shafa_hipd_error_quant_dev, shafa_hipd_error_round_dev,
csrc/planes_lag.hip) and of the drivers on top (shafa-cd_amd/quality.py): declared, exported, bound, the ABI version, the header's
section in its place, the submodule's names re-exported and its own, ErrorStats from hand-made words, every argument error refused
before HIP is touched in the stated order, the drivers' ValueErrors before a device is touched, and a numpy model of the record
(include/shafa_hip.h: "Error statistics") over the quantising and the rounding models on DESIGN 7.28's field (no GPU needed)."""
import ctypes as C
import fractions
import math
import os
import struct

import numpy as np
import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64
from test_planes_lag_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAMES = ("shafa_hipd_error_dev", "shafa_hipd_error_quant_dev", "shafa_hipd_error_round_dev")
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
INT = {4: np.int32, 8: np.int64}
FORMATS = {"float16": (2, 10), "bfloat16": (2, 7), "float32": (4, 23), "float64": (8, 52)}
NONE = (1 << 64) - 1
PINF, NINF = 0x7FF0000000000000, 0xFFF0000000000000


@pytest.fixture(scope="module")
def quality(shafa):
    return pkgload.load_submodule("quality")


def _u32(*v):
    return (C.c_uint32 * len(v))(*v)


def _f64(*v):
    return (C.c_double * len(v))(*v)


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def test_declared_exported_and_bound(shafa, quality):
    declared = declared_symbols(HEADER)
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert getattr(shafa.lib(), name).restype is C.c_int and getattr(shafa.lib(), name).argtypes, name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("error_dev", "error_quant_dev", "error_round_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("tensor_errors", "field_errors", "rounded_errors", "field_curve", "rounded_curve", "fit_psnr", "fit_keep_bits_snr",
                 "verify_fields", "verify_rounded"):
        assert callable(getattr(quality, name, None)), name
        assert getattr(shafa, name) is getattr(quality, name), name           # re-exported, and the submodule's own
        assert getattr(quality, name).__module__ == quality.__name__
    assert shafa.ErrorStats is quality.ErrorStats and quality.ErrorStats.__module__ == quality.__name__
    assert shafa.ERR_WORDS == quality.ERR_WORDS == 12
    with open(HEADER) as f:
        text = f.read()
    assert "#define SHAFA_ERR_WORDS 12" in text
    assert text.index("Point-wise relative bounds") < text.index("shafa_hipd_hist_planes_grid_round_dev(") \
        < text.index("Error statistics") < text.index(NAMES[0] + "(") < text.index(NAMES[1] + "(") < text.index(NAMES[2] + "(") \
        < text.index("Byte columns")


def test_error_stats_from_hand_made_words(quality):
    E = quality.ErrorStats
    assert E.__slots__ == ("n", "finite", "others", "others_changed", "outliers", "over", "sum_e2", "sum_x2", "max_e", "max_at",
                           "min_x", "max_x")
    s = E([10, 8, 2, 1, 3, 4, _bits(2.0), _bits(800.0), _bits(1.0), 7, _bits(-5.0), _bits(15.0)])
    assert not hasattr(s, "__dict__")
    assert (s.n, s.finite, s.others, s.others_changed, s.outliers, s.over) == (10, 8, 2, 1, 3, 4)
    assert (s.sum_e2, s.sum_x2, s.max_e, s.max_at, s.min_x, s.max_x) == (2.0, 800.0, 1.0, 7, -5.0, 15.0)
    assert s.mse == 0.25 and s.rmse == 0.5 and s.value_range == 20.0 and s.nrmse == 0.025
    assert s.psnr == pytest.approx(20 * math.log10(20.0) - 10 * math.log10(0.25), rel=1e-15)
    assert s.snr == pytest.approx(10 * math.log10(400.0), rel=1e-15)
    assert s.max_error == 1.0 and s.argmax == 7
    assert s.words() == [10, 8, 2, 1, 3, 4, _bits(2.0), _bits(800.0), _bits(1.0), 7, _bits(-5.0), _bits(15.0)]
    assert repr(s).startswith("ErrorStats(n=10, finite=8")
    # signed int64 words, as a tensor's tolist gives them
    t = E([10, 8, 2, 1, 3, 4, _bits(2.0), _bits(800.0), _bits(1.0), 7, _bits(-5.0) - (1 << 64), _bits(15.0)])
    assert t.min_x == -5.0
    # mse 0: inf
    z = E([4, 4, 0, 0, 0, 0, 0, _bits(30.0), 0, 0, _bits(1.0), _bits(4.0)])
    assert z.mse == 0.0 and z.rmse == 0.0 and z.psnr == math.inf and z.snr == math.inf and z.nrmse == 0.0 and z.argmax == 0
    # no finite element: nan
    e = E([3, 0, 3, 0, 3, 0, 0, 0, 0, NONE, PINF, NINF])
    for v in (e.mse, e.rmse, e.value_range, e.nrmse, e.psnr, e.snr):
        assert math.isnan(v)
    assert e.argmax is None and e.max_error == 0.0 and e.min_x == math.inf and e.max_x == -math.inf
    # a range of 0: nan, but the SNR stands
    c = E([2, 2, 0, 0, 0, 0, _bits(0.5), _bits(8.0), _bits(0.5), 0, _bits(2.0), _bits(2.0)])
    assert math.isnan(c.psnr) and math.isnan(c.nrmse) and c.snr == pytest.approx(10 * math.log10(16.0))
    for bad in ([], [0] * 11, [0] * 13):
        with pytest.raises(ValueError, match="ErrorStats: a record of 12 words"):
            E(bad)


@pytest.mark.parametrize("entry", ["pair", "quant", "round"])
def test_argument_errors_before_hip(shafa, entry):
    """the stated order (include/shafa_hip.h: "Error statistics"): the fused entries follow the corresponding hist entry for the
    arguments they share, shafa_hipd_error_dev follows shafa_hipd_compare_dev on side a; then the entry's own"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE
    TOP = (1 << 64) - 1
    MANT = {2: 7, 4: 23, 8: 52}
    pair, quant = entry == "pair", entry == "quant"
    inf = math.inf

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=4, mant=None, keep=_u32(0, 3, 7), step=_f64(0.5, 0.25, 2.0), bound=_f64(0.25, 0.125, 1.0),
                 abs=_f64(0.0, 1.5, inf), rel=_f64(0.0, 0.0625, 1e300), d_el=A.p, off=_u64(0, 16, (1 << 40) + 32),
                 cap=_u64(5, 100, 70000), d_n=A.p, d_ref=C.c_void_p(A.p.value + 8), roff=_u64(0, 8, (1 << 40) + 24), d_stat=A.p)
        a.update(kw)
        e = a["elem"] if a["elem"] in (2, 4, 8) else 8
        if a["mant"] is None:
            a["mant"] = _u32(*[MANT[e]] * 3)
        elif a["mant"] == "null":
            a["mant"] = None
        if pair:
            return L.shafa_hipd_error_dev(a["b"], None, a["nb"], a["elem"], a["mant"], a["abs"], a["rel"], a["d_el"], a["off"],
                                          a["cap"], a["d_n"], a["d_ref"], a["roff"], a["d_stat"])
        if quant:
            return L.shafa_hipd_error_quant_dev(a["b"], None, a["nb"], a["elem"], a["step"], a["bound"], a["d_el"], a["off"], a["cap"],
                                                a["d_n"], a["d_stat"])
        return L.shafa_hipd_error_round_dev(a["b"], None, a["nb"], a["elem"], a["mant"], a["keep"], a["d_el"], a["off"], a["cap"],
                                            a["d_n"], a["d_stat"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    assert reached_hip(call()) and reached_hip(call(elem=8))
    if not quant:
        assert reached_hip(call(elem=2)) and reached_hip(call(elem=2, mant=_u32(7, 10, 7), keep=_u32(7, 10, 0)))
    # 1. the device pointers and the element size, in front of nblocks
    for k in ("b", "d_el", "d_n") + (("d_ref",) if pair else ()):
        for nb in (3, 0, -1, 0x7FFFFFFF):
            assert call(**{k: None}, nb=nb) == OM, (k, nb)
    for elem in (0, 1, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF) + ((2,) if quant else ()):       # elem 2: refused by the quant entry
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    if pair:                                                                # side a is a decoder's output: 16-aligned
        for nb in (3, 0, 0x7FFFFFFF):
            assert call(d_el=C.c_void_p(A.p.value + 8), nb=nb) == OM and call(d_el=A.odd, nb=nb) == OM
    # 2. no block: success, no host array is looked at — these entries' own neither
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, mant="null", keep=None, step=None, bound=None, abs=None, rel=None, roff=None, d_stat=None) == OK
    # 3. past max_blocks
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF, cap=None, mant="null", step=None, d_stat=None) == LM
    # 4. the capacities, in front of everything of these entries' own
    assert call(cap=None) == OM and call(cap=None, d_stat=None) == OM
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big) == LM and call(cap=_u64(TOP, 0, 0)) == LM and call(cap=_u64(TOP // 4, TOP // 4, TOP // 4)) == LM
    own = (dict(mant="null"), dict(keep=None), dict(step=None), dict(bound=None), dict(abs=None), dict(rel=None), dict(d_stat=None),
           dict(abs=_f64(-1.0, 0, 0)), dict(rel=_f64(inf, 0, 0)), dict(step=_f64(0.0, 1, 1)), dict(keep=_u32(99, 0, 0)))
    for kw in own + (() if pair else (dict(off=None),)) + ((dict(roff=None),) if pair else ()):
        assert call(cap=big, **kw) == LM, kw
    # 5. the host arrays and the alignments
    assert call(off=None) == OM and call(off=None, d_stat=None) == OM
    if pair:
        assert call(off=None, cap=None) == OM
        for bad in (_u64(1, 16, 4096), _u64(0, 24, 4096), _u64(0, 16, 4100)):
            assert call(off=bad) == OM
        assert call(off=_u64(0, 24, 4096), cap=big) == OM                  # compare_dev's order: side a's offsets first
        assert call(roff=None) == OM and call(roff=_u64(0, 8, 26)) == OM and call(d_ref=C.c_void_p(A.p.value + 2)) == OM
        assert call(elem=8, roff=_u64(0, 8, 28)) == OM and call(elem=8, d_ref=C.c_void_p(A.p.value + 4)) == OM
        assert reached_hip(call(d_ref=C.c_void_p(A.p.value + 4), roff=_u64(0, 4, 28)))
        assert reached_hip(call(elem=2, d_ref=C.c_void_p(A.p.value + 2), roff=_u64(0, 2, (1 << 40) + 6)))
        assert call(elem=2, d_ref=C.c_void_p(A.p.value + 1)) == OM and call(elem=2, roff=_u64(0, 3, 6)) == OM
    else:
        assert call(off=_u64(0, 8, (1 << 40) + 26)) == OM and call(d_el=C.c_void_p(A.p.value + 2)) == OM
        assert reached_hip(call(off=_u64(0, 4, (1 << 40) + 28), d_el=C.c_void_p(A.p.value + 4)))
        if not quant:
            assert call(elem=2, off=_u64(0, 8, (1 << 40) + 25)) == OM and call(elem=2, d_el=C.c_void_p(A.p.value + 1)) == OM
            assert reached_hip(call(elem=2, off=_u64(0, 2, (1 << 40) + 26), d_el=C.c_void_p(A.p.value + 2)))
    # 6. the rule's parameters, through the checks the existing entries share
    legal = {2: (7, 10), 4: (23,), 8: (52,)}
    if quant:
        assert call(step=None) == OM and call(bound=None) == OM
        for i in range(3):
            for bad in (0.0, -1.0, inf, -inf, math.nan, 1e-310, 5e-324):
                for which in ("step", "bound"):
                    v = [0.5, 0.25, 2.0]
                    v[i] = bad
                    assert call(**{which: _f64(*v)}) == OM and call(elem=8, **{which: _f64(*v)}) == OM, (i, bad, which)
            v = [0.5, 0.25, 2.0]
            v[i] = 0.1                                                     # not a float32
            assert call(step=_f64(*v)) == OM and call(bound=_f64(*v)) == OM
            assert reached_hip(call(elem=8, step=_f64(*v))) and reached_hip(call(elem=8, bound=_f64(*v)))
            v[i] = 1e-40                                                   # a float32 denormal; fine in double
            assert call(step=_f64(*v)) == OM and reached_hip(call(elem=8, bound=_f64(*v)))
        assert call(step=None, d_stat=None) == OM
        assert reached_hip(call(nb=2, step=_f64(0.5, 0.25, 0.0), bound=_f64(0.25, 0.125, -1.0)))       # only the call's blocks
    else:
        assert call(mant="null") == OM
        if not pair:
            assert call(keep=None) == OM
        for elem in (2, 4, 8):
            for i in range(3):
                for m in list(range(0, 70)) + [0xFFFFFFFF]:
                    mt = [legal[elem][0]] * 3
                    mt[i] = m
                    rc = call(elem=elem, mant=_u32(*mt), keep=_u32(0, 0, 0), d_ref=A.p)
                    assert reached_hip(rc) if m in legal[elem] else rc == OM, (elem, i, m)
                if pair:
                    continue
                for m in legal[elem]:
                    for keep, ok in ((0, True), (m // 2, True), (m, True), (m + 1, False), (0xFFFFFFFF, False)):
                        mt, kp = [legal[elem][0]] * 3, [0, 0, 0]
                        mt[i], kp[i] = m, keep
                        rc = call(elem=elem, mant=_u32(*mt), keep=_u32(*kp))
                        assert reached_hip(rc) if ok else rc == OM, (elem, i, m, keep)
            m = legal[elem][0]
            assert reached_hip(call(elem=elem, nb=2, mant=_u32(m, m, 99), keep=_u32(0, 0, 99), d_ref=A.p))
    # 7. the entry's own: d_stat, then the two bounds in every block's place
    assert call(d_stat=None) == OM
    if pair:
        assert call(abs=None) == OM and call(rel=None) == OM and call(abs=None, mant=_u32(23, 7, 23)) == OM
        for i in range(3):
            for bad, ok in ((-1.0, False), (-5e-324, False), (math.nan, False), (-inf, False), (inf, True), (0.0, True), (-0.0, True),
                            (5e-324, True), (1e308, True)):
                v = [0.0, 1.5, inf]
                v[i] = bad
                rc = call(abs=_f64(*v))
                assert reached_hip(rc) if ok else rc == OM, ("abs", i, bad)
            for bad, ok in ((-1.0, False), (-5e-324, False), (math.nan, False), (-inf, False), (inf, False), (0.0, True), (-0.0, True),
                            (5e-324, True), (1e308, True)):
                v = [0.0, 0.0625, 1e300]
                v[i] = bad
                rc = call(rel=_f64(*v))
                assert reached_hip(rc) if ok else rc == OM, ("rel", i, bad)
        assert reached_hip(call(nb=2, abs=_f64(0, 0, -1.0), rel=_f64(0, 0, inf)))      # only the call's blocks


def test_drivers_refuse_bad_arguments_before_a_device(shafa, quality, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    Q = quality
    cpu = torch.zeros(64, dtype=torch.float32)
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.float32))
    f2 = _FakeCuda(torch.zeros(4, 6, dtype=torch.float32))
    d = _FakeCuda(torch.zeros(4, 6, dtype=torch.float64))
    h = _FakeCuda(torch.zeros(4, 6, dtype=torch.float16))
    b = _FakeCuda(torch.zeros(4, 6, dtype=torch.bfloat16))
    i32 = _FakeCuda(torch.zeros(4, 6, dtype=torch.int32))
    # tensor_errors: the pairs
    for bad in (None, b"abc", 5, cpu, [cpu], [None]):
        with pytest.raises(ValueError, match="tensor_errors: "):
            Q.tensor_errors(bad, bad)
    with pytest.raises(ValueError, match="tensor_errors: one pair of tensors or two lists of equal length"):
        Q.tensor_errors(f, [f2])
    with pytest.raises(ValueError, match="tensor_errors: one original per tensor"):
        Q.tensor_errors([f, f2], [f])
    with pytest.raises(ValueError, match="tensor_errors: float16, bfloat16, float32 and float64 tensors"):
        Q.tensor_errors(i32, i32)
    with pytest.raises(ValueError, match="tensor_errors: torch.float32 .* against an original of torch.float64"):
        Q.tensor_errors(f, d)
    with pytest.raises(ValueError, match="tensor_errors: torch.float32 .* against an original of torch.float32"):
        Q.tensor_errors(f, _FakeCuda(torch.zeros(6, 4, dtype=torch.float32)))
    for bad in (-1.0, math.nan, -math.inf, True, None, "1"):
        with pytest.raises(ValueError, match="tensor_errors: abs_bound is a float >= 0 or inf"):
            Q.tensor_errors(f, f2, abs_bound=bad)
        with pytest.raises(ValueError, match="tensor_errors: abs_bound is a float >= 0 or inf"):
            Q.tensor_errors([f, h], [f2, h], abs_bound=[1.0, bad])
    for bad in (-1.0, math.nan, math.inf, True, None, "1"):
        with pytest.raises(ValueError, match="tensor_errors: rel_bound is a finite float >= 0"):
            Q.tensor_errors(f, f2, rel_bound=bad)
    with pytest.raises(ValueError, match="tensor_errors: abs_bound is a float or a list with one float per tensor"):
        Q.tensor_errors([f, h], [f2, h], abs_bound=[1.0])
    with pytest.raises(ValueError, match="tensor_errors: rel_bound is a float or a list with one float per tensor"):
        Q.tensor_errors(f, f2, rel_bound=[1.0, 2.0])
    assert Q.tensor_errors([], []) == []
    # the fused drivers
    for fn in (Q.field_errors, Q.field_curve):
        name = fn.__name__ if fn is Q.field_errors else "field_rates"
        for bad in (None, 5, [f], cpu):
            with pytest.raises(ValueError, match=f"{name}: "):
                fn(bad, [1e-3])
        for t in (h, b, i32):
            with pytest.raises(ValueError, match=f"{name}: float32 and float64 tensors"):
                fn(t, [1e-3])
        for errs in ([], 1e-3, None):
            with pytest.raises(ValueError, match=f"{name}: abs_errors is a non-empty list of floats"):
                fn(f, errs)
        for e in (0.0, -1.0, math.inf, math.nan, True, "1", 1e-60):
            with pytest.raises(ValueError, match=f"{name}: (an )?abs_error"):
                fn(f, [1e-3, e])
    with pytest.raises(ValueError, match="fit_psnr: min_psnr is a float in dB"):
        Q.fit_psnr(f, None, [1e-3])
    with pytest.raises(ValueError, match="fit_psnr: min_psnr is a float in dB"):
        Q.fit_psnr(f, math.nan, [1e-3])
    with pytest.raises(ValueError, match="field_errors: float32 and float64 tensors"):
        Q.fit_psnr(h, 60.0, [1e-3])
    with pytest.raises(ValueError, match="field_errors: abs_errors is a non-empty list"):
        Q.fit_psnr(f, 60.0, [])
    for fn in (Q.rounded_errors, Q.rounded_curve):
        for bad in (None, 5, [f], cpu):
            with pytest.raises(ValueError, match=f"{fn.__name__}: "):
                fn(bad, [3])
        with pytest.raises(ValueError, match=f"{fn.__name__}: float16, bfloat16, float32 and float64 tensors"):
            fn(i32, [3])
        for keeps in ([], 3, "abc"):
            with pytest.raises(ValueError, match=f"{fn.__name__}: keeps is a non-empty list of ints"):
                fn(f, keeps)
        for t, top in ((f, 23), (d, 52), (h, 10), (b, 7)):
            for keep in (True, None, 3.0, -1, top + 1):
                with pytest.raises(ValueError, match=f"{fn.__name__}: keep_bits is an int 0 .. {top}"):
                    fn(t, [0, keep])
    with pytest.raises(ValueError, match="fit_keep_bits_snr: min_snr is a float in dB"):
        Q.fit_keep_bits_snr(b, "40")
    with pytest.raises(ValueError, match="fit_keep_bits_snr: keep_bits is an int 0 .. 7"):
        Q.fit_keep_bits_snr(b, 40.0, [8])
    with pytest.raises(ValueError, match="fit_keep_bits_snr: float16, bfloat16, float32 and float64 tensors"):
        Q.fit_keep_bits_snr(i32, 40.0)
    # the verifiers
    raw = torch.zeros(24, dtype=torch.uint8)
    none = torch.zeros(0, dtype=torch.int64)
    cf = shafa.CompressedField(torch.float32, (4, 6), (1, 6), 1e-3, 0.5, 0.25, [raw] * 4, none, none, 96)
    cr = shafa.CompressedRounded(torch.float32, (4, 6), (1, 6), 10, [raw] * 4, none, none, 96)
    for bad in (None, 5, [None], cr, [cr], [cf, cr]):
        with pytest.raises(ValueError, match="verify_fields: a CompressedField or a list of them"):
            Q.verify_fields(bad, [f])
    for bad in (None, 5, [None], cf, [cf]):
        with pytest.raises(ValueError, match="verify_rounded: a CompressedRounded or a list of them"):
            Q.verify_rounded(bad, [f])
    for fn, it in ((Q.verify_fields, cf), (Q.verify_rounded, cr)):
        name = fn.__name__
        for orig in (None, [], [f, f2], 5):
            with pytest.raises(ValueError, match=f"{name}: one original per item"):
                fn([it], orig)
        with pytest.raises(ValueError, match=f"{name}: contiguous CUDA tensors"):
            fn([it], [cpu])
        with pytest.raises(ValueError, match=f"{name}: an item of torch.float32 .* against an original of torch.float64"):
            fn(it, d)
        with pytest.raises(ValueError, match=f"{name}: an item of torch.float32 .* against an original of torch.float32"):
            fn(it, _FakeCuda(torch.zeros(24, dtype=torch.float32)))
        assert fn([], []) == []
    with pytest.raises(ValueError, match="verify_fields: an item's bound is a finite float > 0"):
        Q.verify_fields(shafa.CompressedField(torch.float32, (4, 6), (1, 6), 1e-3, 0.5, math.nan, [raw] * 4, none, none, 96), f)
    with pytest.raises(ValueError, match="verify_rounded: keep_bits is an int 0 .. 23"):
        Q.verify_rounded(shafa.CompressedRounded(torch.float32, (4, 6), (1, 6), 24, [raw] * 4, none, none, 96), f)
    assert "2^53 of the smallest normal" in " ".join(Q.verify_rounded.__doc__.split())


# ---------------------------------------------------------------- the numpy models, written out again
def quant_model(x, step, bound):
    """include/shafa_hip.h, "Error-bounded fields": x a float32 or float64 array -> (x' = T(code) * step, good); one numpy
    operation in T each"""
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
    return xr, good


def round_model(x, mant, keep):
    """include/shafa_hip.h, "Point-wise relative bounds": x an array of bit patterns -> (x' as bits, good)"""
    U = x.dtype.type
    W = 8 * x.dtype.itemsize
    d = mant - keep
    MAG, INF, MIN = U((1 << (W - 1)) - 1), U(((1 << (W - 1 - mant)) - 1) << mant), U(1 << mant)
    S, M = x >> U(W - 1), x & MAG
    rn = M if d == 0 else (M + U((1 << (d - 1)) - 1) + ((M >> U(d)) & U(1))) >> U(d)
    R = np.where(M >= INF, M >> U(d), rn)
    back = (R << U(d)) & MAG
    good = np.where((M < MIN) | (M >= INF), back == M, back < INF)
    neg = S & (R != 0).astype(U)                                           # the sign of the code: -0.0 comes back as +0.0
    return (neg << U(W - 1)) | back, good


def as_double(bits, name):
    """D(.): the values of bit patterns of a format as doubles, exact"""
    if name == "bfloat16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return bits.view({"float16": np.float16, "float32": np.float32, "float64": np.float64}[name]).astype(np.float64)


def record(xb, yb, name, outliers, abs_b=math.inf, rel_b=0.0):
    """the record of include/shafa_hip.h, "Error statistics", for the bit patterns xb (the original) and yb (what came back);
    words 6 and 7 as Python floats summed by math.fsum, the others as the header has them"""
    x, y = as_double(xb, name), as_double(yb, name)
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(all="ignore"):
        e = np.abs(x - y)
        over = fin & (e > np.float64(abs_b) + np.float64(rel_b) * np.abs(x))
    ef, xf = e[fin], x[fin]
    emax = float(ef.max()) if ef.size else 0.0
    at = int(np.flatnonzero(fin & (e == emax))[0]) if ef.size else NONE
    zero = lambda v: 0.0 if v == 0 else v
    with np.errstate(over="ignore"):
        se2, sx2 = math.fsum((ef * ef).tolist()), math.fsum((xf * xf).tolist())
    return [xb.size, int(fin.sum()), int((~fin).sum()), int((~fin & (xb != yb)).sum()), outliers, int(over.sum()), se2, sx2,
            _bits(emax), at, _bits(zero(float(xf.min())) if xf.size else math.inf), _bits(zero(float(xf.max())) if xf.size else -math.inf)]


def the_field(name):
    """DESIGN 7.28's [32, 64, 64] field in a format, as bit patterns: 1000 sin(x / 9) cos(y / 13) sin(z / 7 + 0.3)"""
    import torch
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.float64)
    f = 1000 * np.sin(x / 9) * np.cos(y / 13) * np.sin(z / 7 + 0.3)
    k = FORMATS[name][0]
    t = torch.from_numpy(f).to(getattr(torch, name)).reshape(-1)
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[k]).numpy().view(UINT[k]).copy()


NAN_AT = (0, 70000, 131071)


def planted(name):
    """the field with three NaNs planted: the first element, one inside, the last"""
    k, mant = FORMATS[name]
    W = 8 * k
    x = the_field(name)
    inf = ((1 << (W - 1 - mant)) - 1) << mant
    for j, i in enumerate(NAN_AT):
        x[i] = UINT[k](inf | (1 << (mant - 1)) | (j << (W - 1) if j < 2 else 0))       # quiet NaNs, one of them negative
    return x


@pytest.mark.parametrize("name", ["float32", "float64"])
def test_the_record_under_the_quantising_model(shafa, quality, name):
    k, mant = FORMATS[name]
    xb = planted(name)
    x = xb.view({4: np.float32, 8: np.float64}[k])
    top = 1000.0
    for ratio in (1e3, 1e4, 1e5):
        step, bound = shafa.fields._params("test", top / ratio, k)
        xr, good = quant_model(x, step, bound)
        yb = np.where(good, xr.view(UINT[k]), xb)                          # an outlier comes back bit for bit
        r = record(xb, yb, name, int((~good).sum()))
        assert r[0] == 131072 and r[1] == 131069 and r[2] == 3 and r[3] == 0 and r[4] == 3 and r[5] == 0, (name, ratio, r[:6])
        emax = struct.unpack("<d", struct.pack("<Q", r[8]))[0]
        assert 0 < emax <= bound and r[9] not in NAN_AT
        s = quality.ErrorStats(r[:6] + [_bits(r[6]), _bits(r[7])] + r[8:])
        assert s.max_error == emax and s.argmax == r[9] and s.outliers == 3 and s.others == 3
        # uniform quantisation noise: the RMSE lies near step / sqrt(12), and PSNR and SNR follow from the sums
        assert 0.9 * step / math.sqrt(12) < s.rmse < 1.1 * step / math.sqrt(12)
        rng_ = s.max_x - s.min_x
        assert 1990 < rng_ <= 2000 and s.psnr == pytest.approx(20 * math.log10(rng_ / s.rmse), rel=1e-12)
        assert s.snr == pytest.approx(10 * math.log10(r[7] / r[6]), rel=1e-12)


@pytest.mark.parametrize("name,keeps", [("float32", (0, 7, 10, 23)), ("float64", (0, 7, 10, 52)), ("float16", (0, 3, 5, 10)),
                                        ("bfloat16", (0, 2, 3, 7))])
def test_the_record_under_the_rounding_model(quality, name, keeps):
    k, mant = FORMATS[name]
    xb = planted(name)
    xv = as_double(xb, name)
    rng = np.random.default_rng(mant)
    sample = rng.choice(xb.size, 2048, replace=False)
    F = fractions.Fraction
    for keep in keeps:
        xr, good = round_model(xb, mant, keep)
        yb = np.where(good, xr, xb)
        # a quiet NaN keeps its one payload bit while keep >= 1; at keep 0 the bit is dropped and the NaN is an outlier
        nout = int((~good).sum())
        assert nout == (3 if keep == 0 else 0), (name, keep, nout)
        r = record(xb, yb, name, nout, abs_b=0.0, rel_b=2.0 ** -(keep + 1))
        assert r[0] == 131072 and r[1] == 131069 and r[2] == 3 and r[3] == 0 and r[5] == 0, (name, keep, r[:6])
        yv = as_double(yb, name)
        scale = F(1, 1 << (keep + 1))
        for i in sample:
            if math.isfinite(xv[i]):
                fx = F(float(xv[i]))
                assert abs(fx - F(float(yv[i]))) <= scale * abs(fx), (name, keep, int(i))
        s = quality.ErrorStats(r[:6] + [_bits(r[6]), _bits(r[7])] + r[8:])
        if keep == mant:
            assert s.max_error == 0.0 and s.psnr == math.inf and s.snr == math.inf and s.argmax == 1
        else:
            assert s.max_error > 0 and s.snr > 6.0 * keep and s.argmax not in NAN_AT


def test_word_4_on_the_field_with_nans_is_three(quality):
    """the NaNs are the only outliers of the quantising rule on the field at these bounds, and every NaN is one: a NaN is never
    inside the code range"""
    xb = planted("float32")
    xr, good = quant_model(xb.view(np.float32), 0.5, 0.25)
    assert sorted(np.flatnonzero(~good).tolist()) == sorted(NAN_AT)

"""CPU-side checks of the point-wise relative bounds (shafa_hipd_split_planes_grid_round_dev, shafa_hipd_merge_planes_grid_round_dev,
shafa_hipd_hist_planes_grid_round_dev, csrc/planes_lag.hip) and of the drivers on top (shafa-cd_amd/rounding.py): declared, exported,
bound, the ABI version, the header's section in its place, the submodule's names re-exported and its own, every argument error
refused before HIP is touched — the quantising entries' in their order, then these entries' own where those check step and bound,
then the record arguments — the drivers' ValueErrors before a device is touched, and the numpy model of the rule
(include/shafa_hip.h: "Point-wise relative bounds"): exhaustive over the 16-bit formats at every keep, on random bit patterns at
32 and 64 bits, the guarantee in exact arithmetic, and which elements are outliers (no GPU needed)."""
import ctypes as C
import fractions
import os

import numpy as np
import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64
from test_planes_lag_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAMES = ("shafa_hipd_split_planes_grid_round_dev", "shafa_hipd_merge_planes_grid_round_dev",
         "shafa_hipd_hist_planes_grid_round_dev")
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
FORMATS = {"float16": (2, 10), "bfloat16": (2, 7), "float32": (4, 23), "float64": (8, 52)}


@pytest.fixture(scope="module")
def rounding(shafa):
    return pkgload.load_submodule("rounding")


def _u32(*v):
    return (C.c_uint32 * len(v))(*v)


def test_declared_exported_and_bound(shafa, rounding):
    import torch
    declared = declared_symbols(HEADER)
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert getattr(shafa.lib(), name).restype is C.c_int and getattr(shafa.lib(), name).argtypes, name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_grid_round_dev", "merge_planes_grid_round_dev", "hist_planes_grid_round_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("round_field", "restore_rounded", "compress_rounded", "decompress_rounded", "rounded_histograms", "rounded_sizes",
                 "rounded_rates", "fit_keep_bits"):
        assert callable(getattr(rounding, name, None)), name
        assert getattr(shafa, name) is getattr(rounding, name), name          # re-exported, and the submodule's own
        assert getattr(rounding, name).__module__ == rounding.__name__
    assert shafa.MANTISSA_BITS is rounding.MANTISSA_BITS
    assert dict(rounding.MANTISSA_BITS) == {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23, torch.float64: 52}
    assert rounding.MANTISSA_BITS[torch.bfloat16] == 7 and torch.int32 not in rounding.MANTISSA_BITS
    assert isinstance(rounding.CompressedRounded, type) and shafa.CompressedRounded is rounding.CompressedRounded
    assert rounding.CompressedRounded.__module__ == rounding.__name__
    assert rounding.CompressedRounded.__slots__ == ("dtype", "shape", "lags", "keep_bits", "planes", "outlier_pos", "outlier_bits",
                                                    "nbytes")
    with open(HEADER) as f:
        text = f.read()
    assert text.index("Field sizes under an error bound") < text.index("shafa_hipd_hist_planes_grid_quant_dev(") \
        < text.index("Point-wise relative bounds") < text.index(NAMES[0] + "(") < text.index(NAMES[1] + "(") \
        < text.index(NAMES[2] + "(") < text.index("Byte columns")


@pytest.mark.parametrize("entry", ["split", "merge", "hist"])
def test_argument_errors_before_hip(shafa, entry):
    """the corresponding quantising entry's checks in its order (tests/test_fields_cpu.py, tests/test_field_hist_cpu.py) on the
    stand-in batch with elem 2, 4 or 8 at the elem check; then, where that entry checks step and bound, NULL h_mant / h_keep, a
    mant that is not the format's, keep > mant; then the record arguments"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE
    TOP = (1 << 64) - 1
    MANT = {2: 7, 4: 23, 8: 52}
    hist, merge = entry == "hist", entry == "merge"

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=4, nl=3, lags=_u64(1, 0, 0, 1, 7, TOP, 1 << 63, TOP, 0), mant=None, keep=_u32(0, 3, 7),
                 d_el=A.p, off=_u64(0, 8, (1 << 40) + 24), cap=_u64(5, 100, 70000), d_n=A.p, d_planes=A.p, poff=None, d_outl=A.p,
                 ooff=_u64(0, 16, 17), ocnt=_u64(16, 1, 0), d_outl_n=A.p, d_freq=A.p)
        a.update(kw)
        e = a["elem"] if a["elem"] in (2, 4, 8) else 8
        if a["mant"] is None:
            a["mant"] = _u32(*[MANT[e]] * 3)
        elif a["mant"] == "null":
            a["mant"] = None
        if a["poff"] is None:
            a["poff"] = _u64(*[16 * i for i in range(3 * e)])
        if hist:
            return L.shafa_hipd_hist_planes_grid_round_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["mant"], a["keep"],
                                                           a["d_el"], a["off"], a["cap"], a["d_n"], a["d_freq"], a["d_outl_n"])
        if merge:
            return L.shafa_hipd_merge_planes_grid_round_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["mant"], a["keep"],
                                                            a["d_planes"], a["poff"], a["cap"], a["d_n"], a["d_outl"], a["ooff"],
                                                            a["ocnt"], a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_grid_round_dev(a["b"], None, a["nb"], a["elem"], a["nl"], a["lags"], a["mant"], a["keep"],
                                                        a["d_el"], a["off"], a["cap"], a["d_n"], a["d_planes"], a["poff"],
                                                        a["d_outl"], a["ooff"], a["ocnt"], a["d_outl_n"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    assert reached_hip(call()) and reached_hip(call(elem=8)) and reached_hip(call(elem=2))
    assert reached_hip(call(elem=2, mant=_u32(7, 10, 7), keep=_u32(7, 10, 0)))     # both 16-bit formats in one call
    assert reached_hip(call(nl=1, lags=_u64(1, 7, TOP)))
    if not hist:
        assert reached_hip(call(d_outl=None, ocnt=_u64(0, 0, 0)))          # no records anywhere: no record buffer needed
    # 1. the device pointers, the element size and nlags, in front of nblocks
    for k in ("b", "d_el", "d_n") + (("d_freq",) if hist else ("d_planes",)):
        for nb in (3, 0, -1, 0x7FFFFFFF):
            assert call(**{k: None}, nb=nb) == OM, (k, nb)
    for elem in (0, 1, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    for nl in (0, 4, 0xFFFFFFFF):
        assert call(nl=nl) == OM and call(nl=nl, nb=0) == OM and call(nl=nl, nb=0x7FFFFFFF) == OM, nl
    # 2. no block: success, no host array is looked at — these entries' own neither
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, lags=None, mant="null", keep=None, ooff=None, ocnt=None, d_outl=None, d_outl_n=None) == OK
    # 3. past max_blocks
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF, cap=None, mant="null") == LM
    # 4. the capacities, in front of everything of these entries' own
    assert call(cap=None) == OM and call(cap=None, mant="null") == OM
    big = _u64(5, (1 << 31) * T, 7)
    assert call(cap=big) == LM and call(cap=_u64(TOP, 0, 0)) == LM
    for kw in (dict(mant="null"), dict(keep=None), dict(mant=_u32(23, 7, 23)), dict(keep=_u32(0, 24, 0)), dict(d_outl_n=None),
               dict(ooff=None), dict(ocnt=None), dict(d_outl=None), dict(lags=None), dict(off=None)):
        assert call(cap=big, **kw) == LM, kw
    # 5. the host arrays, alignments and rows of lags
    assert call(off=None) == OM and call(lags=None) == OM
    if not hist:
        assert call(d_planes=C.c_void_p(A.p.value + 8)) == OM
    assert call(off=_u64(0, 8, (1 << 40) + 26)) == OM and call(d_el=C.c_void_p(A.p.value + 2)) == OM
    assert call(elem=2, off=_u64(0, 8, (1 << 40) + 25)) == OM and call(elem=2, d_el=C.c_void_p(A.p.value + 1)) == OM
    assert reached_hip(call(elem=2, off=_u64(0, 2, (1 << 40) + 26), d_el=C.c_void_p(A.p.value + 2)))
    for rows in ((1, 0, 0, 0, 1, 0, 1, 2, 3), (1, 0, 0, 3, 3, 0, 1, 2, 3), (1, 0, 0, 1, 7, TOP, 0, 0, 0), (1, 0, 7, 1, 2, 3, 1, 2, 3)):
        assert call(lags=_u64(*rows)) == OM, rows                           # the row of zeros is malformed in all three
    # 6. these entries' own, where the quantising entries check step and bound
    assert call(mant="null") == OM and call(keep=None) == OM
    legal = {2: (7, 10), 4: (23,), 8: (52,)}
    for elem in (2, 4, 8):
        for i in range(3):
            for m in list(range(0, 70)) + [0xFFFFFFFF]:
                mt, kp = [legal[elem][0]] * 3, [0, 0, 0]
                mt[i] = m
                rc = call(elem=elem, mant=_u32(*mt), keep=_u32(*kp))
                assert reached_hip(rc) if m in legal[elem] else rc == OM, (elem, i, m)
            for m in legal[elem]:
                for keep, ok in ((0, True), (m // 2, True), (m, True), (m + 1, False), (0xFFFFFFFF, False)):
                    mt, kp = [legal[elem][0]] * 3, [0, 0, 0]
                    mt[i], kp[i] = m, keep
                    rc = call(elem=elem, mant=_u32(*mt), keep=_u32(*kp))
                    assert reached_hip(rc) if ok else rc == OM, (elem, i, m, keep)
        m = legal[elem][0]
        assert reached_hip(call(elem=elem, nb=2, mant=_u32(m, m, 99), keep=_u32(0, 0, 99)))      # only the call's blocks
    # 7. then the record arguments as there
    if hist:
        assert call(d_outl_n=None) == OM
        assert call(d_outl_n=None, mant=_u32(23, 7, 23)) == OM
        return
    if not merge:
        assert call(d_outl_n=None) == OM
    assert call(ooff=None) == OM and call(ocnt=None) == OM
    assert call(d_outl=None) == OM                                          # a block has records
    assert call(d_outl=None, ocnt=_u64(0, 0, 1)) == OM and reached_hip(call(nb=2, d_outl=None, ocnt=_u64(0, 0, 1)))


def test_drivers_refuse_bad_arguments_before_a_device(shafa, rounding, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    R = rounding
    cpu = torch.zeros(64, dtype=torch.float32)
    f = _FakeCuda(torch.zeros(4, 6, dtype=torch.float32))
    d = _FakeCuda(torch.zeros(4, 6, dtype=torch.float64))
    h = _FakeCuda(torch.zeros(4, 6, dtype=torch.float16))
    b = _FakeCuda(torch.zeros(4, 6, dtype=torch.bfloat16))
    for bad in (None, b"abc", 5, cpu, [cpu], [None]):
        with pytest.raises(ValueError, match="compress_rounded: "):
            R.compress_rounded(bad, 3)
    # a dtype outside the four
    for dt in (torch.int32, torch.int16, torch.int64, torch.uint8):
        other = _FakeCuda(torch.zeros(8, dtype=dt))
        with pytest.raises(ValueError, match="compress_rounded: float16, bfloat16, float32 and float64 tensors"):
            R.compress_rounded([f, other], 3)
        with pytest.raises(ValueError, match="round_field: float16, bfloat16, float32 and float64 tensors"):
            R.round_field(other, 3, (1,))
        with pytest.raises(ValueError, match="rounded_sizes: float16, bfloat16, float32 and float64 tensors"):
            R.rounded_sizes(other, 3)
        with pytest.raises(ValueError, match="rounded_rates: float16, bfloat16, float32 and float64 tensors"):
            R.rounded_rates(other, [3])
        with pytest.raises(ValueError, match="fit_keep_bits: float16, bfloat16, float32 and float64 tensors"):
            R.fit_keep_bits(other, 100)
        with pytest.raises(ValueError, match="rounded_histograms: float16, bfloat16, float32 and float64 tensors"):
            R.rounded_histograms(other, 3, [(1,)])
        with pytest.raises(ValueError, match="restore_rounded: float16, bfloat16, float32 and float64 tensors"):
            R.restore_rounded(torch.zeros(4, 8, dtype=torch.uint8), dt, (8,), (1,), 3, torch.zeros(0, dtype=torch.int64),
                              torch.zeros(0, dtype=torch.int64))
    # a bool, a non-int or an out-of-range keep_bits
    for t, top in ((f, 23), (d, 52), (h, 10), (b, 7)):
        for keep in (True, False, None, 3.0, "3", -1, top + 1, 1 << 40):
            with pytest.raises(ValueError, match="compress_rounded: keep_bits is an int 0 .. %d" % top):
                R.compress_rounded(t, keep)
            with pytest.raises(ValueError, match="compress_rounded: keep_bits is an int 0 .. %d" % top):
                R.compress_rounded([f, t], [3, keep])
            with pytest.raises(ValueError, match="round_field: keep_bits is an int"):
                R.round_field(t, keep, (1,))
            with pytest.raises(ValueError, match="rounded_sizes: keep_bits is an int"):
                R.rounded_sizes(t, keep)
            with pytest.raises(ValueError, match="rounded_rates: keep_bits is an int"):
                R.rounded_rates(t, [0, keep])
            with pytest.raises(ValueError, match="fit_keep_bits: keep_bits is an int"):
                R.fit_keep_bits(t, 100, keeps=[keep])
            with pytest.raises(ValueError, match="rounded_histograms: keep_bits is an int"):
                R.rounded_histograms(t, keep, [(1,)])
    # a list of the wrong length
    for keeps in ([], [3], [3] * 3, (3,)):
        with pytest.raises(ValueError, match="compress_rounded: keep_bits is an int or a list with one int per tensor"):
            R.compress_rounded([f, d], keeps)
        with pytest.raises(ValueError, match="rounded_sizes: keep_bits is an int or a list with one int per tensor"):
            R.rounded_sizes([f, d], keeps)
    with pytest.raises(ValueError, match="rounded_histograms: keep_bits is an int or a list with one int per entry"):
        R.rounded_histograms(f, [1, 2, 3], [(1,), ()])
    for keeps in ([], 3, "abc"):
        with pytest.raises(ValueError, match="rounded_rates: keeps is a non-empty list of ints"):
            R.rounded_rates(f, keeps)
    with pytest.raises(ValueError, match="rounded_rates: keeps is a non-empty list of ints"):
        R.rounded_rates(f, None)
    for mb in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="fit_keep_bits: max_bytes is an int >= 0"):
            R.fit_keep_bits(f, mb)
    assert R.compress_rounded([], 3) == [] and R.decompress_rounded([]) == []
    with pytest.raises(ValueError, match="compress_rounded: block_size"):
        R.compress_rounded(f, 3, block_size=-1)
    with pytest.raises(ValueError, match="compress_rounded: lags are strictly increasing"):
        R.compress_rounded(f, 3, lags=(6, 1))
    with pytest.raises(ValueError, match="compress_rounded: lags is a tuple of ints or a list with one tuple per tensor"):
        R.compress_rounded([f, d], 3, lags=[(1,)])
    with pytest.raises(ValueError, match="compress_rounded: axis 2 of a tensor of 2 dimensions"):
        R.compress_rounded(f, 3, axes=(0, 2))
    with pytest.raises(ValueError, match="rounded_histograms: an entry of lag_sets is a tuple"):
        R.rounded_histograms(f, 3, [[1]])
    # () is legal wherever lags go: the refusal behind it is the next check's
    with pytest.raises(ValueError, match="compress_rounded: block_size"):
        R.compress_rounded([f, d], 3, lags=[(), (1, 6)], block_size=-1)
    with pytest.raises(ValueError, match="compress_rounded: block_size"):
        R.compress_rounded(f, 3, lags=(), block_size=-1)
    with pytest.raises(ValueError, match="rounded_sizes: keep_bits"):
        R.rounded_sizes(f, 99, candidates=[(), (1,)])
    # foreign items
    raw = torch.zeros(24, dtype=torch.uint8)
    none = torch.zeros(0, dtype=torch.int64)
    cg = shafa.CompressedGrid(torch.float32, (4, 6), (1, 6), [raw] * 4, 96)
    cf = shafa.CompressedField(torch.float32, (4, 6), (1, 6), 1e-3, 0.5, 0.25, [raw] * 4, none, none, 96)
    for bad in (cg, [cg], cf, [cf], None, 5, [None], shafa.CompressedTensor(torch.float32, (24,), [raw] * 4, 96)):
        with pytest.raises(ValueError, match="decompress_rounded: a CompressedRounded or a list of them"):
            R.decompress_rounded(bad)
    CR = R.CompressedRounded
    item = CR(torch.float32, (4, 6), (1, 6), 10, [raw] * 4, none, none, 96)
    assert not hasattr(item, "__dict__") and repr(item).startswith("CompressedRounded(torch.float32, (4, 6), lags=(1, 6), keep_bits=10")
    with pytest.raises(ValueError, match="decompress_grids: a CompressedGrid or a list of them"):
        shafa.decompress_grids([item])
    with pytest.raises(ValueError, match="decompress_fields: a CompressedField or a list of them"):
        shafa.decompress_fields([item])
    for keep in (True, 24, -1, 2.0):
        with pytest.raises(ValueError, match="decompress_rounded: keep_bits is an int 0 .. 23"):
            R.decompress_rounded(CR(torch.float32, (4, 6), (1, 6), keep, [raw] * 4, none, none, 96))
    with pytest.raises(ValueError, match="decompress_rounded: keep_bits is an int 0 .. 7"):
        R.decompress_rounded(CR(torch.bfloat16, (4, 6), (1, 6), 8, [raw] * 2, none, none, 48))
    with pytest.raises(ValueError, match="decompress_rounded: (lags are|a lag is)"):
        R.decompress_rounded(CR(torch.float32, (4, 6), (6, 1), 10, [raw] * 4, none, none, 96))
    with pytest.raises(ValueError, match="decompress_rounded: float16, bfloat16, float32 and float64 tensors"):
        R.decompress_rounded(CR(torch.int32, (4, 6), (1, 6), 10, [raw] * 4, none, none, 96))
    with pytest.raises(ValueError, match="decompress_rounded: one position and one bit pattern per outlier"):
        R.decompress_rounded(CR(torch.float32, (4, 6), (1, 6), 10, [raw] * 4, none, torch.zeros(1, dtype=torch.int64), 96))
    # a lossless item that carries outliers
    one = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="decompress_rounded: an item kept lossless has no outliers"):
        R.decompress_rounded(CR(torch.float32, (4, 6), (1, 6), None, [raw] * 4, _FakeCuda(one), _FakeCuda(one), 96))
    for it in (item, CR(torch.float16, (4, 6), (), None, [raw] * 2, none, none, 48)):
        with pytest.raises(ValueError, match="decompress_rounded: planes are CUDA tensors"):
            R.decompress_rounded(it)


# ---------------------------------------------------------------- the numpy model of the rule
def model(x, mant, keep):
    """include/shafa_hip.h, "Point-wise relative bounds", in numpy: x an array of uint16, uint32 or uint64 bit patterns -> (the
    codes as unsigned integers of that width, x' as bits, good).  Every operation is one unsigned operation of the width."""
    U = x.dtype.type
    W = 8 * x.dtype.itemsize
    d = mant - keep
    MAG, INF, MIN = U((1 << (W - 1)) - 1), U(((1 << (W - 1 - mant)) - 1) << mant), U(1 << mant)
    S, M = x >> U(W - 1), x & MAG
    rn = M if d == 0 else (M + U((1 << (d - 1)) - 1) + ((M >> U(d)) & U(1))) >> U(d)
    R = np.where(M >= INF, M >> U(d), rn)
    code = np.where(S == 1, U(0) - R, R)
    back = (R << U(d)) & MAG
    good = np.where((M < MIN) | (M >= INF), back == M, back < INF)
    return code, merged(code, mant, keep), good


def merged(code, mant, keep):
    """what the merge makes of ANY code: the sign of the signed integer, |code| << d mod 2^(W-1)"""
    U = code.dtype.type
    W = 8 * code.dtype.itemsize
    neg = code >> U(W - 1)
    a = np.where(neg == 1, U(0) - code, code)
    return (neg << U(W - 1)) | ((a << U(mant - keep)) & U((1 << (W - 1)) - 1))


def as_float(bits, name):
    """the values of bit patterns of a format, in the narrowest numpy float that holds them exactly"""
    if name == "bfloat16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view({"float16": np.float16, "float32": np.float32, "float64": np.float64}[name])


def classes(x, mant, keep):
    """the three kinds of outlier, each from its own description: (a normal value that rounds up to Inf, a denormal with a
    dropped bit set, a NaN whose payload reaches into the dropped bits)"""
    U = x.dtype.type
    W = 8 * x.dtype.itemsize
    d = mant - keep
    MAG, INF, MIN = U((1 << (W - 1)) - 1), U(((1 << (W - 1 - mant)) - 1) << mant), U(1 << mant)
    M = x & MAG
    low = M & U((1 << d) - 1)
    # the top binade's mantissas from which the nearest multiple of 2^d, ties to even, is 2^(mant + 1): the carry makes Inf
    frac, top = M & U(MIN - U(1)), (M >> U(mant)) == (INF >> U(mant)) - U(1)
    up = np.zeros(x.shape, bool)
    if d:
        rest = int(MIN) - frac.astype(np.int64 if W < 64 else np.uint64)     # the distance to the next binade, > 0
        half = 1 << (d - 1)
        kept_odd = ((M >> U(d)) & U(1)) == 1
        up = (rest < half) | ((rest == half) & kept_odd)
    return top & up, (M > 0) & (M < MIN) & (low != 0), (M > INF) & (low != 0)


def check_guarantee(x, name, mant, keep, exact):
    """the contract's guarantee on the bit patterns x of a format; `exact`: the indices whose bound is checked in Fractions"""
    F = fractions.Fraction
    U = x.dtype.type
    W = 8 * x.dtype.itemsize
    MAG, INF, MIN = U((1 << (W - 1)) - 1), U(((1 << (W - 1 - mant)) - 1) << mant), U(1 << mant)
    code, xr, good = model(x, mant, keep)
    M = x & MAG
    normal = (M >= MIN) & (M < INF)
    # every other good element comes back equal in value: bit for bit, but -0.0 as +0.0
    other = good & ~normal
    minus0 = x == U(1 << (W - 1))
    assert (xr[other & ~minus0] == x[other & ~minus0]).all() and (xr[minus0] == 0).all()
    assert good[M == 0].all() and good[M == INF].all()                      # zeros and infinities are never outliers
    # a good normal element is finite, keeps its sign, and is within 2^-(keep + 1) |x|
    gn = good & normal
    assert ((xr[gn] & MAG) < INF).all() and ((xr[gn] >> U(W - 1)) == (x[gn] >> U(W - 1))).all()
    assert ((xr[gn] & U((1 << (mant - keep)) - 1)) == 0).all()              # the dropped bits are zeros
    xv, rv = as_float(x, name), as_float(xr, name)
    scale = F(1, 1 << (keep + 1))
    for i in exact:
        if gn[i]:
            fx = F(float(xv[i]))
            assert abs(fx - F(float(rv[i]))) <= scale * abs(fx), (name, keep, hex(int(x[i])))
    # keep = mant is the identity but for -0.0
    if keep == mant:
        assert good.all() and (xr[~minus0] == x[~minus0]).all()
    # the code of ANY element restores to x' (model does so by construction: the code alone gives x'), the pattern 0 has code 0
    assert (merged(code, mant, keep) == xr).all()
    assert model(np.zeros(1, x.dtype), mant, keep)[0][0] == 0
    # the outliers are exactly the three classes
    up, den, nan = classes(x, mant, keep)
    assert not (up & den).any() and not (up & nan).any() and not (den & nan).any()
    assert ((~good) == (up | den | nan)).all(), (name, keep)
    assert (((xr[up] & MAG) == INF)).all()                                  # rounds up to Inf exactly
    return good


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_the_model_exhaustive_at_16_bits(rounding, name):
    """all 65 536 bit patterns at EVERY keep, every good normal element's bound in fractions.Fraction"""
    k, mant = FORMATS[name]
    assert k == 2 and sorted(rounding.MANTISSA_BITS.values()) == [7, 10, 23, 52]
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    every = range(65536)
    seen_outlier = False
    for keep in range(mant + 1):
        good = check_guarantee(x, name, mant, keep, every)
        seen_outlier |= bool((~good).any())
    assert seen_outlier


@pytest.mark.parametrize("name", ["float32", "float64"])
def test_the_model_on_random_bit_patterns(rounding, name):
    """10^5 random bit patterns at keep 0, 1, mant / 2, mant - 1 and mant, with the borders planted"""
    k, mant = FORMATS[name]
    assert rounding.MANTISSA_BITS is not None
    U = UINT[k]
    W = 8 * k
    rng = np.random.default_rng(mant)
    x = rng.integers(0, 1 << W, 100000, dtype=np.uint64).astype(U)
    INF, MIN = ((1 << (W - 1 - mant)) - 1) << mant, 1 << mant
    for keep in (0, 1, mant // 2, mant - 1, mant):
        d = mant - keep
        border = [0, 1 << (W - 1), 1, MIN - 1, MIN, MIN + 1, INF - 1, INF, INF + 1, INF + (1 << d), INF | (MIN >> 1), (1 << (W - 1)) - 1,
                  INF - MIN, INF - (1 << d) if d else INF - 1, INF - (1 << d) // 2 - 1 if d else INF - 2, INF - (1 << d) // 2 if d else INF - 3,
                  3 << d, (3 << d) + (1 << d) // 2, (2 << d) + (1 << d) // 2, MIN + (((1 << d) * 3) // 2), MIN + (1 << d) // 2]
        xs = x.copy()
        for j, v in enumerate(border):
            xs[2 * j] = U(v % (1 << (W - 1)))
            xs[2 * j + 1] = U((v % (1 << (W - 1))) | (1 << (W - 1)))
        check_guarantee(xs, name, mant, keep, range(xs.size))


def the_field(name):
    """DESIGN 7.28's [32, 64, 64] field in a format, as bit patterns: 1000 sin(x / 9) cos(y / 13) sin(z / 7 + 0.3)"""
    import torch
    z, y, x = np.mgrid[0:32, 0:64, 0:64].astype(np.float64)
    f = 1000 * np.sin(x / 9) * np.cos(y / 13) * np.sin(z / 7 + 0.3)
    k = FORMATS[name][0]
    t = torch.from_numpy(f).to(getattr(torch, name)).reshape(-1)
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[k]).numpy().view(UINT[k])


@pytest.mark.parametrize("name,keeps", [("float32", (7, 10, 15)), ("float64", (7, 10, 15)), ("float16", (3, 5, 7)),
                                        ("bfloat16", (2, 3, 5))])
def test_the_model_on_the_field(rounding, shafa, name, keeps):
    k, mant = FORMATS[name]
    x = the_field(name)
    assert x.size == 131072 and shafa.fields.outlier_capacity(x.size) == 2064
    xv = as_float(x, name).astype(np.float64)
    for keep in keeps:
        code, xr, good = model(x, mant, keep)
        assert int((~good).sum()) == 0, (name, keep)
        rv = as_float(xr, name).astype(np.float64)
        assert (np.abs(xv - rv) <= np.abs(xv) * 2.0 ** -(keep + 1)).all()    # exact in float64 at these magnitudes and widths

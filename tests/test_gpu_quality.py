"""shafa_hipd_error_dev / shafa_hipd_error_quant_dev / shafa_hipd_error_round_dev (csrc/planes_lag.hip) and the drivers on top
(shafa-cd_amd/quality.py) against numpy on the host.  The record (include/shafa_hip.h: "Error statistics") and the two rules that
make what comes back ("Error-bounded fields", "Point-wise relative bounds") are restated here in numpy.  Words 0 - 5 and 9 are
compared integer for integer, words 8, 10 and 11 bit for bit, and the two sums, words 6 and 7, within a relative n 2^-52 of
math.fsum over numpy's own terms: the terms are bit-identical by the contract, a sum of n non-negative doubles in any order errs by
less than n 2^-53 of itself, and the reference's own rounding takes the other half; a sum whose terms are all 0 is exactly 0.0.

d_stat holds 0xA5 between guard words and whole buffers are compared.  A lane has 16 elements, a tile T = PLANES_TILE."""
import math
import struct

import numpy as np
import pytest

from test_gpu_planes_lag import FILL, UINT, _fill, _sizes, _to
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

MANT = {"float16": 10, "bfloat16": 7, "float32": 23, "float64": 52}
ELEM = {"float16": 2, "bfloat16": 2, "float32": 4, "float64": 8}
FLOAT = {4: np.float32, 8: np.float64}
INT = {4: np.int32, 8: np.int64}
FMTS = {2: ("bfloat16", "float16"), 4: ("float32",), 8: ("float64",)}
FILL64 = int.from_bytes(bytes([FILL] * 8), "little")
NONE = (1 << 64) - 1
W12 = 12


def _b(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# ---------------------------------------------------------------- the rules and the record, in numpy
def _round(x, mant, keep):
    """"Point-wise relative bounds": bit patterns -> (what comes back as bits, good)"""
    U = x.dtype.type
    W = 8 * x.dtype.itemsize
    d = U(mant - keep)
    MAG, INF, MIN = U((1 << (W - 1)) - 1), U(((1 << (W - 1 - mant)) - 1) << mant), U(1 << mant)
    S, M = x >> U(W - 1), x & MAG
    rn = M if mant == keep else (M + U((1 << (mant - keep - 1)) - 1) + ((M >> d) & U(1))) >> d
    R = np.where(M >= INF, M >> d, rn)
    back = (R << d) & MAG
    good = np.where((M < MIN) | (M >= INF), back == M, back < INF)
    neg = S & (R != 0).astype(U)                                           # the sign of the code: -0.0 comes back as +0.0
    return np.where(good, (neg << U(W - 1)) | back, x), good


def _quant(xb, step, bound):
    """"Error-bounded fields": bit patterns of floats or doubles -> (what comes back as bits, good); one operation in T each"""
    k = xb.dtype.itemsize
    T = FLOAT[k]
    x = xb.view(T)
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
    return np.where(good, xr.view(UINT[k]), xb), good


def _dbl(bits, fmt):
    """D(.)"""
    with np.errstate(invalid="ignore"):                                    # a signalling NaN stays a NaN
        if fmt == "bfloat16":
            return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
        return bits.view({"float16": np.float16, "float32": np.float32, "float64": np.float64}[fmt]).astype(np.float64)


def _record(xb, yb, fmt, outliers=0, abs_b=None, rel_b=0.0):
    """the twelve words; 6 and 7 as Python floats from math.fsum.  abs_b None: a fused entry, word 5 is 0"""
    x, y = _dbl(xb, fmt), _dbl(yb, fmt)
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(all="ignore"):
        e = np.abs(x - y)
        over = fin & (e > np.float64(abs_b) + np.float64(rel_b) * np.abs(x)) if abs_b is not None else np.zeros(x.shape, bool)
    ef, xf = e[fin], x[fin]
    emax = float(ef.max()) if ef.size else 0.0
    at = int(np.flatnonzero(fin & (e == emax))[0]) if ef.size else NONE
    zero = lambda v: 0.0 if v == 0 else v
    return [xb.size, int(fin.sum()), int((~fin).sum()), int((~fin & (xb != yb)).sum()), outliers, int(over.sum()),
            math.fsum((ef * ef).tolist()), math.fsum((xf * xf).tolist()), _b(emax), at,
            _b(zero(float(xf.min())) if xf.size else math.inf), _b(zero(float(xf.max())) if xf.size else -math.inf)]


def _same(got, want, what=""):
    """one record of uint64 against _record's"""
    got = [int(v) for v in got]
    for i in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):
        assert got[i] == want[i], (what, i, got, want)
    for i in (6, 7):
        g = struct.unpack("<d", struct.pack("<Q", got[i]))[0]
        if want[i] == 0.0:
            assert got[i] == 0, (what, i, g)                               # every term is 0: exactly +0.0
        else:
            assert abs(g - want[i]) <= want[0] * 2.0 ** -52 * want[i], (what, i, g, want[i])


def _whole(d_stat, wants, what=""):
    """the whole buffer: a guard word, the records, a guard word"""
    got = d_stat.cpu().numpy().view(np.uint64)
    assert got.size == W12 * len(wants) + 2 and got[0] == FILL64 and got[-1] == FILL64, what
    for b, w in enumerate(wants):
        _same(got[1 + W12 * b:1 + W12 * (b + 1)], w, (what, b))
    return got[1:-1].reshape(-1, W12)


# ---------------------------------------------------------------- the data
def _to_bits(v, fmt):
    if fmt == "bfloat16":
        return (v.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return v.astype({"float16": np.float16, "float32": np.float32, "float64": np.float64}[fmt]).view(UINT[ELEM[fmt]])


def _consts(fmt):
    mant, W = MANT[fmt], 8 * ELEM[fmt]
    return 1 << (W - 1), ((1 << (W - 1 - mant)) - 1) << mant, 1 << mant


def _values(n, fmt, T, seed, ties=()):
    """a ramp with a sine over several binades and both signs; -0.0, denormals, the smallest normal and exact ties sprinkled
    through it; NaN and +-Inf at the first and the last element, at 15 / 16 / 17 and across the tile border"""
    SIGN, INF, MIN = _consts(fmt)
    i = np.arange(n, dtype=np.float64)
    span = {"float16": 12, "bfloat16": 60, "float32": 60, "float64": 400}[fmt]
    with np.errstate(over="ignore"):
        v = (1.0 + 0.37 * np.sin(i / 11 + seed)) * 2.0 ** (span * np.sin(i / 301 + 0.1 * seed)) * np.where((i // 7) % 3 == 1, -1.0, 1.0)
        x = _to_bits(v, fmt).copy()
    U = x.dtype.type
    one = (INF >> 1) & ~(MIN - 1)
    sp = [0, SIGN, 1, 3 | SIGN, MIN - 1, MIN, SIGN | MIN, one | (MIN >> 1), one | (MIN >> 2) | (MIN >> 1), SIGN | one | 1,
          one + 5 * MIN + (MIN >> 3)] + [int(_to_bits(np.array([t]), fmt)[0]) for t in ties]
    for j, v in enumerate(sp):
        x[5 + j + seed % 3:n:97] = U(v)
    nonfin = [INF, INF | (MIN >> 1), SIGN | INF, SIGN | INF | 1]
    for j, at in enumerate(sorted({0, n - 1, 15, 16, 17, T - 1, T, T + 1})):
        if 0 <= at < n:
            x[at] = U(nonfin[(j + seed) % 4])
    return x


def _blocks(k, T, params):
    """the blocks of one launch at element size k: (what, format, elements off a 16-byte boundary, bit patterns, parameter) —
    `params` a list the blocks cycle through, params[1] the one the planted blocks take"""
    SIZES = [0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3]
    offs = list(range(8)) if k == 2 else [0, 1, 3]
    out = []
    for j, n in enumerate(SIZES):
        fmt = FMTS[k][j % len(FMTS[k])]
        p = params[j % len(params)]
        out.append((f"n={n}", fmt, offs[j % len(offs)], _values(n, fmt, T, j, p.get("ties", ())), p))
    if k == 2:                                                             # every offset 0 .. 7, and the other format at the large sizes
        for j, n in enumerate([T + 1, 2 * T + 3, 17, T - 1, 33, 100, T, 16]):
            fmt = FMTS[k][(j + 1) % 2]
            out.append((f"n={n}'", fmt, (j + 3) % 8, _values(n, fmt, T, 20 + j), params[(j + 2) % len(params)]))
    for j, fmt in enumerate(FMTS[k]):
        SIGN, INF, MIN = _consts(fmt)
        U = UINT[k]
        p = params[1]
        ramp = lambda n: _to_bits(1.0 + (np.arange(n) % 1000) / 1024.0, fmt)
        out.append(("no finite element", fmt, 1, np.array([INF, SIGN | INF, INF | (MIN >> 1), SIGN | INF | 1] * 10, U), p))
        out.append(("zeros", fmt, 3, np.zeros(33, U), p))
        big = _to_bits(np.array([p["big"]]), fmt)[0]
        x = p["small"](2 * T + 3, fmt)
        x[[100, 100 + 16 * 64, T + 3]] = big                                # twice in a tile (two waves) and in the next tile
        out.append(("largest thrice", fmt, 0, x, dict(p, first=100)))
        x = p["small"](T + 17, fmt)
        x[-1] = big                                                        # the last element of a cut tile
        out.append(("largest last", fmt, 1, x, dict(p, first=T + 16)))
        x = ramp(50)
        x[0], x[-1] = _to_bits(np.array([-16384.0]), fmt)[0], _to_bits(np.array([16384.0]), fmt)[0]
        out.append(("min first, max last", fmt, 0, x.copy(), p))
        out.append(("max first, min last", fmt, 3, x[::-1].copy(), p))
    return out


class _Image:
    """the blocks' bit patterns in a host image, block b at off[b]: `a` elements behind a multiple of 64 bytes"""

    def __init__(self, k, xs, a):
        self.off, pos = [], 0
        for x, o in zip(xs, a):
            pos = (pos + 16 + 63) // 64 * 64 + o * k
            self.off.append(pos)
            pos += x.size * k
        self.img = np.full(pos + 80, FILL, np.uint8)
        for x, o in zip(xs, self.off):
            self.img[o:o + x.size * k] = x.view(np.uint8)


def _stream():
    import torch
    return torch.cuda.Stream(device=_dev())


def _fill64(n):
    import torch
    return torch.full((n * 8,), FILL, dtype=torch.uint8, device=_dev()).view(torch.int64)


def _small_round(n, fmt):
    return _to_bits(1.0 + (np.arange(n) % 1000) / 1024.0, fmt).copy()


def _small_quant(n, fmt):
    return _to_bits((np.arange(n) % 97) / 97.0 - 0.5, fmt).copy()


def _round_params():
    """keep 0, 1, mant / 2, mant - 1 and mant; the planted blocks take keep 1, at which 1280 is an exact tie and comes back as 1024"""
    return [dict(keep=f, big=1280.0, small=_small_round) for f in (lambda m: 0, lambda m: 1, lambda m: m // 2, lambda m: m - 1, lambda m: m)]


def _quant_params(shafa, k):
    out = []
    for e in (2.0 ** -21, 1e-3, 0.25, 1.5, 1e5):
        step, bound = (0.5, 0.25) if e == 0.25 else shafa.fields._params("test", e, k)
        out.append(dict(step=step, bound=bound, ties=[(j + 0.5) * step for j in (-3, -2, 0, 1, 2, 1001)], big=1.25, small=_small_quant))
    out[1], out[2] = out[2], out[1]                                        # the planted blocks take step 0.5: 1.25 is an exact tie
    return out


# ---------------------------------------------------------------- 1. one launch of each entry per element size
@pytest.mark.parametrize("k", (2, 4, 8))
def test_one_launch_of_the_rounding_entry(shafa, k):
    T = shafa.PLANES_TILE
    blocks = _blocks(k, T, _round_params())
    xs = [b[3] for b in blocks]
    L = _Image(k, xs, [b[2] for b in blocks])
    mant = [MANT[b[1]] for b in blocks]
    keep = [b[4]["keep"](m) for b, m in zip(blocks, mant)]
    assert {0, 1} <= set(keep) and any(kp == m for kp, m in zip(keep, mant)) and (k != 2 or {7, 10} == set(mant))
    wants = []
    for (what, fmt, _, x, p), m, kp in zip(blocks, mant, keep):
        y, good = _round(x, m, kp)
        wants.append(_record(x, y, fmt, int((~good).sum())))
        if "first" in p and kp < m:
            assert wants[-1][9] == p["first"] and struct.unpack("<d", struct.pack("<Q", wants[-1][8]))[0] == 256.0, (what, wants[-1])
    nb = len(blocks)
    st = _stream()
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_el, d_stat = _to(L.img), _fill64(W12 * nb + 2)
        bt.error_round_dev(st, k, mant, keep, d_el, L.off, [x.size for x in xs], _sizes([x.size for x in xs]), d_stat[1:-1])
        assert bt.finish(st, nb) == (0, [0] * nb)
        _whole(d_stat, wants, [b[0] for b in blocks])
        assert d_el.cpu().numpy().tobytes() == L.img.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("k", (4, 8))
def test_one_launch_of_the_quantising_entry(shafa, k):
    T = shafa.PLANES_TILE
    params = _quant_params(shafa, k)
    assert len({p["step"] for p in params}) == 5
    blocks = _blocks(k, T, params)
    xs = [b[3] for b in blocks]
    L = _Image(k, xs, [b[2] for b in blocks])
    wants = []
    for what, fmt, _, x, p in blocks:
        y, good = _quant(x, p["step"], p["bound"])
        wants.append(_record(x, y, fmt, int((~good).sum())))
        if "first" in p:
            assert wants[-1][9] == p["first"] and wants[-1][8] == _b(0.25), (what, wants[-1])
    assert any(w[4] > 3 for w in wants) and any(w[4] == 0 and w[1] for w in wants)
    nb = len(blocks)
    st = _stream()
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_el, d_stat = _to(L.img), _fill64(W12 * nb + 2)
        bt.error_quant_dev(st, k, [b[4]["step"] for b in blocks], [b[4]["bound"] for b in blocks], d_el, L.off, [x.size for x in xs],
                           _sizes([x.size for x in xs]), d_stat[1:-1])
        assert bt.finish(st, nb) == (0, [0] * nb)
        _whole(d_stat, wants, [b[0] for b in blocks])
        assert d_el.cpu().numpy().tobytes() == L.img.tobytes()
    finally:
        bt.close()


def _came_back(x, fmt, seed, first=None):
    """a second tensor for x: the rounding rule's at half the mantissa, then NaNs with other payloads, a finite value where the
    original has a NaN and the other way round; `first`: the planted blocks, whose y is x but for the planted elements"""
    SIGN, INF, MIN = _consts(fmt)
    U = x.dtype.type
    if first is not None:
        y = x.copy()
        big = _to_bits(np.array([1280.0]), fmt)[0]
        y[x == big] = _to_bits(np.array([1280.0 + 256.0]), fmt)[0]
        return y
    y, _ = _round(x, MANT[fmt], MANT[fmt] // 2)
    y = y.copy()
    nan = np.flatnonzero((x & U(SIGN - 1)) > U(INF))
    y[nan[1::2]] ^= U(2)                                                   # another payload, or an infinity
    y[nan[2::5]] = _to_bits(np.array([1.0]), fmt)[0]
    fin = np.flatnonzero((x & U(SIGN - 1)) < U(INF))
    y[fin[seed % 7::53]] = U(INF | (MIN >> 1))
    return y


PAIR_BOUNDS = ((math.inf, 0.0), (0.0, 0.0), (0.0, 2.0 ** -6), (1e-3, 0.0), (0.5, 2.0 ** -4))


@pytest.mark.parametrize("k", (2, 4, 8))
def test_one_launch_of_the_two_tensor_entry(shafa, k):
    T = shafa.PLANES_TILE
    blocks = _blocks(k, T, [dict(big=1280.0, small=_small_round)] * 2)
    xs = [b[3] for b in blocks]
    ys = [_came_back(b[3], b[1], j, b[4].get("first")) for j, b in enumerate(blocks)]
    R, A = _Image(k, xs, [b[2] for b in blocks]), _Image(k, ys, [0] * len(blocks))
    bounds = [PAIR_BOUNDS[j % 5] for j in range(len(blocks))]
    mant = [MANT[b[1]] for b in blocks]
    wants = [_record(x, y, b[1], 0, *bd) for x, y, b, bd in zip(xs, ys, blocks, bounds)]
    for b, w in zip(blocks, wants):
        if "first" in b[4]:
            assert w[9] == b[4]["first"] and w[8] == _b(256.0), (b[0], w)
    assert any(w[3] for w in wants) and any(w[5] for w in wants) and any(w[2] > w[3] > 0 for w in wants)
    nb = len(blocks)
    st = _stream()
    bt = shafa.Batch(nb, 1 << 20)
    try:
        d_a, d_ref, d_stat = _to(A.img), _to(R.img), _fill64(W12 * nb + 2)
        assert d_a.data_ptr() % 16 == 0 and not any(o % 16 for o in A.off)
        bt.error_dev(st, k, mant, [b[0] for b in bounds], [b[1] for b in bounds], d_a, A.off, [x.size for x in xs],
                     _sizes([x.size for x in xs]), d_ref, R.off, d_stat[1:-1])
        assert bt.finish(st, nb) == (0, [0] * nb)
        _whole(d_stat, wants, [b[0] for b in blocks])
        assert d_a.cpu().numpy().tobytes() == A.img.tobytes() and d_ref.cpu().numpy().tobytes() == R.img.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. a record is a function of its block alone
@pytest.mark.parametrize("entry,k", [("round", 2), ("quant", 4), ("pair", 8), ("round", 8)])
def test_the_same_block_gives_the_same_words(shafa, entry, k):
    """three times in one call among different neighbours, alone in another call, and at another alignment"""
    T = shafa.PLANES_TILE
    fmt = FMTS[k][0]
    x = _values(2 * T + 3, fmt, T, 5)
    others = [_values(n, fmt, T, 9 + n % 5) for n in (T + 1, 17, 3 * T, 1)]
    y, yo = _came_back(x, fmt, 1), [_came_back(o, fmt, 2) for o in others]
    step, bound = shafa.fields._params("test", 1e-3, 4)

    def launch(bt, st, xs, ys, a):
        R, A = _Image(k, xs, a), _Image(k, ys, [0] * len(xs))
        n = [v.size for v in xs]
        d_stat, d_ref = _fill64(W12 * len(xs) + 2), _to(R.img)
        if entry == "round":
            bt.error_round_dev(st, k, [MANT[fmt]] * len(xs), [3] * len(xs), d_ref, R.off, n, _sizes(n), d_stat[1:-1])
        elif entry == "quant":
            bt.error_quant_dev(st, k, [step] * len(xs), [bound] * len(xs), d_ref, R.off, n, _sizes(n), d_stat[1:-1])
        else:
            bt.error_dev(st, k, [MANT[fmt]] * len(xs), [1e-3] * len(xs), [2.0 ** -9] * len(xs), _to(A.img), A.off, n, _sizes(n), d_ref,
                         R.off, d_stat[1:-1])
        assert bt.finish(st, len(xs)) == (0, [0] * len(xs))
        return d_stat.cpu().numpy().view(np.uint64)[1:-1].reshape(-1, W12)

    st = _stream()
    bt = shafa.Batch(8, 1 << 20)
    try:
        many = launch(bt, st, [x, others[0], x, others[1], others[2], x, others[3]], [y, yo[0], y, yo[1], yo[2], y, yo[3]],
                      [0, 1, 3, 0, 2, 1, 0])
        alone = launch(bt, st, [x], [y], [0])
        moved = launch(bt, st, [others[1], x], [yo[1], y], [1, 16 // k - 1])
    finally:
        bt.close()
    want = many[0].tolist()
    assert want[0] == 2 * T + 3 and want[1] > 0 and want[2] > 0
    for got in (many[2], many[5], alone[0], moved[1]):
        assert got.tolist() == want


# ---------------------------------------------------------------- 3. the fused entries against the two steps they replace
def _tensor(bits, fmt, shape=None):
    import torch
    k = ELEM[fmt]
    t = torch.from_numpy(bits.view({2: np.int16, 4: np.int32, 8: np.int64}[k]).copy()).to(_dev()).view(getattr(torch, fmt))
    return t if shape is None else t.view(shape)


def _host_bits(t):
    import torch
    k = t.element_size()
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[k]).cpu().numpy().view(UINT[k]).reshape(-1)


@pytest.mark.parametrize("fmt", ("float32", "float64"))
def test_fused_quantising_against_split_merge_and_compare(shafa, fmt):
    T = shafa.PLANES_TILE
    k = ELEM[fmt]
    step, bound = shafa.fields._params("test", 1e-3, k)
    x = _values(2 * T + 3, fmt, T, 2, ties=[(j + 0.5) * step for j in (-2, 0, 7)])
    t = _tensor(x, fmt)
    planes, pos, bits = shafa.quantize_field(t, 1e-3, (1,))
    back = shafa.restore_field(planes, t.dtype, t.shape, (1,), step, pos, bits)
    y, good = _quant(x, step, bound)
    assert _host_bits(back).tobytes() == y.tobytes()
    fused = shafa.field_errors(t, [1e-3])[0].words()
    two = shafa.tensor_errors(back, t).words()
    _same(fused, _record(x, y, fmt, int((~good).sum())), "fused")
    for i in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11):                             # the terms are the same and so is the tree
        assert fused[i] == two[i], (i, fused, two)
    _, outl = shafa.field_histograms(t, 1e-3, [(1,)])
    assert fused[4] == int(outl.cpu()[0]) == int(pos.numel()) > 0 and two[4] == 0


@pytest.mark.parametrize("fmt,keep", (("bfloat16", 2), ("float16", 4), ("float32", 9), ("float64", 30)))
def test_fused_rounding_against_split_merge_and_compare(shafa, fmt, keep):
    T = shafa.PLANES_TILE
    x = _values(2 * T + 3, fmt, T, 4)
    t = _tensor(x, fmt)
    planes, pos, bits = shafa.round_field(t, keep, (1,))
    back = shafa.restore_rounded(planes, t.dtype, t.shape, (1,), keep, pos, bits)
    y, good = _round(x, MANT[fmt], keep)
    assert _host_bits(back).tobytes() == y.tobytes()
    fused = shafa.rounded_errors(t, [keep])[0].words()
    two = shafa.tensor_errors(back, t).words()
    _same(fused, _record(x, y, fmt, int((~good).sum())), "fused")
    for i in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11):
        assert fused[i] == two[i], (i, fused, two)
    _, outl = shafa.rounded_histograms(t, keep, [(1,)])
    assert fused[4] == int(outl.cpu()[0]) == int(pos.numel()) > 0 and two[4] == 0


def test_all_patterns_of_both_16_bit_formats(shafa):
    """65 536 bit patterns of bfloat16 and of float16 through error_round_dev at keep 0, 3 and mant: six blocks, one launch"""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    cases = [(fmt, keep) for fmt in ("bfloat16", "float16") for keep in (0, 3, MANT[fmt])]
    wants = []
    for fmt, keep in cases:
        y, good = _round(x, MANT[fmt], keep)
        wants.append(_record(x, y, fmt, int((~good).sum())))
    st = _stream()
    bt = shafa.Batch(6, 1 << 20)
    try:
        d_el, d_stat = _to(x.view(np.uint8)), _fill64(W12 * 6 + 2)
        bt.error_round_dev(st, 2, [MANT[f] for f, _ in cases], [kp for _, kp in cases], d_el, [0] * 6, [65536] * 6, _sizes([65536] * 6),
                           d_stat[1:-1])
        assert bt.finish(st, 6) == (0, [0] * 6)
        got = _whole(d_stat, wants, cases)
    finally:
        bt.close()
    assert [int(g[4]) for g in got[[2, 5]]] == [0, 0] and all(int(g[4]) > 0 for g in got[[0, 1, 3, 4]])


# ---------------------------------------------------------------- 4. word 5
def test_the_elements_past_the_bound_are_counted(shafa):
    """one element planted 3 bound off is counted, and not at abs = inf; e = rel |x| exactly is inside, one ulp more is not"""
    n, bound = 1000, 0.125
    x = (np.arange(n) % 37).astype(np.float32) * np.float32(0.5)
    y = x + np.float32(bound / 2)
    y[777] = x[777] + np.float32(3 * bound)
    xr = np.full(64, 16.0, np.float32)
    yr = xr.copy()
    yr[10], yr[20], yr[30], yr[40] = 17.0, np.nextafter(np.float32(17.0), np.float32(18)), 15.0, np.nextafter(np.float32(15.0), np.float32(0))
    xs, ys = [x, x, xr, xr], [y, y, yr, yr]
    bounds = [(bound, 0.0), (math.inf, 0.0), (0.0, 2.0 ** -4), (0.0, 0.0)]
    R, A = _Image(4, [v.view(np.uint32) for v in xs], [1, 0, 3, 2]), _Image(4, [v.view(np.uint32) for v in ys], [0] * 4)
    wants = [_record(a.view(np.uint32), b.view(np.uint32), "float32", 0, *bd) for a, b, bd in zip(xs, ys, bounds)]
    assert [w[5] for w in wants] == [1, 0, 2, 4] and wants[0][9] == 777
    st = _stream()
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_stat = _fill64(W12 * 4 + 2)
        ns = [v.size for v in xs]
        bt.error_dev(st, 4, [23] * 4, [b[0] for b in bounds], [b[1] for b in bounds], _to(A.img), A.off, ns, _sizes(ns), _to(R.img),
                     R.off, d_stat[1:-1])
        assert bt.finish(st, 4) == (0, [0] * 4)
        _whole(d_stat, wants)
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. a block past its capacity; launches behind a busy stream
@pytest.mark.parametrize("entry", ("pair", "quant", "round"))
def test_a_block_past_its_capacity(shafa, entry):
    T = shafa.PLANES_TILE
    xs = [_values(n, "float32", T, n % 5) for n in (100, T + 5, 33)]
    ys = [_came_back(x, "float32", 1) for x in xs]
    R, A = _Image(4, xs, [1, 0, 3]), _Image(4, ys, [0] * 3)
    caps = [100, T, 33]                                                    # the middle block's d_n is past its capacity
    ns = [x.size for x in xs]
    fused = lambda x, r: _record(x, r[0], "float32", int((~r[1]).sum()))
    if entry == "pair":
        wants = [_record(x, y, "float32", 0, 1e-3, 0.0) for x, y in zip(xs, ys)]
    elif entry == "quant":
        wants = [fused(x, _quant(x, 0.5, 0.25)) for x in xs]
    else:
        wants = [fused(x, _round(x, 23, 5)) for x in xs]
    wants[1] = [0] * 12
    wants[1][6] = wants[1][7] = 0.0
    st = _stream()
    bt = shafa.Batch(3, 1 << 20)
    try:
        d_stat, d_ref = _fill64(W12 * 3 + 2), _to(R.img)
        if entry == "pair":
            bt.error_dev(st, 4, [23] * 3, [1e-3] * 3, [0.0] * 3, _to(A.img), A.off, caps, _sizes(ns), d_ref, R.off, d_stat[1:-1])
        elif entry == "quant":
            bt.error_quant_dev(st, 4, [0.5] * 3, [0.25] * 3, d_ref, R.off, caps, _sizes(ns), d_stat[1:-1])
        else:
            bt.error_round_dev(st, 4, [23] * 3, [5] * 3, d_ref, R.off, caps, _sizes(ns), d_stat[1:-1])
        assert bt.finish(st, 3, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [0, shafa.OUTSIDE_MODULE, 0])
        got = _whole(d_stat, wants)
        assert got[1].tolist() == [0] * 12
    finally:
        bt.close()


def test_four_launches_behind_a_busy_stream(shafa):
    import torch
    T = shafa.PLANES_TILE
    xs = [_values(n, "float32", T, n % 7) for n in (2 * T + 3, 17, T)]
    ys = [_came_back(x, "float32", 3) for x in xs]
    R, A = _Image(4, xs, [3, 1, 0]), _Image(4, ys, [0] * 3)
    ns = [x.size for x in xs]
    w_pair = [_record(x, y, "float32", 0, 0.0, 2.0 ** -12) for x, y in zip(xs, ys)]
    w_quant = [_record(x, r[0], "float32", int((~r[1]).sum())) for x, r in ((x, _quant(x, 0.5, 0.25)) for x in xs)]
    w_r5 = [_record(x, r[0], "float32", int((~r[1]).sum())) for x, r in ((x, _round(x, 23, 5)) for x in xs)]
    w_r0 = [_record(x, r[0], "float32", int((~r[1]).sum())) for x, r in ((x, _round(x, 23, 0)) for x in xs)]
    st = _stream()
    bt = shafa.Batch(3, 1 << 20)
    try:
        d_ref, d_a, d_n = _to(R.img), _to(A.img), _sizes(ns)
        d = [_fill64(W12 * 3 + 2) for _ in range(4)]
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            busy = torch.zeros(32 << 20, dtype=torch.float32, device=_dev())
            for _ in range(8):
                busy.add_(1.0)
        bt.error_dev(st, 4, [23] * 3, [0.0] * 3, [2.0 ** -12] * 3, d_a, A.off, ns, d_n, d_ref, R.off, d[0][1:-1])
        bt.error_quant_dev(st, 4, [0.5] * 3, [0.25] * 3, d_ref, R.off, ns, d_n, d[1][1:-1])
        bt.error_round_dev(st, 4, [23] * 3, [5] * 3, d_ref, R.off, ns, d_n, d[2][1:-1])
        bt.error_round_dev(st, 4, [23] * 3, [0] * 3, d_ref, R.off, ns, d_n, d[3][1:-1])
        assert bt.finish(st, 3) == (0, [0] * 3)
        for got, want, what in zip(d, (w_pair, w_quant, w_r5, w_r0), ("pair", "quant", "round 5", "round 0")):
            _whole(got, want, what)
        assert float(busy[0].cpu()) == 8.0
    finally:
        bt.close()


# ---------------------------------------------------------------- 6. the drivers
def _field(fmt):
    """a smooth [8, 32, 48] field with a NaN and an infinity in it"""
    z, y, x = np.mgrid[0:8, 0:32, 0:48].astype(np.float64)
    f = 1000 * np.sin(x / 9) * np.cos(y / 13) * np.sin(z / 7 + 0.3)
    b = _to_bits(f.reshape(-1), fmt).copy()
    SIGN, INF, MIN = _consts(fmt)
    b[1234], b[77] = INF | (MIN >> 1), SIGN | INF
    return b


def _psnr_snr(xb, yb, fmt):
    x, y = _dbl(xb, fmt), _dbl(yb, fmt)
    fin = np.isfinite(x) & np.isfinite(y)
    x, y = x[fin], y[fin]
    mse = float(np.mean((x - y) ** 2))
    return 20 * math.log10(float(x.max() - x.min())) - 10 * math.log10(mse), 10 * math.log10(float(np.sum(x * x)) / float(np.sum((x - y) ** 2)))


def test_field_errors_and_curve_and_fit(shafa):
    fmt = "float32"
    xb = _field(fmt)
    t = _tensor(xb, fmt, (8, 32, 48))
    bounds = [1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0]
    all6 = shafa.field_errors(t, bounds)
    assert [s.words() for s in all6] == [shafa.field_errors(t, [e])[0].words() for e in bounds]
    model = []
    for e, s in zip(bounds, all6):
        y, good = _quant(xb, *shafa.fields._params("test", e, 4))
        _same(s.words(), _record(xb, y, fmt, int((~good).sum())), e)
        model.append(_psnr_snr(xb, y, fmt))
        assert s.psnr == pytest.approx(model[-1][0], rel=1e-9) and s.snr == pytest.approx(model[-1][1], rel=1e-9)
        assert s.others == 2 and s.outliers >= 2 and s.max_error <= e
    # against numpy on the decompressed tensor
    item = shafa.compress_fields(t, 0.1)[0]
    assert item.step > 0
    back = shafa.decompress_fields([item])[0]
    p, q = _psnr_snr(xb, _host_bits(back), fmt)
    assert all6[2].psnr == pytest.approx(p, rel=1e-9) and all6[2].snr == pytest.approx(q, rel=1e-9)
    curve = shafa.field_curve(t, bounds)
    rates = shafa.field_rates(t, bounds)
    assert [(e, nb, no) for e, nb, no, _ in curve] == rates and [c[3].words() for c in curve] == [s.words() for s in all6]
    assert all(c[2] == c[3].outliers for c in curve)
    psnrs = [m[0] for m in model]
    assert psnrs == sorted(psnrs, reverse=True)
    target = (psnrs[2] + psnrs[3]) / 2
    assert shafa.fit_psnr(t, target, bounds) == 0.1 and shafa.fit_psnr(t, target, bounds[::-1]) == 0.1
    assert shafa.fit_psnr(t, psnrs[5] - 1, bounds) == 100.0
    assert shafa.fit_psnr(t, 1e6, bounds) is None


@pytest.mark.parametrize("fmt", ("bfloat16", "float16", "float64"))
def test_rounded_errors_and_curve_and_fit(shafa, fmt):
    xb = _field(fmt)
    t = _tensor(xb, fmt, (8, 32, 48))
    mant = MANT[fmt]
    every = shafa.rounded_errors(t)
    assert len(every) == mant + 1
    keeps = list(range(mant + 1)) if mant < 20 else [0, 1, 2, 3, 26, 51, 52]
    assert [every[kp].words() for kp in keeps] == [shafa.rounded_errors(t, [kp])[0].words() for kp in keeps]
    snrs = {}
    for kp in keeps:
        y, good = _round(xb, mant, kp)
        _same(every[kp].words(), _record(xb, y, fmt, int((~good).sum())), kp)
        if kp < mant:
            snrs[kp] = _psnr_snr(xb, y, fmt)[1]
            assert every[kp].snr == pytest.approx(snrs[kp], rel=1e-9)
    assert every[mant].snr == math.inf and every[mant].max_error == 0.0
    item = shafa.compress_rounded(t, 3)[0]
    assert item.keep_bits == 3
    back = shafa.decompress_rounded([item])[0]
    assert every[3].snr == pytest.approx(_psnr_snr(xb, _host_bits(back), fmt)[1], rel=1e-9)
    few = [0, 3, mant]
    curve = shafa.rounded_curve(t, few)
    assert [(kp, nb, no) for kp, nb, no, _ in curve] == shafa.rounded_rates(t, few)
    assert [c[3].words() for c in curve] == [every[kp].words() for kp in few]
    cap = shafa.fields.outlier_capacity(t.numel())
    target = (snrs[2] + snrs[3]) / 2
    want = min(kp for kp in keeps if kp == mant or snrs[kp] >= target)
    assert every[3].outliers <= cap and shafa.fit_keep_bits_snr(t, target) == want == 3
    assert shafa.fit_keep_bits_snr(t, target, [5, 1, 4]) == 4
    assert shafa.fit_keep_bits_snr(t, 300.0, [0, 1, 2]) is None


def test_verify_fields_and_rounded(shafa):
    import torch
    ts = {fmt: _tensor(_field(fmt), fmt, (8, 32, 48)) for fmt in MANT}
    # a tensor compress_fields keeps lossless: float32 cannot hold 10^6 to 10^-9
    noise = _tensor(_to_bits(1e6 + np.arange(4096) * 0.37, "float32"), "float32")
    items = shafa.compress_fields([ts["float32"], ts["float64"], noise], [0.05, 1e-4, 1e-9])
    assert items[2].step == 0.0 and items[0].step > 0 and items[1].step > 0
    res = shafa.verify_fields(items, [ts["float32"], ts["float64"], noise])
    assert [ok for ok, _ in res] == [True] * 3
    assert res[2][1].max_error == 0.0 and 0 < res[0][1].max_error <= items[0].bound and 0 < res[1][1].max_error <= items[1].bound
    assert res[0][1].others == 2 and res[0][1].others_changed == 0 and res[0][1].n == 8 * 32 * 48
    # one element of the original moved by 3 bound
    moved = ts["float32"].clone()
    moved.view(-1)[5000] += 3 * items[0].bound
    (ok0, s0), (ok1, _) = shafa.verify_fields(items[:2], [moved, ts["float64"]])
    assert not ok0 and ok1 and s0.over == 1 and s0.argmax == 5000 and s0.max_error > 1.9 * items[0].bound
    # a NaN that came back with other bits
    nan = ts["float32"].clone()
    nan.view(torch.int32).view(-1)[1234] ^= 1
    ok, s = shafa.verify_fields(items[0], nan)[0]
    assert not ok and s.over == 0 and s.others_changed == 1
    # rounded items of all four dtypes, one kept lossless: denormals at keep 0 are all outliers
    den = _tensor(np.arange(1, 4097, dtype=np.uint16) % 127 + 1, "bfloat16")
    origs = [ts["bfloat16"], ts["float16"], ts["float32"], ts["float64"], den]
    ritems = shafa.compress_rounded(origs, [3, 4, 10, 20, 0])
    assert ritems[4].keep_bits is None and [it.keep_bits for it in ritems[:4]] == [3, 4, 10, 20]
    res = shafa.verify_rounded(ritems, origs)
    assert [ok for ok, _ in res] == [True] * 5 and all(s.max_error > 0 for _, s in res[:4]) and res[4][1].max_error == 0.0
    # values in [1, 2) and one original moved by 3 x 2^-(keep + 1) of itself
    flat = _tensor(_to_bits(1.0 + (np.arange(5000) % 64) / 64.0, "bfloat16"), "bfloat16")
    it = shafa.compress_rounded(flat, 3)[0]
    moved = flat.clone()
    assert float(moved[128]) == 1.0
    moved[128] = 1.0 + 3.0 / 16
    (ok, s), = shafa.verify_rounded([it], [moved])
    assert not ok and s.over == 1 and s.argmax == 128 and s.max_error == 3.0 / 16
    assert shafa.verify_rounded(it, flat)[0][0]


def test_a_mixed_list_with_an_empty_and_a_0_dimensional_tensor(shafa):
    import torch
    dev = _dev()
    xb = _field("float32")
    t = _tensor(xb, "float32")
    y, _ = _round(xb, 23, 8)
    back = _tensor(y, "float32")
    h = _tensor(_field("float16"), "float16")
    empty, scalar = torch.empty(0, dtype=torch.float64, device=dev), torch.tensor(3.0, dtype=torch.float32, device=dev)
    res = shafa.tensor_errors([empty, back, scalar, h, back[3:]], [empty, t, scalar, h, t[3:]], rel_bound=2.0 ** -9)
    none = [0] * 9 + [NONE, _b(math.inf), _b(-math.inf)]
    assert res[0].words() == none and res[2].words() == none and res[0].argmax is None and math.isnan(res[0].psnr)
    _same(res[1].words(), _record(xb, y, "float32", 0, math.inf, 2.0 ** -9), "pair")
    assert res[1].over == 0 and res[3].max_error == 0.0 and res[3].n == h.numel() and res[3].others == 2
    _same(res[4].words(), _record(xb[3:], y[3:], "float32", 0, math.inf, 2.0 ** -9), "a view that is no multiple of 16")
    one = shafa.tensor_errors(back, t, abs_bound=0.0)
    assert one.over == _record(xb, y, "float32", 0, 0.0, 0.0)[5] > 0 and one.words()[:5] == res[1].words()[:5]
    for s in shafa.field_errors(empty.float(), [1e-3, 1.0]) + shafa.rounded_errors(scalar, [0, 5]):
        assert s.words() == none

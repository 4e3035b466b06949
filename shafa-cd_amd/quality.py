"""Error statistics — what a bound costs: ErrorStats, tensor_errors, field_errors / rounded_errors, field_curve / rounded_curve,
fit_psnr / fit_keep_bits_snr and verify_fields / verify_rounded on top of Batch.error_dev / error_quant_dev / error_round_dev
(csrc/planes_lag.hip; include/shafa_hip.h: "Error statistics").

fields.py and rounding.py size every candidate bound in one read of the tensor: the rate half of a rate-distortion curve.  This
module is the distortion half.  The fused entries make what the quantising or the rounding merge would give back in registers and
fold the error of every element into one record of twelve words per (tensor, bound): RMSE, PSNR, SNR, the largest error and where
it is, the value range, and the counts of non-finite elements and outliers.  No planes, no records, no temporary.  The two-tensor
entry does the same for whatever has been decompressed already, and counts the elements past a bound abs + rel |x|: the
per-element guarantee, confirmed after the fact.

The sums are taken in a fixed order without atomics: the same tensor gives the same twelve words every time.

The drivers live in this submodule; the package re-exports them."""
import math
import sys

_pkg = sys.modules[__package__]

ERR_WORDS = 12
_NONE = (1 << 64) - 1


def _log10(v):
    return math.log10(v) if v > 0 else (-math.inf if v == 0 else math.nan)


class ErrorStats:
    """One record of the error entries, decoded: `n` elements compared; `finite` of them finite in the original and in what came
    back, `others` not (a NaN or an infinity on either side), `others_changed` of those with other bits than the original's;
    `outliers`, the elements the entry's rule gives back bit for bit (0 from the two-tensor entry); `over`, the finite elements
    with |x - y| > abs_bound + rel_bound |x| (0 from the fused entries); `sum_e2` and `sum_x2`, the sums of (x - y)^2 and of x^2
    over the finite elements; `max_e`, the largest |x - y| of them, at the flat index `max_at` (the smallest such; 2^64 - 1 where
    no element is finite); `min_x` and `max_x`, the extremes of the finite originals (inf and -inf where there is none)."""
    __slots__ = ("n", "finite", "others", "others_changed", "outliers", "over", "sum_e2", "sum_x2", "max_e", "max_at", "min_x",
                 "max_x")

    def __init__(self, words):
        import struct
        words = [int(w) & _NONE for w in words]
        if len(words) != ERR_WORDS:
            raise ValueError(f"ErrorStats: a record of {ERR_WORDS} words")
        f = lambda w: struct.unpack("<d", struct.pack("<Q", w))[0]
        self.n, self.finite, self.others, self.others_changed, self.outliers, self.over = words[:6]
        self.sum_e2, self.sum_x2, self.max_e = f(words[6]), f(words[7]), f(words[8])
        self.max_at = words[9]
        self.min_x, self.max_x = f(words[10]), f(words[11])

    @property
    def mse(self):
        """the mean squared error over the finite elements; nan where there is none"""
        return self.sum_e2 / self.finite if self.finite else math.nan

    @property
    def rmse(self):
        return math.sqrt(self.mse) if self.finite else math.nan

    @property
    def value_range(self):
        """max - min of the finite originals; nan where there is none"""
        return self.max_x - self.min_x if self.finite else math.nan

    @property
    def nrmse(self):
        """rmse / value_range; nan with no finite element or a range of 0"""
        return self.rmse / self.value_range if self.finite and self.value_range > 0 else math.nan

    @property
    def psnr(self):
        """20 log10(value_range) - 10 log10(mse) in dB: inf at mse 0, nan with no finite element or a range of 0"""
        if not self.finite or not self.value_range > 0:
            return math.nan
        if self.mse == 0:
            return math.inf
        return 20 * _log10(self.value_range) - 10 * _log10(self.mse)

    @property
    def snr(self):
        """10 log10(sum_x2 / sum_e2) in dB: inf at sum_e2 0, nan with no finite element"""
        if not self.finite:
            return math.nan
        if self.sum_e2 == 0:
            return math.inf
        return 10 * _log10(self.sum_x2) - 10 * _log10(self.sum_e2)

    @property
    def max_error(self):
        return self.max_e

    @property
    def argmax(self):
        """the flat index of the largest error, None where no element is finite"""
        return None if self.max_at == _NONE else self.max_at

    def words(self):
        """the record again"""
        import struct
        b = lambda v: struct.unpack("<Q", struct.pack("<d", v))[0]
        return [self.n, self.finite, self.others, self.others_changed, self.outliers, self.over, b(self.sum_e2), b(self.sum_x2),
                b(self.max_e), self.max_at, b(self.min_x), b(self.max_x)]

    def __repr__(self):
        return (f"ErrorStats(n={self.n}, finite={self.finite}, others={self.others}, others_changed={self.others_changed}, "
                f"outliers={self.outliers}, over={self.over}, rmse={self.rmse!r}, max_error={self.max_e!r}, argmax={self.argmax}, "
                f"range=[{self.min_x!r}, {self.max_x!r}], psnr={self.psnr!r}, snr={self.snr!r})")


def _empty():
    """the record of n = 0"""
    return ErrorStats([0] * 9 + [_NONE, 0x7FF0000000000000, 0xFFF0000000000000])


def _decode(d_stat):
    """the records of an int64 CUDA tensor [nb, 12] -> [ErrorStats]"""
    return [ErrorStats(row) for row in d_stat.cpu().view(-1, ERR_WORDS).tolist()]


# ---- the arguments
def _float_tensors(what, tensors):
    return _pkg.rounding._rounded_tensors(what, tensors)


def _one_tensor(what, t):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    return t


def _abs_bound(what, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or v < 0:
        raise ValueError(f"{what}: abs_bound is a float >= 0 or inf, not {v!r}")
    return float(v)


def _rel_bound(what, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{what}: rel_bound is a finite float >= 0, not {v!r}")
    return float(v)


def _per_tensor(what, name, v, count, check):
    if isinstance(v, (list, tuple)):
        if len(v) != count:
            raise ValueError(f"{what}: {name} is a float or a list with one float per tensor")
        return [check(what, e) for e in v]
    return [check(what, v)] * count


def _target(what, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
        raise ValueError(f"{what}: {name} is a float in dB, not {v!r}")
    return float(v)


def _pairs(what, a, ref):
    """the tensors that came back and their originals, checked: lists of equal length, dtype for dtype and shape for shape"""
    import torch
    if isinstance(a, torch.Tensor) != isinstance(ref, torch.Tensor):
        raise ValueError(f"{what}: one pair of tensors or two lists of equal length")
    As, Rs = _float_tensors(what, a), _float_tensors(what, ref)
    if len(As) != len(Rs):
        raise ValueError(f"{what}: one original per tensor")
    for x, y in zip(As, Rs):
        if x.dtype != y.dtype or x.shape != y.shape:
            raise ValueError(f"{what}: {x.dtype} {tuple(x.shape)} against an original of {y.dtype} {tuple(y.shape)}")
        if x.device != Rs[0].device:
            raise ValueError(f"{what}: the tensors are on one device")
    return As, Rs


# ---- the launches
def _pair_errors(As, Rs, abs_b, rel_b, stream):
    """error_dev over checked pairs, one launch per element size, one finish, one read-back -> [ErrorStats]"""
    import torch
    out = [None if t.numel() and t.dim() else _empty() for t in As]
    units = [(n, k) if out[i] is None else (0, k) for i, (n, k) in enumerate(_pkg._elements(As))]
    groups = _pkg._by_width(units)
    if not groups:
        return out
    dev = As[0].device
    mant = _pkg.rounding.MANTISSA_BITS
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        As = [t if t.data_ptr() % 16 == 0 else t.clone() for t in As]      # side a is a decoder's region: multiples of 16
        order = [i for _, idx in groups for i in idx]
        d_n = torch.tensor([units[i][0] for i in order], dtype=torch.int64, device=dev)
        d_stat = torch.empty((len(order), ERR_WORDS), dtype=torch.int64, device=dev)
        bt = _pkg.Batch(max(len(idx) for _, idx in groups), 1 << 20)
        try:
            at = 0
            for w, idx in groups:
                abase, rbase = min(As[i].data_ptr() for i in idx) // 16 * 16, min(Rs[i].data_ptr() for i in idx)
                numel = [units[i][0] for i in idx]
                bt.error_dev(st, w, [mant[As[i].dtype] for i in idx], [abs_b[i] for i in idx], [rel_b[i] for i in idx], abase,
                             [As[i].data_ptr() - abase for i in idx], numel, d_n[at:at + len(idx)], rbase,
                             [Rs[i].data_ptr() - rbase for i in idx], d_stat[at:at + len(idx)])
                at += len(idx)
            bt.finish(st, bt.max_blocks)
            for i, s in zip(order, _decode(d_stat)):
                out[i] = s
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return out


def _fused_errors(t, launch, count, stream):
    """one block per candidate on t's region in ONE launch (launch(bt, st, k, [0] * count, [n] * count, d_n, d_stat)), one finish,
    one read-back -> [ErrorStats]"""
    import torch
    if not t.numel() or not t.dim():
        return [_empty() for _ in range(count)]
    dev, k, n = t.device, t.element_size(), t.numel()
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        d_n = torch.full((count,), n, dtype=torch.int64, device=dev)
        d_stat = torch.empty((count, ERR_WORDS), dtype=torch.int64, device=dev)
        bt = _pkg.Batch(count, 1 << 20)
        try:
            launch(bt, st, k, [0] * count, [n] * count, d_n, d_stat)
            bt.finish(st, count)
            out = _decode(d_stat)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return out


def _keeps_of(what, t, keeps):
    if keeps is None:
        keeps = list(range(_pkg.rounding.MANTISSA_BITS[t.dtype] + 1))
    if not isinstance(keeps, (list, tuple)) or not keeps:
        raise ValueError(f"{what}: keeps is a non-empty list of ints, not {keeps!r}")
    return [_pkg.rounding._keep(what, k, t.dtype) for k in keeps]


# ---- the drivers
def tensor_errors(a, ref, abs_bound=math.inf, rel_bound=0.0, stream=None):
    """The error statistics of what came back, `a`, against the original, `ref`: one pair of contiguous CUDA tensors -> an
    ErrorStats, or two lists of equal length -> a list of them.  The tensors of a pair have one dtype — bfloat16, float16, float32
    or float64 — and one shape.  `over` counts the finite elements with |x - y| > abs_bound + rel_bound |x|: `abs_bound` a float
    >= 0 or inf, `rel_bound` a finite float >= 0, each for all pairs or in a list with one per pair.  Anything else is a ValueError
    before any device work.  An empty or 0-dimensional tensor gives the record of n = 0.  Both tensors are read where they lie
    (an `a` that is no multiple of 16 bytes is copied first); one error_dev launch per element size, one synchronisation."""
    import torch
    what = "tensor_errors"
    single = isinstance(a, torch.Tensor)
    As, Rs = _pairs(what, a, ref)
    abs_b = _per_tensor(what, "abs_bound", abs_bound, len(As), _abs_bound)
    rel_b = _per_tensor(what, "rel_bound", rel_bound, len(As), _rel_bound)
    if not As:
        return []
    out = _pair_errors(As, Rs, abs_b, rel_b, stream)
    return out[0] if single else out


def field_errors(t, abs_errors, stream=None):
    """What compress_fields(t, abs_error) would cost in accuracy for every abs_error of the non-empty list `abs_errors`, without
    compressing: one ErrorStats per bound, of the float32 or float64 CUDA tensor `t` against what decompress_fields would give
    back — the restored value where it keeps the bound, the element's own bits where it is an outlier (`outliers` counts those).
    Step and bound are compress_fields'.  One block per bound on the same region, in ONE error_quant_dev launch; one
    synchronisation.  compress_fields' ValueErrors, before any device work."""
    what = "field_errors"
    t = _pkg.fields._field_tensors(what, _one_tensor(what, t))[0]
    params = _pkg.fields._bounds(what, abs_errors, t.element_size())
    return _fused_errors(t, lambda bt, st, k, off, cap, d_n, d_stat: bt.error_quant_dev(
        st, k, [p[0] for p in params], [p[1] for p in params], t, off, cap, d_n, d_stat), len(params), stream)


def rounded_errors(t, keeps=None, stream=None):
    """field_errors for compress_rounded: one ErrorStats per number of kept bits of the list `keeps` (None: every one from 0 to
    MANTISSA_BITS[dtype]) of the bfloat16, float16, float32 or float64 CUDA tensor `t`.  One block per keep on the same region, in
    ONE error_round_dev launch; one synchronisation."""
    what = "rounded_errors"
    t = _float_tensors(what, _one_tensor(what, t))[0]
    keeps = _keeps_of(what, t, keeps)
    mant = _pkg.rounding.MANTISSA_BITS[t.dtype]
    return _fused_errors(t, lambda bt, st, k, off, cap, d_n, d_stat: bt.error_round_dev(
        st, k, [mant] * len(keeps), keeps, t, off, cap, d_n, d_stat), len(keeps), stream)


def field_curve(t, abs_errors, lags=None, axes=None):
    """The rate-distortion curve of one tensor under absolute bounds: [(abs_error, nbytes, outliers, ErrorStats)] in the order of
    `abs_errors` — field_rates' entries with field_errors' behind them: that call and one error launch."""
    rates = _pkg.fields.field_rates(t, abs_errors, lags, axes)
    return [(e, nb, no, s) for (e, nb, no), s in zip(rates, field_errors(t, abs_errors))]


def rounded_curve(t, keeps=None, lags=None, axes=None):
    """The rate-distortion curve of one tensor over kept mantissa bits: [(keep_bits, nbytes, outliers, ErrorStats)] —
    rounded_rates' entries with rounded_errors' behind them: that call and one error launch.  keeps=None: every keep."""
    what = "rounded_curve"
    keeps = _keeps_of(what, _float_tensors(what, _one_tensor(what, t))[0], keeps)
    rates = _pkg.rounding.rounded_rates(t, keeps, lags, axes)
    return [(k, nb, no, s) for (k, nb, no), s in zip(rates, rounded_errors(t, keeps))]


def fit_psnr(t, min_psnr, abs_errors):
    """The LARGEST abs_error of the list `abs_errors` at which the tensor keeps a PSNR of at least `min_psnr` dB with no more
    outliers than fields.outlier_capacity(numel) (compress_fields would keep it lossless otherwise); None where none does.
    field_errors' arguments and launch."""
    what = "fit_psnr"
    min_psnr = _target(what, "min_psnr", min_psnr)
    stats = field_errors(t, abs_errors)
    cap = _pkg.fields.outlier_capacity(t.numel())
    fits = [e for e, s in zip(abs_errors, stats) if s.psnr >= min_psnr and s.outliers <= cap]
    return max(fits) if fits else None


def fit_keep_bits_snr(t, min_snr, keeps=None):
    """The SMALLEST number of kept bits of the list `keeps` (None: every one) at which the tensor keeps an SNR of at least
    `min_snr` dB with no more outliers than fields.outlier_capacity(numel); None where none does.  rounded_errors' arguments and
    launch."""
    what = "fit_keep_bits_snr"
    min_snr = _target(what, "min_snr", min_snr)
    keeps = _keeps_of(what, _float_tensors(what, _one_tensor(what, t))[0], keeps)
    stats = rounded_errors(t, keeps)
    cap = _pkg.fields.outlier_capacity(t.numel())
    fits = [k for k, s in zip(keeps, stats) if s.snr >= min_snr and s.outliers <= cap]
    return min(fits) if fits else None


def _verify(what, kind, items, originals, bounds_of, decompress):
    import torch
    if isinstance(items, kind):
        items = [items]
    if isinstance(originals, torch.Tensor):
        originals = [originals]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, kind) for it in items):
        raise ValueError(f"{what}: a {kind.__name__} or a list of them")
    if not isinstance(originals, (list, tuple)) or len(originals) != len(items):
        raise ValueError(f"{what}: one original per item")
    Rs = _float_tensors(what, list(originals))
    for it, r in zip(items, Rs):
        if it.dtype != r.dtype or tuple(it.shape) != tuple(r.shape):
            raise ValueError(f"{what}: an item of {it.dtype} {tuple(it.shape)} against an original of {r.dtype} {tuple(r.shape)}")
    bounds = [bounds_of(it) for it in items]
    if not items:
        return []
    back = decompress(list(items))
    stats = _pair_errors([b.contiguous() for b in back], Rs, [b[0] for b in bounds], [b[1] for b in bounds], None)
    return [(s.over == 0 and s.others_changed == 0, s) for s in stats]


def verify_fields(items, originals):
    """Does every element of compress_fields' `items` come back within its item's bound?  Decompresses the items and compares
    each with its original (`originals`: the tensors, in the items' order, on the items' device) in one error_dev launch per
    element size, with abs_bound = the item's `bound` and rel_bound = 0; an item kept lossless: both 0.  Returns [(ok, ErrorStats)],
    ok exactly when no finite element errs by more than the bound (`over` == 0) and every NaN and infinity came back bit for bit
    (`others_changed` == 0).  The threshold is exact: e <= bound is one comparison of doubles."""
    def bounds_of(it):
        if not (it.step == 0.0 or (math.isfinite(it.bound) and it.bound > 0)):
            raise ValueError(f"verify_fields: an item's bound is a finite float > 0, not {it.bound!r}")
        return (0.0, 0.0) if it.step == 0.0 else (it.bound, 0.0)
    return _verify("verify_fields", _pkg.fields.CompressedField, items, originals, bounds_of, _pkg.fields.decompress_fields)


def verify_rounded(items, originals):
    """verify_fields for compress_rounded's items: abs_bound = 0 and rel_bound = 2^-(keep_bits + 1), the guarantee of a normal
    element; an item kept lossless (keep_bits None): both 0.  Zeros, good denormals, infinities and NaNs come back as they were
    (-0.0 as +0.0, an error of 0) and outliers bit for bit, so the one threshold serves them all.  The threshold rel |x| is one
    double multiplication: exact for bfloat16, float16 and float32 elements; at float64 it can round for |x| within 2^53 of the
    smallest normal, where the product is denormal.  No other case is inexact."""
    def bounds_of(it):
        if it.keep_bits is None:
            return (0.0, 0.0)
        return (0.0, 2.0 ** -(_pkg.rounding._keep("verify_rounded", it.keep_bits, it.dtype) + 1))
    return _verify("verify_rounded", _pkg.rounding.CompressedRounded, items, originals, bounds_of,
                   _pkg.rounding.decompress_rounded)

"""Point-wise relative bounds — "keep k mantissa bits": round_field / restore_rounded, compress_rounded / decompress_rounded and the
sizes without the planes (rounded_histograms, rounded_sizes, rounded_rates, fit_keep_bits) on top of
Batch.split_planes_grid_round_dev / merge_planes_grid_round_dev / hist_planes_grid_round_dev (csrc/planes_lag.hip;
include/shafa_hip.h: "Point-wise relative bounds").

compress_fields bounds the ABSOLUTE error of float32 and float64 fields.  A field that spans decades, and the bfloat16 and float16
tensors torch users hold on the device, want a bound relative to each element instead: the mantissa rounded to `keep_bits` bits,
half to even, the carry free to enter the exponent.  That is integer work on the element's own bits, so the guarantee is exact:
a normal element comes back within 2^-(keep_bits + 1) of itself, relatively; zeros, infinities and the NaNs and denormals that
lose no set bit come back as they were (-0.0 as +0.0); the few elements the rounding cannot keep — a value that rounds up to Inf,
a denormal or a NaN with a dropped bit set — are outliers, kept with their own bits.  The rounding runs inside the Lorenzo split,
so no temporary of codes exists; noise wants no differences at all, and lags=() gives that.

The drivers live in this submodule; the package re-exports them.  What is the rounding's own is here: its argument checks, its
item and its Quantiser, the three Batch entries with their rows of (mantissa width, kept bits).  The chains — split, merge,
compress, decompress, sizes and rates — are fields.py's, written for any Quantiser, the histogram loop and the order-0 model
grids.py's; all are reached through the package at the time of the call."""
import collections.abc
import sys

_pkg = sys.modules[__package__]


class _MantissaBits(collections.abc.Mapping):
    """dtype -> the format's mantissa width; the dtypes are looked up at the first use, so that the package imports without
    torch as it did"""
    _bits = None

    def _table(self):
        if self._bits is None:
            import torch
            type(self)._bits = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23, torch.float64: 52}
        return self._bits

    def __getitem__(self, dtype):
        return self._table()[dtype]

    def __iter__(self):
        return iter(self._table())

    def __len__(self):
        return len(self._table())

    def __repr__(self):
        return repr(self._table())


MANTISSA_BITS = _MantissaBits()


class CompressedRounded:
    """A float16, bfloat16, float32 or float64 tensor compressed with `keep_bits` of its mantissa kept (compress_rounded), in
    memory: `dtype` and `shape` of the original, `lags` as CompressedGrid's or () for no differences, `planes` as CompressedGrid's,
    of the zigzag-folded differences of the codes, `outlier_pos` (int64, sorted) and `outlier_bits` (int64, the element's bits in
    the low bits) — the elements given back bit for bit — and `nbytes`, the planes' bytes plus (8 + element size) per outlier.
    `keep_bits = None` marks a tensor kept LOSSLESS: its planes are compress_grids', it has no outliers.  decompress_rounded alone
    gives the tensor back."""
    __slots__ = ("dtype", "shape", "lags", "keep_bits", "planes", "outlier_pos", "outlier_bits", "nbytes")

    def __init__(self, dtype, shape, lags, keep_bits, planes, outlier_pos, outlier_bits, nbytes):
        self.dtype, self.shape, self.lags, self.keep_bits = dtype, tuple(shape), tuple(lags), keep_bits
        self.planes, self.outlier_pos, self.outlier_bits, self.nbytes = list(planes), outlier_pos, outlier_bits, int(nbytes)

    def __repr__(self):
        kinds = ["raw" if not isinstance(p, dict) else "+".join(sorted(p)) for p in self.planes]
        return (f"CompressedRounded({self.dtype}, {self.shape}, lags={self.lags}, keep_bits={self.keep_bits}, planes={kinds}, "
                f"outliers={int(self.outlier_pos.numel())}, nbytes={self.nbytes})")


# ---- the arguments
def _rounded_tensors(what, tensors):
    ts = _pkg._plane_tensors(what, tensors)
    for t in ts:
        if t.dtype not in MANTISSA_BITS:
            raise ValueError(f"{what}: float16, bfloat16, float32 and float64 tensors, not {t.dtype}")
    return ts


def _keep(what, keep, dtype):
    """a number of kept bits for a dtype, checked"""
    mant = MANTISSA_BITS[dtype]
    if isinstance(keep, bool) or not isinstance(keep, int) or not 0 <= keep <= mant:
        raise ValueError(f"{what}: keep_bits is an int 0 .. {mant} for {dtype}, not {keep!r}")
    return keep


def _keeps(what, ts, keep_bits):
    """one keep per checked tensor from `keep_bits`, an int for all tensors or a list with one per tensor"""
    if isinstance(keep_bits, (list, tuple)):
        if len(keep_bits) != len(ts):
            raise ValueError(f"{what}: keep_bits is an int or a list with one int per tensor")
        return [_keep(what, k, t.dtype) for k, t in zip(keep_bits, ts)]
    return [_keep(what, keep_bits, t.dtype) for t in ts]


def _lag_set(what, lags):
    """a tuple of lags as split_grid takes them, or (): no differences"""
    if isinstance(lags, (list, tuple)) and len(lags) == 0:
        return ()
    return _pkg.grids._lag_tuple(what, lags)


def _rounded_lags(what, ts, axes, lags):
    """grids._lags with () legal, for all tensors or in a list with one entry per tensor"""
    if lags is None:
        return _pkg.grids._lags(what, ts, axes, None)
    if isinstance(lags, list):
        if len(lags) != len(ts) or any(isinstance(x, int) for x in lags):
            raise ValueError(f"{what}: lags is a tuple of ints or a list with one tuple per tensor")
        return [_lag_set(what, g) for g in lags]
    return [_lag_set(what, lags)] * len(ts)


def _rows(dtypes, keeps):
    """the rounding quantiser's rows: (the dtype's mantissa width, the kept bits) per tensor or entry"""
    return [(MANTISSA_BITS[d], k) for d, k in zip(dtypes, keeps)]


# ---- the quantiser: the chains are fields.py's, with these three entries and this item
def _rounded_item(t, lags, row, lossless, planes, pos, bits, nbytes):
    """a keep_bits of None says lossless"""
    return CompressedRounded(t.dtype, t.shape, lags, None if lossless else row[1], planes, pos, bits, nbytes)


def _hist(bt, st, w, lags, rows, base, offs, numel, *out):
    """() among a histogram's candidates is the split's: a lag at the capacity, not grid_histograms' plain planes"""
    bt.hist_planes_grid_round_dev(st, w, [_pkg.fields._device_lags(g, n) for g, n in zip(lags, numel)], [r[0] for r in rows],
                                  [r[1] for r in rows], base, offs, numel, *out)


_ROUND = _pkg.fields.Quantiser(
    split=lambda bt, st, w, lags, rows, *rest: bt.split_planes_grid_round_dev(st, w, lags, [r[0] for r in rows],
                                                                              [r[1] for r in rows], *rest),
    merge=lambda bt, st, w, lags, rows, *rest: bt.merge_planes_grid_round_dev(st, w, lags, [r[0] for r in rows],
                                                                              [r[1] for r in rows], *rest),
    hist=_hist, item=_rounded_item)


# ---- one tensor, no coder
def round_field(t, keep_bits, lags):
    """The byte planes of the Lorenzo differences of a float CUDA tensor's CODES with `keep_bits` of its mantissa kept, and its
    outliers: (planes, positions, bits).  `planes` is split_grid's [k, numel] uint8 tensor over the codes — sign and the magnitude
    bits rounded half to even and shifted down by the dropped bits, as integers of the element's width; `positions` (int64,
    sorted) and `bits` (int64) are the elements the rounding cannot keep: restore_rounded gives those back bit for bit and every
    other within 2^-(keep_bits + 1) of itself.  `lags` as split_grid takes them, or () for no differences.  One
    split_planes_grid_round_dev launch, a second one with room for every outlier found where fields.outlier_capacity's records
    were too few; one synchronisation each."""
    import torch
    what = "round_field"
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    t = _rounded_tensors(what, t)[0]
    keep = _keep(what, keep_bits, t.dtype)
    lags = _lag_set(what, lags)
    return _pkg.fields._quantise_one(_ROUND, t, lags, (MANTISSA_BITS[t.dtype], keep))


def restore_rounded(planes, dtype, shape, lags, keep_bits, positions, bits, stream=None):
    """round_field's inverse for one tensor: `planes` as merge_grid takes them -> a tensor of `dtype` and `shape`, every element
    the rounded value of its code but the outliers, whose `bits` are stored at their `positions`.  One
    merge_planes_grid_round_dev call, one synchronisation."""
    what = "restore_rounded"
    if dtype not in MANTISSA_BITS:
        raise ValueError(f"{what}: float16, bfloat16, float32 and float64 tensors, not {dtype!r}")
    k, shape, n = _pkg._plane_dtype(what, dtype, shape)
    lags = _lag_set(what, lags)
    keep = _keep(what, keep_bits, dtype)
    return _pkg.fields._restore_one(_ROUND, what, planes, dtype, shape, k, n, lags, (MANTISSA_BITS[dtype], keep), positions, bits,
                                    stream)


# ---- the drivers
def compress_rounded(tensors, keep_bits, axes=None, lags=None, block_size=8 << 20, stream=None):
    """compress_grids for float16, bfloat16, float32 and float64 tensors with `keep_bits` MANTISSA BITS KEPT: every normal element
    comes back within 2^-(keep_bits + 1) of itself, relatively, or bit for bit.  `tensors`, `axes`, `lags` and `block_size` as
    compress_grids takes them, and its argument ValueErrors; `lags=()`, or () in a list with one entry per tensor, means NO
    differences — what noise such as weights wants.  Any other dtype is a ValueError.  `keep_bits` is an int for all tensors or a
    list with one per tensor, 0 .. MANTISSA_BITS[dtype]: a ValueError otherwise, before any device work.  Returns one
    CompressedRounded per tensor, which decompress_rounded gives back.

    The transform is the rule of include/shafa_hip.h, "Point-wise relative bounds": the magnitude bits rounded half to even at
    the lowest kept bit and shifted down, the sign put back as the sign of an integer.  +-Inf, +0.0, and the NaNs and denormals
    that lose no set bit come back as they were, -0.0 as +0.0.  A value that rounds up to Inf, a denormal and a NaN with a dropped
    bit set are OUTLIERS, kept as {position, bits} and given back bit for bit.  keep_bits = MANTISSA_BITS[dtype] changes nothing
    but -0.0.

    A tensor that finds more outliers than fields.outlier_capacity(numel) is kept LOSSLESS, compress_grids' planes and a
    `keep_bits` of None.

    What a number of bits costs can be asked first without compressing: rounded_sizes ranks the candidates' lags, rounded_rates
    and fit_keep_bits size a list of keeps.

    Chain: compress_fields' — one split_planes_grid_round_dev per element size over all tensors, one finish and one read-back of
    the outlier counts (the tensors kept lossless then take one split_planes_grid_dev per element size and a finish) ->
    compressed_sizes -> compress_many; a tensor's records are sorted by position."""
    what = "compress_rounded"
    ts = _rounded_tensors(what, tensors)
    lags = _rounded_lags(what, ts, axes, lags)
    keeps = _keeps(what, ts, keep_bits)
    return _pkg.fields._compress(what, _ROUND, ts, lags, _rows([t.dtype for t in ts], keeps), block_size, stream)


def decompress_rounded(items, stream=None):
    """compress_rounded's inverse: `items` is a CompressedRounded or a list of them (their planes on one device) -> the list of
    tensors, each normal element within 2^-(keep_bits + 1) of the original, relatively, or bit for bit: the outliers, and every
    element of an item kept lossless (a `keep_bits` of None).

    Chain: decompress_fields', with one merge_planes_grid_round_dev per element size over the rounded items.  Anything that is
    not a CompressedRounded is refused with a ValueError before any device work, as is an item whose dtype, lags, keep_bits or
    outliers are malformed, a lossless item that carries outliers among them.  decompress_tensors' errors otherwise."""
    what = "decompress_rounded"
    if isinstance(items, CompressedRounded):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedRounded) for it in items):
        raise ValueError(f"{what}: a CompressedRounded or a list of them (compress_rounded's items)")
    lags, rows = [], []
    for it in items:
        if it.dtype not in MANTISSA_BITS:
            raise ValueError(f"{what}: float16, bfloat16, float32 and float64 tensors, not {it.dtype!r}")
        lags.append(_lag_set(what, it.lags))
        _pkg.fields._records(what, it.outlier_pos, it.outlier_bits, None)
        if it.keep_bits is None and it.outlier_pos.numel():
            raise ValueError(f"{what}: an item kept lossless has no outliers")
        rows.append(None if it.keep_bits is None else (MANTISSA_BITS[it.dtype], _keep(what, it.keep_bits, it.dtype)))
    return _pkg.fields._decompress(what, _ROUND, items, lags, rows, stream)


# ---- sizes at a number of kept bits: the rounding split's histograms without the planes (Batch.hist_planes_grid_round_dev)
def rounded_histograms(t, keep_bits, lag_sets, stream=None):
    """The byte histograms of the planes round_field(t, keep_bits, lags) would give for every `lags` of the list `lag_sets`, and
    its count of outliers, without the planes and without the records: `t` a contiguous float CUDA tensor, every entry of
    `lag_sets` a tuple round_field takes, () among them, and `keep_bits` an int for all entries or a list with one per entry.
    Returns (freq, outliers): int64 CUDA tensors [len(lag_sets), k, 256], every row summing to t.numel(), and [len(lag_sets)].  One
    hist_planes_grid_round_dev launch per HIST_GROUP candidates, one block per candidate on the same region, one
    synchronisation."""
    import torch
    what = "rounded_histograms"
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    t = _rounded_tensors(what, t)[0]
    if not isinstance(lag_sets, (list, tuple)):
        raise ValueError(f"{what}: lag_sets is a list of tuples of lags, not {lag_sets!r}")
    sets = []
    for c in lag_sets:
        if not isinstance(c, tuple):
            raise ValueError(f"{what}: an entry of lag_sets is a tuple of lags, () for no differences, not {c!r}")
        sets.append(_lag_set(what, c))
    if isinstance(keep_bits, (list, tuple)):
        if len(keep_bits) != len(sets):
            raise ValueError(f"{what}: keep_bits is an int or a list with one int per entry of lag_sets")
        keeps = [_keep(what, e, t.dtype) for e in keep_bits]
    else:
        keeps = [_keep(what, keep_bits, t.dtype)] * len(sets)
    return _pkg.grids._histograms(_ROUND.hist, t, sets, _rows([t.dtype] * len(sets), keeps), True, stream)


def _rounded_candidates(what, ts, axes, candidates):
    """one list of candidates per checked tensor: grid_sizes' `candidates`, () — no differences — among them, or else () and every
    subset of each tensor's axis lags"""
    return _pkg.grids._candidates(what, ts, axes, candidates)


def rounded_sizes(tensors, keep_bits, axes=None, candidates=None, stream=None):
    """How large would compress_rounded make each tensor with each candidate's lags, at its keep_bits?  Per tensor a list of
    (lags, nbytes, outliers), sorted by field_sizes' key (outliers > fields.outlier_capacity(numel), nbytes, len(lags), lags): the
    first entry is the candidate to take.  `tensors`, `keep_bits` and `axes` as compress_rounded takes them, and its ValueErrors,
    before any device work.  `candidates` as grid_sizes takes them; a candidate of () is legal here and means no differences;
    None: () and every subset of the tensor's axis lags, at most eight.  An empty or 0-dimensional tensor gives [((), 0, 0)].

    nbytes is field_sizes' order-0 model over the planes the rounding split would write, with its caveats.

    Chain: per element size one hist_planes_grid_round_dev over all tensors' candidates, one block per candidate on its tensor's
    region -> sf_build_codes -> sf_encoded_size_dev -> one finish, one read-back of the sizes and the counts."""
    what = "rounded_sizes"
    ts = _rounded_tensors(what, tensors)
    cands = _rounded_candidates(what, ts, axes, candidates)
    keeps = _keeps(what, ts, keep_bits)
    return _pkg.fields._sizes(_ROUND, ts, cands, _rows([t.dtype for t in ts], keeps), stream)


def _rates(what, t, keeps, lags, axes, stream):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    ts = _rounded_tensors(what, t)
    g = _rounded_lags(what, ts, axes, lags)[0]
    if keeps is None:
        keeps = list(range(MANTISSA_BITS[ts[0].dtype] + 1))
    if not isinstance(keeps, (list, tuple)) or not keeps:
        raise ValueError(f"{what}: keeps is a non-empty list of ints, not {keeps!r}")
    keeps = [_keep(what, k, ts[0].dtype) for k in keeps]
    return _pkg.fields._rate_list(_ROUND, ts[0], g, keeps, _rows([ts[0].dtype] * len(keeps), keeps), stream)


def rounded_rates(t, keeps, lags=None, axes=None, stream=None):
    """The rate of one tensor over a list of kept bits: [(keep_bits, nbytes, outliers)] in the order of `keeps`, a non-empty list
    of ints as compress_rounded takes one.  `lags` as compress_rounded takes them for one tensor, () among them; None: the
    tensor's axis lags (`axes`).  nbytes and outliers are rounded_sizes' model; an entry with more outliers than
    fields.outlier_capacity(numel) is one compress_rounded would keep lossless.  One block per keep on the same region, in ONE
    hist_planes_grid_round_dev launch.  An empty or 0-dimensional tensor gives 0 bytes at every keep."""
    if keeps is None:
        raise ValueError(f"rounded_rates: keeps is a non-empty list of ints, not {keeps!r}")
    return _rates("rounded_rates", t, keeps, lags, axes, stream)


def fit_keep_bits(t, max_bytes, keeps=None, lags=None, axes=None, stream=None):
    """The LARGEST number of kept bits of the list `keeps` (None: every one from 0 to MANTISSA_BITS[dtype], in one launch) at which
    the tensor fits `max_bytes` (an int >= 0): rounded_rates' nbytes <= max_bytes, with no more outliers than
    fields.outlier_capacity(numel).  None where none fits.  rounded_rates' arguments, chain and caveats."""
    what = "fit_keep_bits"
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 0:
        raise ValueError(f"{what}: max_bytes is an int >= 0, not {max_bytes!r}")
    rates = _rates(what, t, keeps, lags, axes, stream)
    n = t.numel()
    fits = [k for k, nb, no in rates if nb <= max_bytes and no <= _pkg.fields.outlier_capacity(n)]
    return max(fits) if fits else None

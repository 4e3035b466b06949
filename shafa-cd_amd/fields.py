"""Error-bounded float fields — the quantiser in front of the Lorenzo differences and the restorer behind them: quantize_field /
restore_field and compress_fields / decompress_fields on top of Batch.split_planes_grid_quant_dev / merge_planes_grid_quant_dev
(csrc/planes_lag.hip; include/shafa_hip.h: "Error-bounded fields").

compress_grids takes a field bit for bit, and the Lorenzo differences of raw float bit patterns leave every mantissa byte raw.
Under an absolute error bound chosen by the caller each value becomes the integer rint(x / step) first, as in the scientific-
data codecs the predictor was taken from, and those integers are differenced exactly: that is where their factors come from.
The quantiser runs inside the grid split, so no temporary of codes exists, and the bound is CHECKED per element on the device
against the very value the decoder will make: an element that misses it — a NaN, an infinity, a value past the code range, a
tie the rounding threw over — is an outlier, kept with its own bits and given back bit for bit.

What a bound costs is the data's to say: field_histograms / field_sizes / choose_field_lags / field_rates / fit_abs_error on top
of Batch.hist_planes_grid_quant_dev count the planes the quantising split would write, and its outliers, without making either,
and give the size under an order-0 model: which lags to take under a bound, the size at each bound of a list, the smallest bound
that fits a budget.

The drivers live in this submodule; the package re-exports them.  Their chains are written for any Quantiser — this module's and
rounding.py's, which keeps its checks, its item and its three entries and calls in here.  The histogram loop and the order-0 model
are grids.py's, the coder's half of the chain (_coded_planes) and the decode chain (_merge_items) the package's, all reached
through the package at the time of the call."""
import collections
import fractions
import math
import sys

import numpy as np

_pkg = sys.modules[__package__]

FIELD_SLACK = 2.0 ** -7         # step = 2 abs_error (1 - FIELD_SLACK): keeps the ties of the restored value inside the bound


class CompressedField:
    """A float32 or float64 tensor compressed under an absolute error bound (compress_fields), in memory: `dtype` and `shape` of
    the original, `lags` as CompressedGrid's, `abs_error` as the caller gave it, `step` and `bound` — the quantiser's step and
    the bound every restored element was checked against, both exactly representable in the dtype — `planes` as CompressedGrid's,
    of the zigzag-folded differences of the codes, `outlier_pos` (int64, sorted) and `outlier_bits` (int64, the element's bits in
    the low bits) — the elements given back bit for bit — and `nbytes`, the planes' bytes plus (8 + element size) per outlier.
    A `step` of 0.0 marks a tensor kept LOSSLESS: its planes are compress_grids', it has no outliers.  decompress_fields alone
    gives the tensor back."""
    __slots__ = ("dtype", "shape", "lags", "abs_error", "step", "bound", "planes", "outlier_pos", "outlier_bits", "nbytes")

    def __init__(self, dtype, shape, lags, abs_error, step, bound, planes, outlier_pos, outlier_bits, nbytes):
        self.dtype, self.shape, self.lags, self.abs_error = dtype, tuple(shape), lags, float(abs_error)
        self.step, self.bound, self.planes = float(step), float(bound), list(planes)
        self.outlier_pos, self.outlier_bits, self.nbytes = outlier_pos, outlier_bits, int(nbytes)

    def __repr__(self):
        kinds = ["raw" if not isinstance(p, dict) else "+".join(sorted(p)) for p in self.planes]
        return (f"CompressedField({self.dtype}, {self.shape}, lags={self.lags}, abs_error={self.abs_error}, step={self.step}, "
                f"planes={kinds}, outliers={int(self.outlier_pos.numel())}, nbytes={self.nbytes})")


# ---- the step and the bound of an abs_error
def _down(v, k):
    """the largest float of k bytes that is <= the positive Fraction v, as a Python float"""
    f = float(v)                                     # the nearest double
    if fractions.Fraction(f) > v:
        f = math.nextafter(f, 0.0)
    if k == 4:
        with np.errstate(over="ignore"):
            g = np.float32(f)
        if float(g) > f:
            g = np.nextafter(g, np.float32(0))
        f = float(g)
    return f


def _legal(v, k):
    """a step or a bound the entries take: finite, normal in the element type and > 0"""
    tiny = float(np.finfo(np.float32 if k == 4 else np.float64).tiny)
    return math.isfinite(v) and v >= tiny


def _inverse(step, k):
    """T(1 / step): the double division, rounded once to float32 at 4 bytes"""
    with np.errstate(over="ignore"):
        return float(np.float32(1.0 / step)) if k == 4 else 1.0 / step


def _params(what, abs_error, k):
    """(step, bound) for an abs_error and an element size: step = 2 abs_error (1 - FIELD_SLACK) and bound = abs_error, each
    rounded DOWN into the element type; a ValueError where the entries would refuse them"""
    if isinstance(abs_error, bool) or not isinstance(abs_error, (int, float)) or not math.isfinite(abs_error) or not abs_error > 0:
        raise ValueError(f"{what}: abs_error is a finite float > 0, not {abs_error!r}")
    e = fractions.Fraction(abs_error)
    step, bound = _down(2 * e * (1 - fractions.Fraction(FIELD_SLACK)), k), _down(e, k)
    if not _legal(step, k) or not _legal(bound, k):
        raise ValueError(f"{what}: an abs_error of {abs_error!r} is below what elements of {k} bytes resolve")
    inv = _inverse(step, k)
    if not math.isfinite(inv) or inv == 0:
        raise ValueError(f"{what}: an abs_error of {abs_error!r} has no inverse step in elements of {k} bytes")
    return step, bound


def _field_tensors(what, tensors):
    import torch
    ts = _pkg._plane_tensors(what, tensors)
    for t in ts:
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: float32 and float64 tensors, not {t.dtype}")
    return ts


def _abs_errors(what, ts, abs_error):
    """one (step, bound) per checked tensor from `abs_error`, a float for all tensors or a list with one per tensor"""
    if isinstance(abs_error, (list, tuple)):
        if len(abs_error) != len(ts):
            raise ValueError(f"{what}: abs_error is a float or a list with one float per tensor")
        errs = list(abs_error)
    else:
        errs = [abs_error] * len(ts)
    return errs, [_params(what, e, t.element_size()) for e, t in zip(errs, ts)]


def outlier_capacity(numel):
    """the records compress_fields gives a tensor: one that finds more is kept lossless"""
    return 16 + numel // 64


# ---- a quantiser, and the chains every quantiser shares
# What differs between the quantising split and the rounding one (rounding.py) is data.  A tensor's parameters are its ROW, opaque
# to the chains below: (step, bound) here, (mantissa width, kept bits) there; None marks a tensor that goes, or went, without the
# quantiser — kept lossless.  `split`, `merge` and `hist` make the Batch call of one launch, f(bt, st, width, lags, rows, *rest):
# they lay the launch's rows out as their entry takes them and hand the rest on as it is (`hist` is grids._histograms' and
# grids._model_sizes').  `item(t, lags, row, lossless, planes, positions, bits, nbytes)` builds the driver's item for a tensor, and
# with it the way the item says that it was kept lossless.
Quantiser = collections.namedtuple("Quantiser", "split merge hist item")


def _field_item(t, lags, row, lossless, planes, pos, bits, nbytes):
    """compress_fields' rows carry the caller's abs_error behind step and bound; a step of 0.0 says lossless"""
    step, bound = (0.0, 0.0) if lossless else row[:2]
    return CompressedField(t.dtype, t.shape, lags, row[2], step, bound, planes, pos, bits, nbytes)


_QUANT = Quantiser(
    split=lambda bt, st, w, lags, rows, *rest: bt.split_planes_grid_quant_dev(st, w, lags, [r[0] for r in rows],
                                                                              [r[1] for r in rows], *rest),
    merge=lambda bt, st, w, lags, rows, *rest: bt.merge_planes_grid_quant_dev(st, w, lags, [r[0] for r in rows], *rest),
    hist=lambda bt, st, w, lags, rows, *rest: bt.hist_planes_grid_quant_dev(st, w, lags, [r[0] for r in rows],
                                                                            [r[1] for r in rows], *rest),
    item=_field_item)


def _device_lags(lags, numel):
    """the row of lags the entries get: () — rounding.py's "no differences" — is a lag at the capacity, which subtracts nothing in
    split and merge alike"""
    return tuple(lags) if len(lags) else (max(int(numel), 1),)


def _layout(units):
    """_split_into's planes buffer: each tensor's plane offsets, multiples of 16, and the buffer's bytes"""
    poff, pos = [], 0
    for n, w in units:
        step = _pkg._al16(n)
        poff.append([pos + j * step for j in range(w)])
        pos += w * step
    return poff, pos + 16


def _split(q, bt, st, dev, ts, units, lags, rows, caps, buf, poff):
    """one split of the quantiser q per element size over ts into buf -> (the records buffer [sum caps, 2], each tensor's first
    record, the counts of outliers found, one per tensor of the launches in their order, and that order)"""
    import torch
    first, pos = [], 0
    for c in caps:
        first.append(pos)
        pos += c
    d_outl = torch.empty((pos, 2), dtype=torch.int64, device=dev)
    groups = _pkg._by_width(units)
    order = [i for _, idx in groups for i in idx]
    d_n = torch.tensor([units[i][0] for i in order], dtype=torch.int64, device=dev)
    d_found = torch.zeros(len(order), dtype=torch.int64, device=dev)
    at = 0
    for w, idx in groups:
        base = min(ts[i].data_ptr() for i in idx)
        q.split(bt, st, w, [_device_lags(lags[i], units[i][0]) for i in idx], [rows[i] for i in idx], base,
                [ts[i].data_ptr() - base for i in idx], [units[i][0] for i in idx], d_n[at:at + len(idx)], buf,
                [o for i in idx for o in poff[i]], d_outl if pos else None, [first[i] for i in idx], [caps[i] for i in idx],
                d_found[at:at + len(idx)])
        at += len(idx)
    return d_outl, first, d_found, order


def _sorted_records(rec):
    """the records [count, 2] -> (positions, bits), sorted by position"""
    import torch
    pos, by = torch.sort(rec[:, 0])
    return pos, rec[:, 1][by].clone()


def _merge(q, records, rows):
    """_merge_into's stand-in for the decode chain (_merge_items) over tensors with the outliers records[i] = (positions, bits):
    those kept lossless (a row of None) through _merge_into as decompress_grids' go, the others through one merge of the
    quantiser q per element size"""
    def merge_into(bt, st, dev, planes, outs, units, kind, lags):
        import torch
        lags = [_device_lags(g, n) for g, (n, _) in zip(lags, units)]
        plain = [i for i in range(len(rows)) if rows[i] is None]
        if plain:
            _pkg._merge_into(bt, st, dev, [planes[i] for i in plain], [outs[i] for i in plain], [units[i] for i in plain], kind,
                             [lags[i] for i in plain])
        groups = _pkg._by_width([(n, w) if rows[i] is not None else (0, w) for i, (n, w) in enumerate(units)])
        if not groups:
            return
        planes = [[p if p.data_ptr() % 16 == 0 else p.clone() for p in ps] for ps in planes]
        order = [i for _, idx in groups for i in idx]
        d_n = torch.tensor([units[i][0] for i in order], dtype=torch.int64, device=dev)
        counts = [int(pos.numel()) for pos, _ in records]
        first, pos = {}, 0
        for i in order:
            first[i] = pos
            pos += counts[i]
        d_outl = torch.stack([torch.cat([records[i][j] for i in order if counts[i]]) for j in (0, 1)], 1).contiguous() if pos else None
        at = 0
        for w, idx in groups:
            pbase = min(p.data_ptr() for i in idx for p in planes[i])
            obase = min(outs[i].data_ptr() for i in idx)
            q.merge(bt, st, w, [lags[i] for i in idx], [rows[i] for i in idx], pbase,
                    [p.data_ptr() - pbase for i in idx for p in planes[i]], [units[i][0] for i in idx], d_n[at:at + len(idx)], d_outl,
                    [first[i] for i in idx], [counts[i] for i in idx], obase, [outs[i].data_ptr() - obase for i in idx])
            at += len(idx)
    return merge_into


def _quantise_one(q, t, lags, row):
    """quantize_field's chain for a checked tensor and any quantiser: one split, a second one with room for every outlier found
    where outlier_capacity's records were too few -> (planes, positions, bits)"""
    import torch
    k, n = t.element_size(), t.numel()
    dev = t.device
    st = _pkg._plane_stream(dev, stream=None)
    poff, nbytes = _layout([(n, k)])
    with torch.cuda.stream(st):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        bt = _pkg.Batch(1, 1 << 20)
        try:
            cap, found, d_outl = outlier_capacity(n), 0, None
            while n:
                d_outl, _, d_found, _ = _split(q, bt, st, dev, [t], [(n, k)], [lags], [row], [cap], buf, poff)
                bt.finish(st, 1)
                found = int(d_found.cpu()[0])
                if found <= cap:
                    break
                cap = found
        finally:
            bt.close()
        pos, bits = _sorted_records(d_outl[:found]) if found else (torch.empty(0, dtype=torch.int64, device=dev),) * 2
    torch.cuda.current_stream(dev).wait_stream(st)
    return buf[:k * _pkg._al16(n)].view(k, _pkg._al16(n))[:, :n], pos, bits


def _records(what, positions, bits, dev):
    import torch
    for r in (positions, bits):
        if not isinstance(r, torch.Tensor) or r.dtype != torch.int64 or r.dim() != 1 or not r.is_contiguous():
            raise ValueError(f"{what}: the outliers' positions and bits are contiguous 1-D int64 tensors")
    if positions.numel() != bits.numel():
        raise ValueError(f"{what}: one position and one bit pattern per outlier")
    for r in (positions, bits):
        if r.numel() and (not r.is_cuda or (dev is not None and r.device != dev)):
            raise ValueError(f"{what}: the outliers are CUDA tensors on the planes' device")


def _restore_one(q, what, planes, dtype, shape, k, n, lags, row, positions, bits, stream):
    """restore_field's chain for any quantiser, behind the checks of dtype, shape, lags and row: the checks of the planes and the
    records, then one merge"""
    import torch
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or not planes.is_cuda or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError(f"{what}: planes is a uint8 CUDA tensor [k, numel] with contiguous rows")
    if tuple(planes.shape) != (k, n):
        raise ValueError(f"{what}: planes of shape {tuple(planes.shape)} for {k} x {n} bytes")
    _records(what, positions, bits, planes.device)
    dev = planes.device
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        out = torch.empty(shape, dtype=dtype, device=dev)
        bt = _pkg.Batch(1, 1 << 20)
        try:
            _merge(q, [(positions, bits)], [row])(bt, st, dev, [[planes[j].contiguous() for j in range(k)]], [out], [(n, k)],
                                                  "planes_grid", [lags])
            bt.finish(st, 1)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return out


def _compress(what, q, ts, lags, rows, block_size, stream):
    """compress_fields' chain for checked tensors and any quantiser: one split per element size, one finish and one read-back of
    the outlier counts; the tensors that found more than their capacity take compress_grids' split in the same places and are
    kept lossless; then the coder, and one item per tensor with its records sorted by position"""
    import torch
    if isinstance(block_size, bool) or not isinstance(block_size, int) or not 0 <= block_size < 1 << 64:
        raise ValueError(f"{what}: block_size is a size in bytes (shafa_block_count's uint64_t)")
    if not ts:
        return []
    dev = ts[0].device
    units = _pkg._elements(ts)
    caps = [outlier_capacity(n) if n else 0 for n, _ in units]
    poff, nbytes = _layout(units)
    st = _pkg._plane_stream(dev, stream)
    found = [0] * len(ts)
    with torch.cuda.stream(st):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        bt = _pkg.Batch(len(ts), 1 << 20)
        try:
            if any(n for n, _ in units):
                d_outl, first, d_found, order = _split(q, bt, st, dev, ts, units, lags, rows, caps, buf, poff)
                bt.finish(st, len(ts))
                for i, c in zip(order, d_found.cpu().tolist()):
                    found[i] = c
            lossless = [i for i in range(len(ts)) if found[i] > caps[i]]
            if lossless:                             # compress_grids' planes in the same places
                groups = [(w, [lossless[j] for j in idx]) for w, idx in _pkg._by_width([units[i] for i in lossless])]
                d_n = torch.tensor([units[i][0] for _, idx in groups for i in idx], dtype=torch.int64, device=dev)
                at = 0
                for w, idx in groups:
                    base = min(ts[i].data_ptr() for i in idx)
                    bt.split_planes_grid_dev(st, w, [_device_lags(lags[i], units[i][0]) for i in idx], base,
                                             [ts[i].data_ptr() - base for i in idx], [units[i][0] for i in idx],
                                             d_n[at:at + len(idx)], buf, [o for i in idx for o in poff[i]])
                    at += len(idx)
                bt.finish(st, len(ts))
        finally:
            bt.close()
        entries = _pkg._coded_planes(buf, poff, units, block_size, st)
        none = torch.empty(0, dtype=torch.int64, device=dev)
        items = []
        for i, (t, ps, nb) in enumerate(zip(ts, entries, _pkg._entry_bytes(entries))):
            keep = found[i] and i not in lossless
            pos, bits = _sorted_records(d_outl[first[i]:first[i] + found[i]]) if keep else (none, none)
            items.append(q.item(t, lags[i], rows[i], i in lossless, ps, pos, bits, nb + (8 + t.element_size()) * int(pos.numel())))
    torch.cuda.current_stream(dev).wait_stream(st)
    return items


def _decompress(what, q, items, lags, rows, stream):
    """decompress_fields' chain for checked items and any quantiser: the decode chain with _merge for its merge"""
    return _pkg._merge_items(what, items, "planes_grid", lags, False, stream,
                             _merge(q, [(it.outlier_pos, it.outlier_bits) for it in items], rows))


# ---- one tensor, no coder
def quantize_field(t, abs_error, lags):
    """The byte planes of the Lorenzo differences of a float32 or float64 CUDA tensor's CODES under the absolute error bound
    `abs_error`, and its outliers: (planes, positions, bits).  `planes` is split_grid's [k, numel] uint8 tensor over the codes
    rint(x * T(1 / step)) as integers of the element's width, step = 2 abs_error (1 - FIELD_SLACK) rounded down into the dtype;
    `positions` (int64, sorted) and `bits` (int64) are the elements whose restored value code * step misses abs_error (rounded
    down into the dtype) or that have no code: restore_field gives those back bit for bit and every other within the bound.
    `lags` as split_grid takes them.  One split_planes_grid_quant_dev launch, a second one with room for every outlier found
    where outlier_capacity's records were too few; one synchronisation each."""
    import torch
    what = "quantize_field"
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    t = _field_tensors(what, t)[0]
    lags = _pkg.grids._lag_tuple(what, lags)
    return _quantise_one(_QUANT, t, lags, _params(what, abs_error, t.element_size()))


def _step(what, step, k):
    if isinstance(step, bool) or not isinstance(step, (int, float)) or not _legal(float(step), k) \
            or (k == 4 and float(np.float32(step)) != step) or not math.isfinite(_inverse(float(step), k)):
        raise ValueError(f"{what}: step is a quantiser's step, a normal float of the dtype > 0, not {step!r}")
    return float(step)


def restore_field(planes, dtype, shape, lags, step, positions, bits, stream=None):
    """quantize_field's inverse for one tensor: `planes` as merge_grid takes them -> a tensor of `dtype` (float32 or float64) and
    `shape`, every element T(code) * step but the outliers, whose `bits` are stored at their `positions`.  One
    merge_planes_grid_quant_dev call, one synchronisation."""
    import torch
    what = "restore_field"
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: float32 and float64 tensors, not {dtype!r}")
    k, shape, n = _pkg._plane_dtype(what, dtype, shape)
    lags = _pkg.grids._lag_tuple(what, lags)
    step = _step(what, step, k)
    return _restore_one(_QUANT, what, planes, dtype, shape, k, n, lags, (step,), positions, bits, stream)


# ---- the drivers
def compress_fields(tensors, abs_error, axes=None, lags=None, block_size=8 << 20, stream=None):
    """compress_grids for float32 and float64 fields UNDER AN ABSOLUTE ERROR BOUND: every element comes back within `abs_error`
    of the original, or bit for bit.  `tensors`, `axes`, `lags` and `block_size` as compress_grids takes them, and its argument
    ValueErrors; any dtype but float32 and float64 is a ValueError.  `abs_error` is a float for all tensors or a list with one
    per tensor, finite and > 0 and not below what the dtype resolves: a ValueError otherwise, before any device work.  Returns
    one CompressedField per tensor, which decompress_fields gives back.

    The transform: code = rint(x * T(1 / step)) as an integer of the element's width, step = 2 abs_error (1 - FIELD_SLACK)
    rounded down into the dtype, and the planes are compress_grids' over the codes.  The decoder makes x' = T(code) * step; the
    split makes the same x' and checks |x - x'| <= bound (abs_error rounded down into the dtype) for every element.  One that
    fails — a NaN, an infinity, a value past the code range of 2^30 (2^62) steps, a tie the rounding of x' threw over the bound
    — is an OUTLIER, kept as {position, bits} and given back bit for bit.  -0.0 may come back as +0.0.  The slack keeps ties
    inside the bound while |x| stays below about 2^16 abs_error at float32.

    A tensor that finds more outliers than outlier_capacity(numel) = 16 + numel // 64 is kept LOSSLESS, compress_grids' planes
    and a `step` of 0.0: the bound sits at the data's own precision there, or the tensor is noise.

    Which lags pay under the bound, and what a bound costs, can be asked first without compressing: choose_field_lags ranks the
    candidates and its pick goes into `lags`; field_rates and fit_abs_error size a list of bounds.

    Chain: one split_planes_grid_quant_dev per element size over all tensors — no temporary of codes exists — one finish and
    one read-back of the outlier counts (the tensors kept lossless then take one split_planes_grid_dev per element size and a
    finish) -> compressed_sizes -> compress_many, as compress_tensors; a tensor's records are sorted by position, so an item
    is reproducible."""
    what = "compress_fields"
    ts = _field_tensors(what, tensors)
    lags = _pkg.grids._lags(what, ts, axes, lags)
    errs, params = _abs_errors(what, ts, abs_error)
    return _compress(what, _QUANT, ts, lags, [p + (e,) for p, e in zip(params, errs)], block_size, stream)


# ---- sizes under a bound: the quantising split's histograms without the planes (Batch.hist_planes_grid_quant_dev)
def _lag_sets(what, cs):
    """candidates that compress_fields can make: tuples of lags, and no () — it has no plain item"""
    out = []
    for c in cs:
        if not isinstance(c, tuple) or c == ():
            raise ValueError(f"{what}: a candidate is a non-empty tuple of lags, not {c!r}: compress_fields makes no plain planes")
        out.append(_pkg.grids._lag_tuple(what, c))
    return out


def _field_candidates(what, ts, axes, candidates):
    """one list of candidates per checked tensor: grid_sizes' `candidates` without (), or else the non-empty subsets of each
    tensor's axis lags"""
    if candidates is None:
        return [_pkg.grids._subsets(g)[1:] for g in _pkg.grids._lags(what, ts, axes, None)]
    return [_lag_sets(what, cs) for cs in _pkg.grids._candidates(what, ts, axes, candidates)]


def _bounds(what, abs_errors, k):
    """a non-empty list of bounds -> its (step, bound) pairs for elements of k bytes"""
    if not isinstance(abs_errors, (list, tuple)) or not abs_errors:
        raise ValueError(f"{what}: abs_errors is a non-empty list of floats, not {abs_errors!r}")
    return [_params(what, e, k) for e in abs_errors]


def _sizes(q, ts, cands, rows, stream):
    """field_sizes' shape for checked tensors and any quantiser: per tensor its candidates as (lags, nbytes, outliers), sorted by
    (outliers > outlier_capacity(numel), nbytes, len(lags), lags); [((), 0, 0)] for an empty or 0-dimensional one"""
    out = [[((), 0, 0)] if not t.numel() or not t.dim() else None for t in ts]
    blocks = [(i, c, rows[i]) for i in range(len(ts)) if out[i] is None for c in cands[i]]
    if not blocks:
        return out
    found = [[] for _ in ts]
    for (i, c, _), (nb, no) in zip(blocks, _pkg.grids._model_sizes(q.hist, ts, blocks, True, stream)):
        found[i].append((c, nb, no))
    key = lambda n: lambda e: (e[2] > outlier_capacity(n), e[1], len(e[0]), e[0])
    return [o if o is not None else sorted(f, key=key(t.numel())) for o, f, t in zip(out, found, ts)]


def _rate_list(q, t, lags, labels, rows, stream):
    """field_rates' shape for a checked tensor and any quantiser: one block per row on the same region, in one launch ->
    [(label, nbytes, outliers)]; 0 bytes at every row for an empty or 0-dimensional tensor"""
    if not t.numel() or not t.dim():
        return [(e, 0, 0) for e in labels]
    sizes = _pkg.grids._model_sizes(q.hist, [t], [(0, lags, r) for r in rows], True, stream)
    return [(e, nb, no) for e, (nb, no) in zip(labels, sizes)]


def field_histograms(t, abs_error, lag_sets, stream=None):
    """The byte histograms of the planes quantize_field(t, abs_error, lags) would give for every `lags` of the list `lag_sets`,
    and its count of outliers, without the planes and without the records: `t` a contiguous float32 or float64 CUDA tensor,
    every entry of `lag_sets` a tuple quantize_field takes — () is a ValueError, there is no plain candidate under a bound —
    and `abs_error` a float for all entries or a list with one per entry: the same lags may appear several times with
    different bounds.  Returns (freq, outliers): int64 CUDA tensors [len(lag_sets), k, 256], every row summing to t.numel(), and
    [len(lag_sets)].  Step and bound are compress_fields' (_params).  One hist_planes_grid_quant_dev launch per HIST_GROUP
    candidates, one block per candidate on the same region, one synchronisation."""
    import torch
    what = "field_histograms"
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    t = _field_tensors(what, t)[0]
    if not isinstance(lag_sets, (list, tuple)):
        raise ValueError(f"{what}: lag_sets is a list of tuples of lags, not {lag_sets!r}")
    sets = _lag_sets(what, lag_sets)
    k = t.element_size()
    if isinstance(abs_error, (list, tuple)):
        if len(abs_error) != len(sets):
            raise ValueError(f"{what}: abs_error is a float or a list with one float per entry of lag_sets")
        params = [_params(what, e, k) for e in abs_error]
    else:
        params = [_params(what, abs_error, k)] * len(sets)
    return _pkg.grids._histograms(_QUANT.hist, t, sets, params, True, stream)


def field_sizes(tensors, abs_error, axes=None, candidates=None, stream=None):
    """How large would compress_fields make each tensor with each candidate's lags, under its bound?  Per tensor a list of
    (lags, nbytes, outliers), sorted by (outliers > outlier_capacity(numel), nbytes, len(lags), lags): the first entry is the
    candidate to take.  `tensors`, `abs_error` and `axes` as compress_fields takes them, and its ValueErrors, before any device
    work.  `candidates` as grid_sizes takes them, but a candidate of () is a ValueError: compress_fields makes no plain planes;
    None: every non-empty subset of the tensor's axis lags, at most seven.  An empty or 0-dimensional tensor gives [((), 0, 0)]
    whatever the candidates.

    nbytes is CompressedField.nbytes' own formula over a MODEL of the planes, of order 0: the sum over the candidate's byte
    planes of min(numel, the Shannon-Fano bytes of the whole plane under the table of its own histogram) — a plane that would
    not shrink counts raw — plus (8 + element size) per outlier.  It is not the size compress_fields reports: it knows nothing
    of RLE, of the split into blocks of block_size with a table each, or of the files' tables and headers (DESIGN 7.31 has both
    side by side).  A candidate with more outliers than outlier_capacity(numel) sorts LAST: compress_fields would keep that
    tensor lossless, its planes would be compress_grids' over the raw bits, and grid_sizes is the model for it then, not this
    number.

    Chain: per element size one hist_planes_grid_quant_dev over all tensors' candidates, one block per candidate on its
    tensor's region — no plane and no record ever exists, and no histogram comes to the host -> sf_build_codes ->
    sf_encoded_size_dev -> one finish, one read-back of the sizes and the counts."""
    what = "field_sizes"
    ts = _field_tensors(what, tensors)
    cands = _field_candidates(what, ts, axes, candidates)
    return _sizes(_QUANT, ts, cands, _abs_errors(what, ts, abs_error)[1], stream)


def choose_field_lags(tensors, abs_error, axes=None, candidates=None, stream=None):
    """Which lags to compress each tensor with under its bound: field_sizes' first entry per tensor, ready for
    compress_fields(tensors, abs_error, lags=[...]) — () for an empty or 0-dimensional tensor, which takes any lags.
    field_sizes' arguments, chain and caveats."""
    return [sizes[0][0] for sizes in field_sizes(tensors, abs_error, axes, candidates, stream)]


def field_rates(t, abs_errors, lags=None, axes=None, stream=None):
    """The rate of one tensor over a list of bounds: [(abs_error, nbytes, outliers)] in the order of `abs_errors`, a non-empty
    list of floats as compress_fields takes one.  `lags` as compress_fields takes them for one tensor; None: the tensor's axis
    lags (`axes`), as there.  nbytes and outliers are field_sizes' model, with its caveats; an entry with more outliers than
    outlier_capacity(numel) is one compress_fields would keep lossless.  One block per bound on the same region, in ONE
    hist_planes_grid_quant_dev launch, then field_sizes' chain.  An empty or 0-dimensional tensor gives 0 bytes at every bound."""
    return _rates("field_rates", t, abs_errors, lags, axes, stream)


def _rates(what, t, abs_errors, lags, axes, stream):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a contiguous CUDA tensor")
    ts = _field_tensors(what, t)
    g = _pkg.grids._lags(what, ts, axes, lags)[0]
    params = _bounds(what, abs_errors, ts[0].element_size())
    return _rate_list(_QUANT, ts[0], g, abs_errors, params, stream)


def fit_abs_error(t, max_bytes, abs_errors, lags=None, axes=None, stream=None):
    """The smallest bound of the list `abs_errors` at which the tensor fits `max_bytes` (an int >= 0): field_rates' nbytes <=
    max_bytes, with no more outliers than outlier_capacity(numel) — past that compress_fields keeps the tensor lossless and the
    model is not its size.  None where no bound of the list does.  field_rates' arguments, chain and caveats."""
    what = "fit_abs_error"
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 0:
        raise ValueError(f"{what}: max_bytes is an int >= 0, not {max_bytes!r}")
    rates = _rates(what, t, abs_errors, lags, axes, stream)
    n = t.numel()
    fits = [e for e, nb, no in rates if nb <= max_bytes and no <= outlier_capacity(n)]
    return min(fits) if fits else None


def decompress_fields(items, stream=None):
    """compress_fields' inverse: `items` is a CompressedField or a list of them (their planes on one device) -> the list of
    tensors, each element within its item's `bound` of the original, or bit for bit: the outliers, and every element of an item
    kept lossless (a `step` of 0.0).

    Chain: decompress_grids', decompress_many over all coded planes, then one merge_planes_grid_quant_dev per element size over
    the quantised items — the sums at every lag in turn, the codes restored in place, the outliers' bits on top — and one
    merge_planes_grid_dev per element size over the lossless ones.  Anything that is not a CompressedField is refused with a
    ValueError before any device work, as is an item whose lags, step or outliers are malformed.  decompress_tensors' errors
    otherwise."""
    import torch
    what = "decompress_fields"
    if isinstance(items, CompressedField):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedField) for it in items):
        raise ValueError(f"{what}: a CompressedField or a list of them (compress_fields' items)")
    lags = [_pkg.grids._lag_tuple(what, it.lags) for it in items]
    rows = []
    for it in items:
        if it.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: float32 and float64 tensors, not {it.dtype!r}")
        _records(what, it.outlier_pos, it.outlier_bits, None)
        lossless = isinstance(it.step, float) and it.step == 0.0
        if lossless and it.outlier_pos.numel():
            raise ValueError(f"{what}: an item kept lossless has no outliers")
        rows.append(None if lossless else (_step(what, it.step, 4 if it.dtype == torch.float32 else 8),))
    return _decompress(what, _QUANT, items, lags, rows, stream)

"""Fixed-width records, one file set per byte column: split_records / merge_records and compress_records / decompress_records
on top of Batch.split_records_dev / merge_records_dev (csrc/records.hip; include/shafa_hip.h: "Byte columns of fixed-width
records").

compress_tensors takes a tensor apart by the bytes of its ELEMENT, 1, 2, 4 or 8 of them.  Here the unit is a RECORD of any
width from 1 to RECORDS_MAX_WIDTH bytes, whatever the dtype: the 3 bytes of an RGB pixel, the 12 of an fp32 xyz point, the 16
of a complex128, the 32 of a binary log's struct.  Column j — byte j of every record — is coded apart, so the red channel does
not share a histogram with the blue one, nor x's exponent byte with z's.

The drivers live in this submodule; the package re-exports them.  What is the records' own is here: the meaning of a width
and of its default, and the item.  The chains are the package's, compress_tensors' and decompress_tensors' with the record as
the unit and "records" as the variant (_plane_entries, _merge_items, _split_one, _merge_one), reached through the package at
the time of the call."""
import sys

_pkg = sys.modules[__package__]


def records_pass(width):
    """SHAFA_RECORDS_PASS(width): the records a workgroup of split_records_dev / merge_records_dev takes through LDS at a time
    — the largest power of two with pass * width <= 32768, 8192 at the most; a multiple of 16 that divides RECORDS_TILE."""
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= _pkg.RECORDS_MAX_WIDTH:
        raise ValueError(f"records_pass: a width of 1 .. {_pkg.RECORDS_MAX_WIDTH}")
    return 8192 if width <= 4 else 4096 if width <= 8 else 2048 if width <= 16 else 1024 if width <= 32 else 512


class CompressedRecords:
    """A tensor compressed by byte column of its fixed-width records (compress_records), in memory: `dtype` and `shape` of the
    original, `width` — the bytes of a record — `planes` — one entry per byte of the record, in the record's order: the dict
    compress_many returns for that column's bytes, or the column itself (a uint8 CUDA tensor) where coding it would not shrink
    it — and `nbytes`, the sum of the file lengths and of the raw columns' lengths.  Not a CompressedTensor: decompress_records
    alone gives the tensor back."""
    __slots__ = ("dtype", "shape", "width", "planes", "nbytes")

    def __init__(self, dtype, shape, width, planes, nbytes):
        self.dtype, self.shape, self.width, self.planes, self.nbytes = dtype, tuple(shape), width, list(planes), int(nbytes)

    def __repr__(self):
        kinds = ["raw" if not isinstance(p, dict) else "+".join(sorted(p)) for p in self.planes]
        return f"CompressedRecords({self.dtype}, {self.shape}, width={self.width}, planes={kinds}, nbytes={self.nbytes})"


def _width(what, w):
    if isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= _pkg.RECORDS_MAX_WIDTH:
        raise ValueError(f"{what}: a width is an int of 1 .. {_pkg.RECORDS_MAX_WIDTH} bytes, not {w!r}")
    return w


def _record_tensors(what, ts, widths):
    """the tensors records are taken of and their widths, checked before any device work -> (list of tensors, list of widths)"""
    import torch
    if isinstance(ts, torch.Tensor):
        ts = [ts]
    if not isinstance(ts, (list, tuple)) or any(not isinstance(t, torch.Tensor) for t in ts):
        raise ValueError(f"{what}: a tensor or a list of tensors")
    if widths is None or (isinstance(widths, int) and not isinstance(widths, bool)):
        widths = [widths] * len(ts)
    elif not isinstance(widths, (list, tuple)) or len(widths) != len(ts):
        raise ValueError(f"{what}: widths is None, an int or a list with one int per tensor")
    out = []
    for t, w in zip(ts, widths):
        es = t.element_size()
        if w is None:                                # the bytes of the last dimension; of the element where there is none
            w = t.shape[-1] * es if t.dim() >= 2 and t.shape[-1] else es
        w = _width(what, w)
        if t.numel() * es % w:
            raise ValueError(f"{what}: a width of {w} does not divide the tensor's {t.numel() * es} bytes")
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what}: contiguous CUDA tensors")
        if t.device != ts[0].device:
            raise ValueError(f"{what}: the tensors are on one device")
        out.append(w)
    return list(ts), out


def split_records(t, width=None, stream=None):
    """The byte columns of a contiguous CUDA tensor taken as records of `width` = 1 .. RECORDS_MAX_WIDTH bytes (None: the bytes
    of its last dimension, or of its element where it has fewer than two dimensions); the width divides the tensor's bytes.  Any
    dtype.  Returns a uint8 tensor [width, records], row j byte j of every record.  Rows start at multiples of 16 bytes: with
    a record count that is no multiple of 16 the result is a view with padded rows.  One split_records_dev launch, one
    synchronisation."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("split_records: a contiguous CUDA tensor")
    (t,), (w,) = _record_tensors("split_records", t, width)
    return _pkg._split_one("records", t, t.numel() * t.element_size() // w, w, stream)


def merge_records(planes, dtype, shape, stream=None):
    """split_records' inverse for one tensor: `planes` is a uint8 CUDA tensor [width, records] with unit stride along a row
    (rows may be padded, as split_records leaves them; rows that do not start at a multiple of 16 bytes are copied first) -> a
    tensor of `dtype` and `shape`, whose bytes are width * records.  One merge_records_dev launch, one synchronisation."""
    import torch
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError("merge_records: planes is a uint8 CUDA tensor [width, records] with contiguous rows")
    w, shape, n = _pkg._record_dtype("merge_records", dtype, shape, int(planes.shape[0]))
    if int(planes.shape[1]) != n:
        raise ValueError(f"merge_records: planes of shape {tuple(planes.shape)} for {w} x {n} bytes")
    if not planes.is_cuda:
        raise ValueError("merge_records: planes is a uint8 CUDA tensor [width, records] with contiguous rows")
    return _pkg._merge_one("records", planes, dtype, shape, stream)


def compress_records(tensors, widths=None, block_size=8 << 20, stream=None):
    """Compress tensors by byte column of their fixed-width records.  `tensors` is a tensor or a list of tensors: contiguous
    CUDA tensors on one device, of ANY dtype (complex128 and bool included) and shape, empty ones included.  `widths` is None,
    an int for all, or one entry (an int or None) per tensor: the bytes of a record, 1 .. RECORDS_MAX_WIDTH, which divide the
    tensor's bytes; None means the bytes of the tensor's last dimension, and the element size for a 0- or 1-dimensional tensor
    (or an empty last dimension).  Returns one CompressedRecords per tensor; decompress_records gives the tensors back bit for
    bit.

    Chain, compress_tensors' own (the package's _plane_entries) with the record as the unit: one split_records_dev per distinct
    width over all tensors of that width (blocks addressed from the lowest tensor address: nothing is concatenated) into one
    buffer at 16-aligned offsets -> compressed_sizes over all columns of 1 KiB or more in one call -> compress_many over exactly
    the columns whose file set comes out smaller than the column.  Every other column stays raw, as a view of the buffer.
    `block_size` is compress_many's."""
    ts, ws = _record_tensors("compress_records", tensors, widths)
    units = [(t.numel() * t.element_size() // w, w) for t, w in zip(ts, ws)]
    entries, nbytes = _pkg._plane_entries("compress_records", ts, units, "records", None, block_size, stream)
    return [CompressedRecords(t.dtype, t.shape, w, ps, nb) for t, w, ps, nb in zip(ts, ws, entries, nbytes)]


def decompress_records(items, stream=None):
    """compress_records' inverse: `items` is a CompressedRecords or a list of them (their columns on one device) -> the list of
    tensors, each equal to the original bit for bit.

    Chain, decompress_tensors' own (the package's _merge_items): decompress_many over all coded columns of all items in one
    call -> one merge_records_dev per distinct width, straight into the freshly allocated result tensors.  A column entry that
    is a ShafaError instance, or whose file set fails to decode, raises that ShafaError; a decoded or raw column whose length is
    not the record count raises ShafaError(FILE_UNRECOGNIZABLE).  Malformed items — a CompressedTensor among them — raise
    ValueError before any device work."""
    if isinstance(items, CompressedRecords):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedRecords) for it in items):
        raise ValueError("decompress_records: a CompressedRecords or a list of them (compress_records' items)")
    return _pkg._merge_items("decompress_records", items, "records", None, False, stream)

"""Fixed-width records, one file set per byte column: split_records / merge_records and compress_records / decompress_records
on top of Batch.split_records_dev / merge_records_dev (csrc/records.hip; include/shafa_hip.h: "Byte columns of fixed-width
records").

compress_tensors takes a tensor apart by the bytes of its ELEMENT, 1, 2, 4 or 8 of them.  Here the unit is a RECORD of any
width from 1 to RECORDS_MAX_WIDTH bytes, whatever the dtype: the 3 bytes of an RGB pixel, the 12 of an fp32 xyz point, the 16
of a complex128, the 32 of a binary log's struct.  Column j — byte j of every record — is coded apart, so the red channel does
not share a histogram with the blue one, nor x's exponent byte with z's.

The drivers live in this submodule; the package re-exports them.  They reach the package's own drivers (compressed_sizes,
compress_many, decompress_many, Batch) through the package at the time of the call."""
import sys

_pkg = sys.modules[__package__]
ShafaError = _pkg.ShafaError


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


def _block_size(what, block_size):
    if isinstance(block_size, bool) or not isinstance(block_size, int) or not 0 <= block_size < 1 << 64:
        raise ValueError(f"{what}: block_size is a size in bytes (shafa_block_count's uint64_t)")


def _by_width(ws, nrec):
    """indices of the tensors with a record, grouped by width -> [(width, [index, ...])]"""
    return [(w, [i for i, (x, n) in enumerate(zip(ws, nrec)) if x == w and n])
            for w in sorted({x for x, n in zip(ws, nrec) if n})]


def _split_into(bt, st, dev, ts, ws, nrec):
    """one split_records_dev per distinct width over ts (blocks addressed from the lowest tensor address: nothing is
    concatenated) -> the columns' buffer and each tensor's column offsets in it, all multiples of 16"""
    import torch
    poff, pos = [], 0
    for w, n in zip(ws, nrec):
        step = _pkg._al16(n)
        poff.append([pos + j * step for j in range(w)])
        pos += w * step
    buf = torch.empty(pos + 16, dtype=torch.uint8, device=dev)
    groups = _by_width(ws, nrec)
    if groups:
        d_n = torch.tensor([nrec[i] for _, idx in groups for i in idx], dtype=torch.int64, device=dev)
    at = 0
    for w, idx in groups:
        base = min(ts[i].data_ptr() for i in idx)
        bt.split_records_dev(st, w, base, [ts[i].data_ptr() - base for i in idx], [nrec[i] for i in idx], d_n[at:at + len(idx)],
                             buf, [o for i in idx for o in poff[i]])
        at += len(idx)
    return buf, poff


def _merge_into(bt, st, dev, planes, outs, ws, nrec):
    """one merge_records_dev per distinct width: planes[i] (the 1-D uint8 columns of tensor i, nrec[i] bytes each) -> outs[i].
    A column that is not 16-aligned is copied first."""
    import torch
    groups = _by_width(ws, nrec)
    if not groups:
        return
    planes = [[p if p.data_ptr() % 16 == 0 else p.clone() for p in ps] for ps in planes]
    d_n = torch.tensor([nrec[i] for _, idx in groups for i in idx], dtype=torch.int64, device=dev)
    at = 0
    for w, idx in groups:
        pbase = min(p.data_ptr() for i in idx for p in planes[i])
        obase = min(outs[i].data_ptr() for i in idx)
        bt.merge_records_dev(st, w, pbase, [p.data_ptr() - pbase for i in idx for p in planes[i]], [nrec[i] for i in idx],
                             d_n[at:at + len(idx)], obase, [outs[i].data_ptr() - obase for i in idx])
        at += len(idx)


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
    dev, n = t.device, t.numel() * t.element_size() // w
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        bt = _pkg.Batch(1, 1 << 20)
        try:
            buf, _ = _split_into(bt, st, dev, [t], [w], [n])
            bt.finish(st, 1)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return buf[:w * _pkg._al16(n)].view(w, _pkg._al16(n))[:, :n]


def _record_dtype(what, dtype, shape, width):
    """dtype, shape and width of a tensor to be put together from columns, checked -> (shape, records)"""
    import torch
    if not isinstance(dtype, torch.dtype):
        raise ValueError(f"{what}: dtype is a torch.dtype")
    try:
        shape = tuple(int(d) for d in shape)
    except TypeError:
        raise ValueError(f"{what}: shape is a sequence of ints") from None
    if any(d < 0 for d in shape):
        raise ValueError(f"{what}: negative dimension")
    nbytes = _pkg._numel(shape) * torch.empty((), dtype=dtype).element_size()
    if nbytes % _width(what, width):
        raise ValueError(f"{what}: a width of {width} does not divide the tensor's {nbytes} bytes")
    return shape, nbytes // width


def merge_records(planes, dtype, shape, stream=None):
    """split_records' inverse for one tensor: `planes` is a uint8 CUDA tensor [width, records] with unit stride along a row
    (rows may be padded, as split_records leaves them; rows that do not start at a multiple of 16 bytes are copied first) -> a
    tensor of `dtype` and `shape`, whose bytes are width * records.  One merge_records_dev launch, one synchronisation."""
    import torch
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError("merge_records: planes is a uint8 CUDA tensor [width, records] with contiguous rows")
    w = int(planes.shape[0])
    shape, n = _record_dtype("merge_records", dtype, shape, w)
    if int(planes.shape[1]) != n:
        raise ValueError(f"merge_records: planes of shape {tuple(planes.shape)} for {w} x {n} bytes")
    if not planes.is_cuda:
        raise ValueError("merge_records: planes is a uint8 CUDA tensor [width, records] with contiguous rows")
    dev = planes.device
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        out = torch.empty(shape, dtype=dtype, device=dev)
        bt = _pkg.Batch(1, 1 << 20)
        try:
            _merge_into(bt, st, dev, [[planes[j].contiguous() for j in range(w)]], [out], [w], [n])
            bt.finish(st, 1)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return out


def compress_records(tensors, widths=None, block_size=8 << 20, stream=None):
    """Compress tensors by byte column of their fixed-width records.  `tensors` is a tensor or a list of tensors: contiguous
    CUDA tensors on one device, of ANY dtype (complex128 and bool included) and shape, empty ones included.  `widths` is None,
    an int for all, or one entry (an int or None) per tensor: the bytes of a record, 1 .. RECORDS_MAX_WIDTH, which divide the
    tensor's bytes; None means the bytes of the tensor's last dimension, and the element size for a 0- or 1-dimensional tensor
    (or an empty last dimension).  Returns one CompressedRecords per tensor; decompress_records gives the tensors back bit for
    bit.

    Chain, compress_tensors': one split_records_dev per distinct width over all tensors of that width (blocks addressed from the
    lowest tensor address: nothing is concatenated) into one buffer at 16-aligned offsets -> compressed_sizes over all columns
    of 1 KiB or more in one call -> compress_many over exactly the columns whose file set comes out smaller than the column.
    Every other column stays raw, as a view of the buffer.  `block_size` is compress_many's."""
    import torch
    ts, ws = _record_tensors("compress_records", tensors, widths)
    _block_size("compress_records", block_size)
    if not ts:
        return []
    nrec = [t.numel() * t.element_size() // w for t, w in zip(ts, ws)]
    dev = ts[0].device
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        bt = _pkg.Batch(len(ts), 1 << 20)
        try:
            buf, poff = _split_into(bt, st, dev, ts, ws, nrec)
            bt.finish(st, len(ts))
        finally:
            bt.close()
        entries = [[buf[o:o + n] for o in poff[i]] for i, n in enumerate(nrec)]
        cand = [(i, j) for i, n in enumerate(nrec) if n >= 1024 for j in range(ws[i])]
        keep = []
        if cand:
            d_in, sizes = _pkg._back_to_back(buf, [(poff[i][j], nrec[i]) for i, j in cand])
            sized = _pkg.compressed_sizes(d_in, sizes, block_size=block_size, stream=st)
            keep = [c for c, e in zip(cand, sized) if isinstance(e, dict) and sum(e.values()) < nrec[c[0]]]
        if keep:
            d_in, sizes = _pkg._back_to_back(buf, [(poff[i][j], nrec[i]) for i, j in keep])
            for (i, j), e in zip(keep, _pkg.compress_many(d_in, sizes, block_size=block_size, stream=st)):
                if isinstance(e, ShafaError):
                    raise e
                entries[i][j] = e
    torch.cuda.current_stream(dev).wait_stream(st)
    return [CompressedRecords(t.dtype, t.shape, w, ps,
                              sum(sum(int(f.numel()) for f in p.values()) if isinstance(p, dict) else int(p.numel()) for p in ps))
            for t, w, ps in zip(ts, ws, entries)]


def decompress_records(items, stream=None):
    """compress_records' inverse: `items` is a CompressedRecords or a list of them (their columns on one device) -> the list of
    tensors, each equal to the original bit for bit.

    Chain: decompress_many over all coded columns of all items in one call -> one merge_records_dev per distinct width,
    straight into the freshly allocated result tensors.  A column entry that is a ShafaError instance, or whose file set fails
    to decode, raises that ShafaError; a decoded or raw column whose length is not the record count raises
    ShafaError(FILE_UNRECOGNIZABLE).  Malformed items — a CompressedTensor among them — raise ValueError before any device
    work."""
    import torch
    what = "decompress_records"
    if isinstance(items, CompressedRecords):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedRecords) for it in items):
        raise ValueError(f"{what}: a CompressedRecords or a list of them (compress_records' items)")
    metas, dev = [], None
    for it in items:
        shape, n = _record_dtype(what, it.dtype, it.shape, it.width)
        if not isinstance(it.planes, (list, tuple)) or len(it.planes) != it.width:
            raise ValueError(f"{what}: records of {it.width} bytes have {it.width} columns")
        for p in it.planes:
            if isinstance(p, ShafaError):
                continue
            if isinstance(p, dict):
                fs = [f for f in p.values() if isinstance(f, torch.Tensor)]
                if not ({".shaf", ".cod"} <= set(p) or {".rle.shaf", ".rle.cod"} <= set(p)) or len(fs) != len(p):
                    raise ValueError(f"{what}: a compressed column is compress_many's dict of files")
            elif isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and p.dim() == 1 and p.is_contiguous():
                fs = [p]
            else:
                raise ValueError(f"{what}: a column is a dict of files or a contiguous 1-D uint8 tensor")
            for f in fs:
                if not f.is_cuda:
                    raise ValueError(f"{what}: columns are CUDA tensors")
                if dev is not None and f.device != dev:
                    raise ValueError(f"{what}: the columns are on one device")
                dev = f.device
        metas.append((shape, n))
    for it in items:
        for p in it.planes:
            if isinstance(p, ShafaError):
                raise p
    if not items:
        return []
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        coded = [(i, j) for i, it in enumerate(items) for j, p in enumerate(it.planes) if isinstance(p, dict)]
        planes = [list(it.planes) for it in items]
        if coded:
            files = [_pkg.plane_files(items[i].planes[j]) for i, j in coded]
            for (i, j), r in zip(coded, _pkg.decompress_many(files, stream=st)):
                if isinstance(r, ShafaError):
                    raise r
                planes[i][j] = r
        for (_, n), ps in zip(metas, planes):
            if any(int(p.numel()) != n for p in ps):
                raise ShafaError(_pkg.FILE_UNRECOGNIZABLE, f"{what}: a column's length is not the record count")
        outs = [torch.empty(shape, dtype=it.dtype, device=dev) for it, (shape, _) in zip(items, metas)]
        bt = _pkg.Batch(len(items), 1 << 20)
        try:
            _merge_into(bt, st, dev, planes, outs, [it.width for it in items], [n for _, n in metas])
            bt.finish(st, len(items))
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return outs

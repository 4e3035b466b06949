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

The drivers live in this submodule; the package re-exports them.  The layout, the record handling and the order-0 model are
fields.py's, the coder's half of the chain (_coded_planes) and the decode chain (_merge_items) the package's, reached through it
at the time of the call."""
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


def _device_lags(lags, numel):
    """the row of lags the entries get: () is a lag at the capacity, which subtracts nothing in split and merge alike"""
    return tuple(lags) if len(lags) else (max(int(numel), 1),)


# ---- the launches
def _split_rounded(bt, st, dev, ts, units, lags, keeps, caps, buf, poff):
    """fields._split_fields with the rounding split: one launch per element size over ts into buf -> (the records buffer, each
    tensor's first record, the counts of outliers found in the launches' order, and that order)"""
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
        bt.split_planes_grid_round_dev(st, w, [_device_lags(lags[i], units[i][0]) for i in idx],
                                       [MANTISSA_BITS[ts[i].dtype] for i in idx], [keeps[i] for i in idx], base,
                                       [ts[i].data_ptr() - base for i in idx], [units[i][0] for i in idx], d_n[at:at + len(idx)], buf,
                                       [o for i in idx for o in poff[i]], d_outl if pos else None, [first[i] for i in idx],
                                       [caps[i] for i in idx], d_found[at:at + len(idx)])
        at += len(idx)
    return d_outl, first, d_found, order


def _merge_rounded(items, keeps):
    """_merge_into's stand-in for decompress_rounded: the lossless items (a keep of None) through _merge_into as decompress_grids'
    go, the others through one merge_planes_grid_round_dev per element size"""
    def merge_into(bt, st, dev, planes, outs, units, kind, lags):
        import torch
        dlags = [_device_lags(g, n) for g, (n, _) in zip(lags, units)]
        plain = [i for i in range(len(items)) if keeps[i] is None]
        if plain:
            _pkg._merge_into(bt, st, dev, [planes[i] for i in plain], [outs[i] for i in plain], [units[i] for i in plain], kind,
                             [dlags[i] for i in plain])
        rounded = [(n, w) if keeps[i] is not None else (0, w) for i, (n, w) in enumerate(units)]
        groups = _pkg._by_width(rounded)
        if not groups:
            return
        planes = [[p if p.data_ptr() % 16 == 0 else p.clone() for p in ps] for ps in planes]
        order = [i for _, idx in groups for i in idx]
        d_n = torch.tensor([units[i][0] for i in order], dtype=torch.int64, device=dev)
        counts = [int(it.outlier_pos.numel()) for it in items]
        first, pos = {}, 0
        for i in order:
            first[i] = pos
            pos += counts[i]
        d_outl = torch.stack([torch.cat([items[i].outlier_pos for i in order if counts[i]]),
                              torch.cat([items[i].outlier_bits for i in order if counts[i]])], 1).contiguous() if pos else None
        at = 0
        for w, idx in groups:
            pbase = min(p.data_ptr() for i in idx for p in planes[i])
            obase = min(outs[i].data_ptr() for i in idx)
            bt.merge_planes_grid_round_dev(st, w, [dlags[i] for i in idx], [MANTISSA_BITS[items[i].dtype] for i in idx],
                                           [keeps[i] for i in idx], pbase, [p.data_ptr() - pbase for i in idx for p in planes[i]],
                                           [units[i][0] for i in idx], d_n[at:at + len(idx)], d_outl, [first[i] for i in idx],
                                           [counts[i] for i in idx], obase, [outs[i].data_ptr() - obase for i in idx])
            at += len(idx)
    return merge_into


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
    k, n = t.element_size(), t.numel()
    dev = t.device
    st = _pkg._plane_stream(dev, stream=None)
    poff, nbytes = _pkg.fields._layout([(n, k)])
    with torch.cuda.stream(st):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        bt = _pkg.Batch(1, 1 << 20)
        try:
            cap, found, d_outl = _pkg.fields.outlier_capacity(n), 0, None
            while n:
                d_outl, _, d_found, _ = _split_rounded(bt, st, dev, [t], [(n, k)], [lags], [keep], [cap], buf, poff)
                bt.finish(st, 1)
                found = int(d_found.cpu()[0])
                if found <= cap:
                    break
                cap = found
        finally:
            bt.close()
        pos, bits = _pkg.fields._sorted_records(d_outl[:found]) if found else (torch.empty(0, dtype=torch.int64, device=dev),) * 2
    torch.cuda.current_stream(dev).wait_stream(st)
    return buf[:k * _pkg._al16(n)].view(k, _pkg._al16(n))[:, :n], pos, bits


def restore_rounded(planes, dtype, shape, lags, keep_bits, positions, bits, stream=None):
    """round_field's inverse for one tensor: `planes` as merge_grid takes them -> a tensor of `dtype` and `shape`, every element
    the rounded value of its code but the outliers, whose `bits` are stored at their `positions`.  One
    merge_planes_grid_round_dev call, one synchronisation."""
    import torch
    what = "restore_rounded"
    if dtype not in MANTISSA_BITS:
        raise ValueError(f"{what}: float16, bfloat16, float32 and float64 tensors, not {dtype!r}")
    k, shape, n = _pkg._plane_dtype(what, dtype, shape)
    lags = _lag_set(what, lags)
    keep = _keep(what, keep_bits, dtype)
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or not planes.is_cuda or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError(f"{what}: planes is a uint8 CUDA tensor [k, numel] with contiguous rows")
    if tuple(planes.shape) != (k, n):
        raise ValueError(f"{what}: planes of shape {tuple(planes.shape)} for {k} x {n} bytes")
    _pkg.fields._records(what, positions, bits, planes.device)
    dev = planes.device
    item = CompressedRounded(dtype, shape, lags, keep, [], positions, bits, 0)
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        out = torch.empty(shape, dtype=dtype, device=dev)
        bt = _pkg.Batch(1, 1 << 20)
        try:
            _merge_rounded([item], [keep])(bt, st, dev, [[planes[j].contiguous() for j in range(k)]], [out], [(n, k)], "planes_grid",
                                           [lags])
            bt.finish(st, 1)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return out


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
    import torch
    what = "compress_rounded"
    ts = _rounded_tensors(what, tensors)
    lags = _rounded_lags(what, ts, axes, lags)
    keeps = _keeps(what, ts, keep_bits)
    if isinstance(block_size, bool) or not isinstance(block_size, int) or not 0 <= block_size < 1 << 64:
        raise ValueError(f"{what}: block_size is a size in bytes (shafa_block_count's uint64_t)")
    if not ts:
        return []
    F = _pkg.fields
    dev = ts[0].device
    units = _pkg._elements(ts)
    caps = [F.outlier_capacity(n) if n else 0 for n, _ in units]
    poff, nbytes = F._layout(units)
    st = _pkg._plane_stream(dev, stream)
    found = [0] * len(ts)
    with torch.cuda.stream(st):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        bt = _pkg.Batch(len(ts), 1 << 20)
        try:
            if any(n for n, _ in units):
                d_outl, first, d_found, order = _split_rounded(bt, st, dev, ts, units, lags, keeps, caps, buf, poff)
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
            pos, bits = F._sorted_records(d_outl[first[i]:first[i] + found[i]]) if keep else (none, none)
            items.append(CompressedRounded(t.dtype, t.shape, lags[i], None if i in lossless else keeps[i], ps, pos, bits,
                                           nb + (8 + t.element_size()) * int(pos.numel())))
    torch.cuda.current_stream(dev).wait_stream(st)
    return items


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
    lags, keeps = [], []
    for it in items:
        if it.dtype not in MANTISSA_BITS:
            raise ValueError(f"{what}: float16, bfloat16, float32 and float64 tensors, not {it.dtype!r}")
        lags.append(_lag_set(what, it.lags))
        _pkg.fields._records(what, it.outlier_pos, it.outlier_bits, None)
        if it.keep_bits is None and it.outlier_pos.numel():
            raise ValueError(f"{what}: an item kept lossless has no outliers")
        keeps.append(None if it.keep_bits is None else _keep(what, it.keep_bits, it.dtype))
    return _pkg._merge_items(what, items, "planes_grid", lags, False, stream, _merge_rounded(list(items), keeps))


# ---- sizes at a number of kept bits: the rounding split's histograms without the planes (Batch.hist_planes_grid_round_dev)
def _model_sizes(ts, blocks, stream):
    """blocks: (index of a non-empty tensor of ts, lags, keep) -> [(nbytes, outliers)] in their order, nbytes field_sizes' order-0
    model.  Per element size one hist_planes_grid_round_dev, Module T and the encoded sizes on the device; one finish, one
    read-back"""
    import ctypes as C
    import torch
    dev = ts[0].device
    st = _pkg._plane_stream(dev, stream)
    widths = sorted({ts[i].element_size() for i, _, _ in blocks})
    groups = [(w, [j for j, (i, _, _) in enumerate(blocks) if ts[i].element_size() == w]) for w in widths]
    with torch.cuda.stream(st):
        bt = _pkg.Batch(max(len(g) * w for w, g in groups), 1 << 20)
        try:
            res = []
            for w, g in groups:
                idx = [blocks[j][0] for j in g]
                base = min(ts[i].data_ptr() for i in idx)
                numel = [ts[i].numel() for i in idx]
                d_n = torch.tensor(numel, dtype=torch.int64, device=dev)
                d_freq = torch.empty(len(g) * w * 256, dtype=torch.int64, device=dev)
                d_outl = torch.empty(len(g), dtype=torch.int64, device=dev)
                bt.hist_planes_grid_round_dev(st, w, [_device_lags(blocks[j][1], n) for j, n in zip(g, numel)],
                                              [MANTISSA_BITS[ts[i].dtype] for i in idx], [blocks[j][2] for j in g], base,
                                              [ts[i].data_ptr() - base for i in idx], numel, d_n, d_freq, d_outl)
                d_tab = torch.empty(len(g) * w * C.sizeof(_pkg.CodeTable), dtype=torch.uint8, device=dev)
                bt.sf_build_codes(st, len(g) * w, d_freq, d_tab)
                d_enc = torch.zeros(len(g) * w, dtype=torch.int64, device=dev)
                bt.sf_encoded_size_dev(st, len(g) * w, d_freq, d_tab, d_enc)
                planes = torch.minimum(d_enc.view(len(g), w), d_n[:, None]).sum(1)
                res.append(torch.stack([planes + (8 + w) * d_outl, d_outl], 1))
            bt.finish(st, bt.max_blocks)
            host = torch.cat(res).cpu().tolist()
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    out = [None] * len(blocks)
    for j, (nb, no) in zip([j for _, g in groups for j in g], host):
        out[j] = (int(nb), int(no))
    return out


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
    dev, k, n = t.device, t.element_size(), t.numel()
    if isinstance(keep_bits, (list, tuple)):
        if len(keep_bits) != len(sets):
            raise ValueError(f"{what}: keep_bits is an int or a list with one int per entry of lag_sets")
        keeps = [_keep(what, e, t.dtype) for e in keep_bits]
    else:
        keeps = [_keep(what, keep_bits, t.dtype)] * len(sets)
    mant = MANTISSA_BITS[t.dtype]
    group = _pkg.grids.HIST_GROUP
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        freq = torch.zeros(len(sets), k, 256, dtype=torch.int64, device=dev)
        outl = torch.zeros(len(sets), dtype=torch.int64, device=dev)
        if sets and n:
            bt = _pkg.Batch(min(len(sets), group), 1 << 20)
            try:
                d_n = torch.full((bt.max_blocks,), n, dtype=torch.int64, device=dev)
                for lo in range(0, len(sets), bt.max_blocks):
                    part, kp = sets[lo:lo + bt.max_blocks], keeps[lo:lo + bt.max_blocks]
                    bt.hist_planes_grid_round_dev(st, k, [_device_lags(c, n) for c in part], [mant] * len(part), kp, t,
                                                  [0] * len(part), [n] * len(part), d_n, freq[lo:lo + len(part)],
                                                  outl[lo:lo + len(part)])
                bt.finish(st, bt.max_blocks)
            finally:
                bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return freq, outl


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
    out = [[((), 0, 0)] if not t.numel() or not t.dim() else None for t in ts]
    blocks = [(i, c, keeps[i]) for i in range(len(ts)) if out[i] is None for c in cands[i]]
    if not blocks:
        return out
    found = [[] for _ in ts]
    for (i, c, _), (nb, no) in zip(blocks, _model_sizes(ts, blocks, stream)):
        found[i].append((c, nb, no))
    cap = _pkg.fields.outlier_capacity
    key = lambda n: lambda e: (e[2] > cap(n), e[1], len(e[0]), e[0])
    return [o if o is not None else sorted(f, key=key(t.numel())) for o, f, t in zip(out, found, ts)]


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
    if not ts[0].numel() or not ts[0].dim():
        return [(k, 0, 0) for k in keeps]
    sizes = _model_sizes(ts, [(0, g, k) for k in keeps], stream)
    return [(k, nb, no) for k, (nb, no) in zip(keeps, sizes)]


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

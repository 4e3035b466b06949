"""Lorenzo differences — the differences along up to three axes at once — one file set per byte plane: split_grid / merge_grid and
compress_grids / decompress_grids on top of Batch.split_planes_grid_dev / merge_planes_grid_dev (csrc/planes_lag.hip;
include/shafa_hip.h: "Byte planes of Lorenzo differences").

compress_strided takes the difference along ONE axis.  A 2-D or 3-D simulation field, a stack of images, [step, y, x] snapshots
are smooth along several axes at once, and one axis alone leaves most of that in place: there the integer Lorenzo predictor of
the scientific-data codecs pays, the differences along every axis in turn, on the bit patterns.

The drivers live in this submodule; the package re-exports them.  What is the grid's own is here: how axes become a tuple of
lags, and the item.  The chains are the package's, compress_tensors' and decompress_tensors' with "planes_grid" as the variant and
the tuples of lags where "planes_lag" has its lags (_plane_entries, _merge_items, _split_one, _merge_one), reached through the
package at the time of the call.

Which lags pay is the data's to say: grid_histograms / grid_sizes / choose_lags on top of Batch.hist_planes_grid_dev count the
candidates' planes without making them and rank the candidates by an order-0 model of their size."""
import ctypes as C
import itertools
import sys

_pkg = sys.modules[__package__]


class CompressedGrid:
    """A tensor compressed by byte plane as its differences along up to three lags (compress_grids), in memory: `dtype` and
    `shape` of the original, `lags` — the tuple of distances in elements of the flattened tensor, increasing — `planes` — one
    entry per byte of the element, plane 0 the least significant, of the zigzag-folded differences: the dict compress_many
    returns for that plane's bytes, or the plane itself (a uint8 CUDA tensor) where coding it would not shrink it — and `nbytes`,
    the sum of the file lengths and of the raw planes' lengths.  Not a CompressedTensor: decompress_grids alone gives the tensor
    back."""
    __slots__ = ("dtype", "shape", "lags", "planes", "nbytes")

    def __init__(self, dtype, shape, lags, planes, nbytes):
        self.dtype, self.shape, self.lags, self.planes, self.nbytes = dtype, tuple(shape), lags, list(planes), int(nbytes)

    def __repr__(self):
        kinds = ["raw" if not isinstance(p, dict) else "+".join(sorted(p)) for p in self.planes]
        return f"CompressedGrid({self.dtype}, {self.shape}, lags={self.lags}, planes={kinds}, nbytes={self.nbytes})"


def _lag_tuple(what, lags):
    """a tuple of 1 .. PLANES_GRID_LAGS strictly increasing lags, checked"""
    if not isinstance(lags, (list, tuple)) or not 1 <= len(lags) <= _pkg.PLANES_GRID_LAGS:
        raise ValueError(f"{what}: lags are a tuple of 1 .. {_pkg.PLANES_GRID_LAGS} ints, not {lags!r}")
    lags = tuple(_pkg.strided._lag(what, g) for g in lags)
    if any(a >= b for a, b in zip(lags, lags[1:])):
        raise ValueError(f"{what}: lags are strictly increasing, not {lags!r}")
    return lags


def _axes_lags(what, shape, axes):
    """the lags of `axes` (a tuple of ints, or None: the last three axes, or all of fewer) of a tensor of `shape`: each axis's lag
    (strided._axis_lag), duplicates — axes of dimension 1 make them — dropped, sorted; (1,) for a 0-dimensional or an empty one"""
    shape = tuple(int(d) for d in shape)
    if axes is None:
        axes = tuple(range(max(0, len(shape) - _pkg.PLANES_GRID_LAGS), len(shape))) or (0,)
    if not isinstance(axes, (list, tuple)) or not axes:
        raise ValueError(f"{what}: axes are a tuple of ints, not {axes!r}")
    lags = tuple(sorted({_pkg.strided._axis_lag(what, shape, a) for a in axes}))
    if len(lags) > _pkg.PLANES_GRID_LAGS:
        raise ValueError(f"{what}: axes {tuple(axes)} of a tensor of shape {shape} make {len(lags)} distinct lags, more than "
                         f"{_pkg.PLANES_GRID_LAGS}")
    return lags


def _lags(what, ts, axes, lags):
    """one tuple of lags per checked tensor, from `lags` (None, a tuple of ints or a list of tuples) or else from `axes` (None, a
    tuple of ints or a list of tuples)"""
    def per_tensor(v, name):
        if isinstance(v, list):
            if len(v) != len(ts) or any(isinstance(x, int) for x in v):
                raise ValueError(f"{what}: {name} is a tuple of ints or a list with one tuple per tensor")
            return list(v)
        return [v] * len(ts)
    if lags is not None:
        return [_lag_tuple(what, g) for g in per_tensor(lags, "lags")]
    return [_axes_lags(what, t.shape, a) for t, a in zip(ts, per_tensor(axes, "axes"))]


def split_grid(t, lags, stream=None):
    """The byte planes of the differences along `lags` (a tuple of 1 .. 3 strictly increasing ints >= 1, in elements of the
    flattened tensor) of a contiguous CUDA tensor with elements of k = 1, 2, 4 or 8 bytes: a uint8 tensor [k, numel], row j byte
    j of the zigzag fold of ((1 - S^L1)(1 - S^L2)(1 - S^L3) x) mod 2^(8 k), x the elements as unsigned integers and 0 in front of
    the tensor, S^L the shift by L elements.  Rows start at multiples of 16 bytes, as split_planes'.  One split_planes_grid_dev
    launch, one synchronisation."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("split_grid: a contiguous CUDA tensor")
    t = _pkg._plane_tensors("split_grid", t)[0]
    lags = _lag_tuple("split_grid", lags)
    return _pkg._split_one("planes_grid", t, t.numel(), t.element_size(), stream, [lags])


def merge_grid(planes, dtype, shape, lags, stream=None):
    """split_grid's inverse for one tensor: `planes` as merge_planes takes them, a uint8 CUDA tensor [k, numel] -> a tensor of
    `dtype` and `shape`: the unfolded differences summed up at every distance of `lags` in turn.  One merge_planes_grid_dev call,
    one synchronisation."""
    import torch
    k, shape, n = _pkg._plane_dtype("merge_grid", dtype, shape)
    lags = _lag_tuple("merge_grid", lags)
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or not planes.is_cuda or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError("merge_grid: planes is a uint8 CUDA tensor [k, numel] with contiguous rows")
    if tuple(planes.shape) != (k, n):
        raise ValueError(f"merge_grid: planes of shape {tuple(planes.shape)} for {k} x {n} bytes")
    return _pkg._merge_one("planes_grid", planes, dtype, shape, stream, [lags])


def compress_grids(tensors, axes=None, lags=None, block_size=8 << 20, stream=None):
    """compress_tensors of every tensor's differences ALONG SEVERAL AXES at once, the integer Lorenzo predictor — a 2-D or 3-D
    field, a stack of images, [step, y, x] snapshots.  `tensors` and `block_size` as compress_tensors takes them, and its argument
    ValueErrors.  `axes` is a tuple of ints for all tensors or a list with one tuple per tensor, negative values counting from
    the back; None: each tensor's last three axes, or all of them if it has fewer.  An axis becomes a lag as in compress_strided
    (the product of the dimensions behind it); duplicate lags — axes of dimension 1 make them — are dropped, the lags sorted, and
    more than three distinct ones are a ValueError.  A 0-dimensional or an empty tensor takes (1,).  `lags`, a tuple of 1 .. 3
    strictly increasing ints of 1 .. 2^64 - 1 or a list with one such tuple per tensor, overrides `axes`: the distances
    themselves, for flat buffers.  Returns one CompressedGrid per tensor, which decompress_grids gives back bit for bit, whatever
    the dtype and the values.

    The differences run over the FLATTENED tensor: d = (1 - S^L1)(1 - S^L2)(1 - S^L3) x, S^L the shift by L elements.  None starts
    afresh at the end of a row or a slab: a row's first element is taken against the last one of the row in front.  With one
    axis this is compress_strided's transform, with axes=(-1,) compress_sequences'.

    It does not always pay.  Every further difference doubles the variance of the noise the data carries: a smooth field of
    integers came out at a third of its best single axis, a noisy uint8 image larger with two axes than with one.
    Which axes pay is the caller's to know: nothing is tried both ways here.  choose_lags ranks the candidates from their planes'
    histograms, without the planes, and its pick goes into `lags`.

    Float fields are taken BIT FOR BIT here, mantissa bytes and all.  Under an absolute error bound compress_fields (fields.py)
    quantises inside the same split and differences the integer codes exactly: a smooth float32 field comes out several times
    smaller.

    Chain: compress_tensors', with one split_planes_grid_dev per element size in place of the plain split — one block a tensor
    with lags of its own, so the number of launches does not depend on the shapes; no temporary of the differences exists ->
    compressed_sizes -> compress_many, as there."""
    ts = _pkg._plane_tensors("compress_grids", tensors)
    lags = _lags("compress_grids", ts, axes, lags)
    entries, nbytes = _pkg._plane_entries("compress_grids", ts, _pkg._elements(ts), "planes_grid", lags, block_size, stream)
    return [CompressedGrid(t.dtype, t.shape, g, ps, nb) for t, g, ps, nb in zip(ts, lags, entries, nbytes)]


# ---- which lags pay: the planes' histograms without the planes (Batch.hist_planes_grid_dev)
HIST_GROUP = 4096               # grid_histograms: candidates per device batch and launch


def _candidate(what, c):
    """a candidate: () — plain planes — or a tuple that _lag_tuple takes"""
    if not isinstance(c, tuple):
        raise ValueError(f"{what}: a candidate is a tuple of lags, () for plain planes, not {c!r}")
    return c if c == () else _lag_tuple(what, c)


def _candidate_list(what, cs):
    if not isinstance(cs, list) or not cs:
        raise ValueError(f"{what}: candidates are a non-empty list of tuples of lags, not {cs!r}")
    return [_candidate(what, c) for c in cs]


def _subsets(lags):
    """() and every non-empty subset of a tuple of lags, fewer lags first: at most eight"""
    return [s for r in range(len(lags) + 1) for s in itertools.combinations(lags, r)]


def _default_candidates(what, shape, axes):
    """the candidates of a tensor of `shape` from its axis lags"""
    return _subsets(_axes_lags(what, shape, axes))


def _candidates(what, ts, axes, candidates):
    """one list of candidates per checked tensor: from `candidates` (a list of tuples for all tensors, or a list with one such
    list per tensor) or else () and the subsets of each tensor's axis lags (`axes` as compress_grids takes them)"""
    if candidates is None:
        return [_subsets(g) for g in _lags(what, ts, axes, None)]
    if isinstance(candidates, list) and any(isinstance(c, list) for c in candidates):
        if len(candidates) != len(ts):
            raise ValueError(f"{what}: candidates is a list of tuples or a list with one such list per tensor")
        return [_candidate_list(what, cs) for cs in candidates]
    return [_candidate_list(what, candidates)] * len(ts)


# The histogram loop and the model-size chain are written once, here, for every split that has them: `hist` makes the split's
# hist Batch call for one launch, hist(bt, st, width, lags, rows, region, offsets, counts, d_n, d_freq, d_outl) with `rows` the
# launch's entries of the caller's parameter rows, which the callable lays out as its entry takes them.  This module's own split has
# no quantiser and no outliers: `outliers` False, no count is made, and d_outl is None.  fields.py and rounding.py pass their
# Quantiser's `hist`.
def _plain_hist(bt, st, width, lags, rows, *rest):
    bt.hist_planes_grid_dev(st, width, lags, *rest[:-1])


def _histograms(hist, t, sets, rows, outliers, stream):
    """one block per entry of `sets` on the region of the checked tensor t, HIST_GROUP entries a launch -> (freq [len(sets), k,
    256], the outliers' counts [len(sets)] or None).  One batch of a launch's blocks, one finish"""
    import torch
    dev, k, n = t.device, t.element_size(), t.numel()
    st = _pkg._plane_stream(dev, stream)
    with torch.cuda.stream(st):
        freq = torch.zeros(len(sets), k, 256, dtype=torch.int64, device=dev)
        outl = torch.zeros(len(sets), dtype=torch.int64, device=dev) if outliers else None
        if sets and n:
            bt = _pkg.Batch(min(len(sets), HIST_GROUP), 1 << 20)
            try:
                d_n = torch.full((bt.max_blocks,), n, dtype=torch.int64, device=dev)
                for lo in range(0, len(sets), bt.max_blocks):
                    part = sets[lo:lo + bt.max_blocks]
                    hist(bt, st, k, part, rows[lo:lo + len(part)], t, [0] * len(part), [n] * len(part), d_n, freq[lo:lo + len(part)],
                         outl[lo:lo + len(part)] if outliers else None)
                bt.finish(st, bt.max_blocks)
            finally:
                bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return freq, outl


def _model_sizes(hist, ts, blocks, outliers, stream):
    """blocks: (index of a non-empty tensor of ts, lags, the block's parameter row) -> in their order the order-0 model of their
    planes' bytes, or with `outliers` [nbytes, count]: (8 + element size) bytes per outlier on top, and their count.  Per element
    size one hist launch over its blocks, Module T and the encoded sizes on the device; one finish, one read-back"""
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
                d_outl = torch.empty(len(g), dtype=torch.int64, device=dev) if outliers else None
                hist(bt, st, w, [blocks[j][1] for j in g], [blocks[j][2] for j in g], base, [ts[i].data_ptr() - base for i in idx],
                     numel, d_n, d_freq, d_outl)
                d_tab = torch.empty(len(g) * w * C.sizeof(_pkg.CodeTable), dtype=torch.uint8, device=dev)
                bt.sf_build_codes(st, len(g) * w, d_freq, d_tab)
                d_enc = torch.zeros(len(g) * w, dtype=torch.int64, device=dev)
                bt.sf_encoded_size_dev(st, len(g) * w, d_freq, d_tab, d_enc)
                planes = torch.minimum(d_enc.view(len(g), w), d_n[:, None]).sum(1)
                res.append(torch.stack([planes + (8 + w) * d_outl, d_outl], 1) if outliers else planes)
            bt.finish(st, bt.max_blocks)
            host = torch.cat(res).cpu().tolist()
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    out = [None] * len(blocks)
    for j, size in zip([j for _, g in groups for j in g], host):
        out[j] = size
    return out


def grid_histograms(t, lag_sets, stream=None):
    """The byte histograms of the planes split_grid(t, lags) would give for every `lags` of the list `lag_sets`, without the
    planes: `t` a contiguous CUDA tensor with elements of k = 1, 2, 4 or 8 bytes, every entry of `lag_sets` a tuple split_grid
    takes or () for plain planes (split_planes').  Returns an int64 CUDA tensor [len(lag_sets), k, 256]; every row sums to
    t.numel().  One hist_planes_grid_dev launch per HIST_GROUP candidates (the batch's max_blocks), one block per candidate on
    the same region, one synchronisation."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("grid_histograms: a contiguous CUDA tensor")
    t = _pkg._plane_tensors("grid_histograms", t)[0]
    if not isinstance(lag_sets, (list, tuple)):
        raise ValueError(f"grid_histograms: lag_sets is a list of tuples of lags, not {lag_sets!r}")
    sets = [_candidate("grid_histograms", c) for c in lag_sets]
    return _histograms(_plain_hist, t, sets, [None] * len(sets), False, stream)[0]


def grid_sizes(tensors, axes=None, candidates=None, stream=None):
    """How large would each candidate's planes be?  Per tensor a list of (lags, nbytes), sorted by (nbytes, len(lags), lags):
    the first entry is the candidate to take, among equals the one with the fewest lags.  `tensors` as compress_grids takes
    them.  `candidates` is a list of tuples for all tensors or a list with one such list per tensor, each tuple () — plain
    planes, compress_tensors — or a tuple of lags as compress_grids' `lags`; None: () and every non-empty subset of the
    tensor's axis lags (`axes` as compress_grids takes them: the last three axes by default), at most eight.  An empty or
    0-dimensional tensor gives [((), 0)] whatever the candidates.

    nbytes is a MODEL of the planes, of order 0: the sum over the candidate's byte planes of min(numel, the Shannon-Fano bytes
    of the whole plane under the table of its own histogram) — a plane that would not shrink counts raw, as compress_tensors
    keeps it.  It is not the size compress_grids reports: it knows nothing of RLE, of the split into blocks of block_size with
    a table each, or of the files' tables and headers (DESIGN 7.29 has both side by side).

    Chain: per element size one hist_planes_grid_dev over all tensors' candidates, one block per candidate on its tensor's
    region — the planes never exist, and no histogram comes to the host -> sf_build_codes -> sf_encoded_size_dev -> one finish,
    one read-back of the sizes."""
    what = "grid_sizes"
    ts = _pkg._plane_tensors(what, tensors)
    cands = _candidates(what, ts, axes, candidates)
    out = [[((), 0)] if not t.numel() or not t.dim() else None for t in ts]
    blocks = [(i, c, None) for i, t in enumerate(ts) if out[i] is None for c in cands[i]]
    if not blocks:
        return out
    found = [[] for _ in ts]
    for (i, c, _), nb in zip(blocks, _model_sizes(_plain_hist, ts, blocks, False, stream)):
        found[i].append((c, nb))
    return [o if o is not None else sorted(f, key=lambda e: (e[1], len(e[0]), e[0])) for o, f in zip(out, found)]


def choose_lags(tensors, axes=None, candidates=None, stream=None):
    """Which lags to compress each tensor with: grid_sizes' first entry per tensor, the candidate whose planes the order-0 model
    makes smallest, among equals the one with the fewest lags.  () says that plain planes win: compress_tensors.  Anything else
    goes to compress_grids(tensor, lags=[...]).  grid_sizes' arguments, chain and caveats."""
    return [sizes[0][0] for sizes in grid_sizes(tensors, axes, candidates, stream)]


def decompress_grids(items, stream=None):
    """compress_grids' inverse: `items` is a CompressedGrid or a list of them (their planes on one device) -> the list of
    tensors, each equal to the original bit for bit.

    Chain: decompress_tensors', with one merge_planes_grid_dev per element size in place of the plain merge: decompress_many over
    all coded planes -> the sums at every lag in turn straight into fresh tensors.  Anything that is not a CompressedGrid — a
    CompressedTensor of any kind, a CompressedStrided, a CompressedRecords — is refused with a ValueError before any device
    work, as is an item whose lags are no tuple of increasing ints >= 1.  decompress_tensors' errors otherwise."""
    if isinstance(items, CompressedGrid):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedGrid) for it in items):
        raise ValueError("decompress_grids: a CompressedGrid or a list of them (compress_grids' items)")
    lags = [_lag_tuple("decompress_grids", it.lags) for it in items]
    return _pkg._merge_items("decompress_grids", items, "planes_grid", lags, False, stream)

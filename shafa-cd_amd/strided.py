"""Differences along an axis, one file set per byte plane: split_strided / merge_strided and compress_strided /
decompress_strided on top of Batch.split_planes_lag_dev / merge_planes_lag_dev (csrc/planes_lag.hip; include/shafa_hip.h: "Byte
planes of lagged differences").

compress_sequences takes the difference of every element to the one in front of it in the FLATTENED tensor, which is the
neighbour along the last axis alone.  A [T, C] sensor log runs along T with its channels interleaved, an [H, W, 3] image along
W at distance 3 and along H at distance 3 W, a [steps, params] stack of checkpoints along steps: there the small difference is
the one to the element one axis stride — the LAG — in front.

The drivers live in this submodule; the package re-exports them.  What is the lag's own is here: how an axis becomes a lag,
and the item.  The chains are the package's, compress_tensors' and decompress_tensors' with "planes_lag" as the variant and the
lags where the XOR variant has its bases (_plane_entries, _merge_items, _split_one, _merge_one), reached through the package at
the time of the call."""
import sys

_pkg = sys.modules[__package__]


class CompressedStrided:
    """A tensor compressed by byte plane as its differences at a distance (compress_strided), in memory: `dtype` and `shape` of
    the original, `lag` — the distance in elements of the flattened tensor — `planes` — one entry per byte of the element, plane
    0 the least significant, of the zigzag-folded differences: the dict compress_many returns for that plane's bytes, or the
    plane itself (a uint8 CUDA tensor) where coding it would not shrink it — and `nbytes`, the sum of the file lengths and of
    the raw planes' lengths.  Not a CompressedTensor: decompress_strided alone gives the tensor back."""
    __slots__ = ("dtype", "shape", "lag", "planes", "nbytes")

    def __init__(self, dtype, shape, lag, planes, nbytes):
        self.dtype, self.shape, self.lag, self.planes, self.nbytes = dtype, tuple(shape), lag, list(planes), int(nbytes)

    def __repr__(self):
        kinds = ["raw" if not isinstance(p, dict) else "+".join(sorted(p)) for p in self.planes]
        return f"CompressedStrided({self.dtype}, {self.shape}, lag={self.lag}, planes={kinds}, nbytes={self.nbytes})"


def _lag(what, lag):
    if isinstance(lag, bool) or not isinstance(lag, int) or not 1 <= lag < 1 << 64:
        raise ValueError(f"{what}: a lag is an int of 1 .. 2^64 - 1 elements, not {lag!r}")
    return lag


def _axis_lag(what, shape, axis):
    """the lag of `axis` of a tensor of `shape`: the product of the dimensions behind it; 1 for a 0-dimensional or an empty one"""
    shape = tuple(int(d) for d in shape)
    if isinstance(axis, bool) or not isinstance(axis, int):
        raise ValueError(f"{what}: an axis is an int, not {axis!r}")
    if not shape:
        if axis not in (0, -1):
            raise ValueError(f"{what}: axis {axis} of a tensor of 0 dimensions")
        return 1
    if not -len(shape) <= axis < len(shape):
        raise ValueError(f"{what}: axis {axis} of a tensor of {len(shape)} dimensions")
    if _pkg._numel(shape) == 0:
        return 1
    return max(1, _pkg._numel(shape[axis % len(shape) + 1:]))


def _lags(what, ts, axis, lag):
    """one lag per checked tensor, from `lag` (None, an int or a list of ints) or else from `axis` (an int or a list of ints)"""
    def per_tensor(v, name):
        if isinstance(v, (list, tuple)):
            if len(v) != len(ts):
                raise ValueError(f"{what}: {name} is an int or a list with one int per tensor")
            return list(v)
        return [v] * len(ts)
    if lag is not None:
        return [_lag(what, g) for g in per_tensor(lag, "lag")]
    return [_axis_lag(what, t.shape, a) for t, a in zip(ts, per_tensor(axis, "axis"))]


def split_strided(t, lag, stream=None):
    """The byte planes of the differences at distance `lag` (an int >= 1, in elements of the flattened tensor) of a contiguous
    CUDA tensor with elements of k = 1, 2, 4 or 8 bytes: a uint8 tensor [k, numel], row j byte j of the zigzag fold of
    (x[i] - x[i - lag]) mod 2^(8 k), x the elements as unsigned integers and 0 in front of the tensor.  Rows start at
    multiples of 16 bytes, as split_planes'.  One split_planes_lag_dev launch, one synchronisation."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("split_strided: a contiguous CUDA tensor")
    t = _pkg._plane_tensors("split_strided", t)[0]
    lag = _lag("split_strided", lag)
    return _pkg._split_one("planes_lag", t, t.numel(), t.element_size(), stream, [lag])


def merge_strided(planes, dtype, shape, lag, stream=None):
    """split_strided's inverse for one tensor: `planes` as merge_planes takes them, a uint8 CUDA tensor [k, numel] -> a tensor of
    `dtype` and `shape`, the prefix sums at distance `lag` of the unfolded differences.  One merge_planes_lag_dev call, one
    synchronisation."""
    import torch
    k, shape, n = _pkg._plane_dtype("merge_strided", dtype, shape)
    lag = _lag("merge_strided", lag)
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or not planes.is_cuda or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError("merge_strided: planes is a uint8 CUDA tensor [k, numel] with contiguous rows")
    if tuple(planes.shape) != (k, n):
        raise ValueError(f"merge_strided: planes of shape {tuple(planes.shape)} for {k} x {n} bytes")
    return _pkg._merge_one("planes_lag", planes, dtype, shape, stream, [lag])


def compress_strided(tensors, axis=0, lag=None, block_size=8 << 20, stream=None):
    """compress_tensors of every tensor's differences ALONG AN AXIS — a [T, C] log along T, an [H, W, 3] image along H or W, a
    stack of checkpoints along its steps.  `tensors` and `block_size` as compress_tensors takes them, and its argument
    ValueErrors.  `axis` is an int for all tensors or a list with one int per tensor, negative values counting from the back;
    a tensor's lag is the product of its dimensions behind that axis, and 1 for a 0-dimensional or an empty tensor.  `lag`, an
    int >= 1 or a list with one per tensor, overrides `axis`: the distance itself, for flat buffers.  Returns one
    CompressedStrided per tensor, which decompress_strided gives back bit for bit, whatever the dtype and the values.

    The difference runs over the FLATTENED tensor at that distance: element i against element i - lag, the first lag elements
    kept as they are.  With axis > 0 the first row of every outer slab is therefore taken against the last row of the slab in
    front of it, not kept: the difference does not start afresh at a slab.  axis = -1 is compress_sequences' transform.

    Chain: compress_tensors', with one split_planes_lag_dev per element size in place of the plain split — one block a tensor
    with a lag of its own, so the number of launches does not depend on the shapes; no temporary of the differences exists ->
    compressed_sizes -> compress_many, as there.  Which axis pays is the caller's to know: nothing is tried both ways."""
    ts = _pkg._plane_tensors("compress_strided", tensors)
    lags = _lags("compress_strided", ts, axis, lag)
    entries, nbytes = _pkg._plane_entries("compress_strided", ts, _pkg._elements(ts), "planes_lag", lags, block_size, stream)
    return [CompressedStrided(t.dtype, t.shape, g, ps, nb) for t, g, ps, nb in zip(ts, lags, entries, nbytes)]


def decompress_strided(items, stream=None):
    """compress_strided's inverse: `items` is a CompressedStrided or a list of them (their planes on one device) -> the list of
    tensors, each equal to the original bit for bit.

    Chain: decompress_tensors', with one merge_planes_lag_dev per element size in place of the plain merge: decompress_many
    over all coded planes -> the prefix sums down the lag's columns straight into fresh tensors.  Anything that is not a
    CompressedStrided — a CompressedTensor of any kind, a CompressedRecords — is refused with a ValueError before any device
    work, as is an item whose lag is no int >= 1.  decompress_tensors' errors otherwise."""
    if isinstance(items, CompressedStrided):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedStrided) for it in items):
        raise ValueError("decompress_strided: a CompressedStrided or a list of them (compress_strided's items)")
    lags = [_lag("decompress_strided", it.lag) for it in items]
    return _pkg._merge_items("decompress_strided", items, "planes_lag", lags, False, stream)

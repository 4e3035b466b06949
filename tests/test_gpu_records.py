"""shafa_hipd_split_records_dev / shafa_hipd_merge_records_dev (csrc/records.hip) and the record drivers on top
(shafa-cd_amd/records.py) against numpy on the host: the columns of n records of w bytes are
np.frombuffer(raw, np.uint8).reshape(n, w).T, nothing is compared with device code — except where the point is that widths 1,
2, 4 and 8 give the plain plane entries' bytes.

The shapes are the smallest at which the kernels can go wrong: a lane takes 16 records of one column, a workgroup takes
P = records_pass(w) records through LDS at a time, a tile is T = RECORDS_TILE records, the record side lies at the byte
alignments 0, 1, 3, 8, 15, and the widths are the powers of two, their neighbours, and odd and even ones in between.  Every
buffer is 0xA5 where no data lies and is compared whole (test_gpu_planes' _Layout), so a byte written in front of a region,
behind a column's d_n bytes or into a guard shows up.  Per width, split and merge each run in ONE launch over all 60 blocks."""
import numpy as np
import pytest

import pkgload
from test_gpu_planes import ALIGN, FILL, _Layout, _bits, _fill, _planes_of, _same, _to
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64)


@pytest.fixture(scope="module")
def records(shafa):
    return pkgload.load_submodule("records")


def _counts(shafa, records, w):
    T, P = shafa.RECORDS_TILE, records.records_pass(w)
    return sorted({0, 1, 15, 16, 17, P - 1, P, P + 1, T - 1, T, T + 1, 3 * T + 5})


def _blocks(shafa, records, w):
    return [(n, a) for n in _counts(shafa, records, w) for a in ALIGN]


# ---------------------------------------------------------------- 1. the two kernels: every count at every alignment, one launch
@pytest.mark.parametrize("w", WIDTHS)
def test_split_against_numpy(shafa, records, w):
    import torch
    blocks = _blocks(shafa, records, w)
    L = _Layout(w, blocks, 4000 + w)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(64, 1 << 20)
    try:
        d_el, d_pl = _to(L.el), _fill(L.pl.size)
        for b, (n, a) in enumerate(blocks):
            assert (d_el.data_ptr() + L.off[b]) % 16 == a
        d_n = torch.tensor(L.n, dtype=torch.int64, device=_dev())
        bt.split_records_dev(st, w, d_el, L.off, [n + (b % 3) for b, n in enumerate(L.n)], d_n, d_pl, L.poff)
        assert bt.finish(st, len(blocks)) == (0, [0] * len(blocks)), w
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes(), w
        assert d_el.cpu().numpy().tobytes() == L.el.tobytes(), w
    finally:
        bt.close()


@pytest.mark.parametrize("w", WIDTHS)
def test_merge_against_numpy_and_round_trip(shafa, records, w):
    import torch
    blocks = _blocks(shafa, records, w)
    L = _Layout(w, blocks, 5000 + w)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(64, 1 << 20)
    try:
        d_n = torch.tensor(L.n, dtype=torch.int64, device=_dev())
        cap = [n + (b % 3) for b, n in enumerate(L.n)]
        # the columns numpy made -> the records
        d_pl, d_out = _to(L.pl), _fill(L.el.size)
        bt.merge_records_dev(st, w, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, len(blocks)) == (0, [0] * len(blocks)), w
        assert d_out.cpu().numpy().tobytes() == L.el.tobytes(), w
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes(), w
        # split -> merge, back to back on the stream, into another alignment
        L2 = _Layout(w, [(n, ALIGN[(ALIGN.index(a) + 2) % len(ALIGN)]) for n, a in blocks], 5000 + w)    # the same bytes
        assert L2.raw == L.raw
        d_el, d_mid, d_back = _to(L.el), _fill(L.pl.size), _fill(L2.el.size)
        bt.split_records_dev(st, w, d_el, L.off, L.n, d_n, d_mid, L.poff)
        bt.merge_records_dev(st, w, d_mid, L.poff, L.n, d_n, d_back, L2.off)
        assert bt.finish(st, len(blocks)) == (0, [0] * len(blocks)), w
        assert d_back.cpu().numpy().tobytes() == L2.el.tobytes(), w
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. mixed blocks in one launch
@pytest.mark.parametrize("w", (3, 12, 33, 64))
def test_nine_blocks_one_launch_one_past_its_capacity(shafa, records, w):
    import torch
    T, P = shafa.RECORDS_TILE, records.records_pass(w)
    ns = [17, 0, T + 1, 15, 3 * T + 5, 0, P - 1, 16, P + 1]
    L = _Layout(w, [(n, ALIGN[b % len(ALIGN)]) for b, n in enumerate(ns)], 60 + w)
    bad = 4
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = torch.tensor(dn, dtype=torch.int64, device=_dev())
        want = [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)]
        # split: the bad block's columns stay as they were
        d_el, d_pl = _to(L.el), _fill(L.pl.size)
        bt.split_records_dev(st, w, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        full_pl, full_el = L.pl.copy(), L.el.copy()
        L.blank(bad)
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes()
        assert d_el.cpu().numpy().tobytes() == full_el.tobytes()
        # merge: the bad block's region stays as it was
        d_pl, d_out = _to(full_pl), _fill(L.el.size)
        bt.merge_records_dev(st, w, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert d_out.cpu().numpy().tobytes() == L.el.tobytes()
        # a capacity of 0 has no tile: its block is still reported, alone and next to others
        d_n1 = torch.tensor([1, 16], dtype=torch.int64, device=_dev())
        d_pl = _fill(L.pl.size)
        bt.split_records_dev(st, w, d_el, L.off[:1], [0], d_n1, d_pl, L.poff[:w])
        assert bt.finish(st, 1, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [shafa.OUTSIDE_MODULE])
        bt.split_records_dev(st, w, d_el, [L.off[0], L.off[7]], [0, 16], d_n1, d_pl, L.poff[:w] + L.poff[7 * w:8 * w])
        assert bt.finish(st, 2, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [shafa.OUTSIDE_MODULE, 0])
        only7 = np.full(L.pl.size, FILL, np.uint8)
        for j in range(w):
            o = L.poff[7 * w + j]
            only7[o:o + 16] = full_pl[o:o + 16]
        assert d_pl.cpu().numpy().tobytes() == only7.tobytes()
        d_out = _fill(L.el.size)
        bt.merge_records_dev(st, w, _to(full_pl), L.poff[:w], [0], d_n1, d_out, L.off[:1])
        assert bt.finish(st, 1, raise_on_error=False) == (shafa.OUTSIDE_MODULE, [shafa.OUTSIDE_MODULE])
        assert d_out.cpu().numpy().tobytes() == bytes([FILL]) * L.el.size
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. a large block, a busy stream, runs of tiles per workgroup
def test_large_block_behind_a_busy_stream_one_finish(shafa):
    """2^20 + 3 records of 12 bytes, split and merged back behind a large torch kernel on the same stream; the size comes from
    a kernel on that stream too.  One finish."""
    import torch
    dev = _dev()
    w, n, a = 12, (1 << 20) + 3, 3
    L = _Layout(w, [(n, a)], 89)
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        half = torch.tensor([[n // 2, n - n // 2]], dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(st):
            busy = torch.empty(1 << 28, dtype=torch.float32, device=dev)
            busy.normal_()                                                 # 1 GiB written: a few hundred microseconds
            d_n = half.sum(dim=1)                                          # the size exists only behind it
            bt.split_records_dev(st, w, d_el, L.off, [n], d_n, d_pl, L.poff)
            bt.merge_records_dev(st, w, d_pl, L.poff, [n], d_n, d_out, L.off)
            assert bt.finish(st, 1) == (0, [0])
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes()
        assert d_out.cpu().numpy().tobytes() == L.el.tobytes()
    finally:
        bt.close()


@pytest.mark.parametrize("w", (3, 32))
def test_runs_of_tiles_per_workgroup(shafa, w):
    """32775 tiles in the capacities: three tiles a workgroup, runs that start in one block and end in the next, and most
    tiles behind their block's real size"""
    import torch
    T = shafa.RECORDS_TILE
    ns = [3 * T + 5, T + 1, 20000]
    cap = [3 * T + 5, 1 << 28, 20000]
    L = _Layout(w, [(n, ALIGN[(b + 1) % len(ALIGN)]) for b, n in enumerate(ns)], 70 + w)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = torch.tensor(ns, dtype=torch.int64, device=_dev())
        d_el, d_pl, d_out = _to(L.el), _fill(L.pl.size), _fill(L.el.size)
        bt.split_records_dev(st, w, d_el, L.off, cap, d_n, d_pl, L.poff)
        bt.merge_records_dev(st, w, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 3) == (0, [0, 0, 0])
        assert d_pl.cpu().numpy().tobytes() == L.pl.tobytes()
        assert d_out.cpu().numpy().tobytes() == L.el.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. widths 1, 2, 4, 8: the plain plane entries' bytes
@pytest.mark.parametrize("w", (1, 2, 4, 8))
def test_power_of_two_widths_equal_the_plane_entries(shafa, records, w):
    import torch
    T, P = shafa.RECORDS_TILE, records.records_pass(w)
    ns = [17, 0, T + 1, 15, 3 * T + 5, 1, P - 1, 16, P + 1]
    L = _Layout(w, [(n, ALIGN[b % len(ALIGN)]) for b, n in enumerate(ns)], 80 + w)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = torch.tensor(ns, dtype=torch.int64, device=_dev())
        d_el = _to(L.el)
        pl_r, pl_p = _fill(L.pl.size), _fill(L.pl.size)
        bt.split_records_dev(st, w, d_el, L.off, ns, d_n, pl_r, L.poff)
        bt.split_planes_dev(st, w, d_el, L.off, ns, d_n, pl_p, L.poff)
        out_r, out_p = _fill(L.el.size), _fill(L.el.size)
        bt.merge_records_dev(st, w, pl_p, L.poff, ns, d_n, out_r, L.off)
        bt.merge_planes_dev(st, w, pl_r, L.poff, ns, d_n, out_p, L.off)
        assert bt.finish(st, 9) == (0, [0] * 9)
        assert torch.equal(pl_r, pl_p) and torch.equal(out_r, out_p)
        assert pl_r.cpu().numpy().tobytes() == L.pl.tobytes() and out_r.cpu().numpy().tobytes() == L.el.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. the drivers
def _tensor(name):
    import torch
    g = torch.Generator().manual_seed(len(name) * 131 + sum(name.encode()))
    rnd = lambda n: torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
    make = {
        "u8-1000x3": lambda: rnd(3000).view(1000, 3),
        "fp32-4099x3": lambda: torch.randn((4099, 3), generator=g),
        "complex128-1023": lambda: torch.complex(torch.randn(1023, generator=g, dtype=torch.float64),
                                                 torch.randn(1023, generator=g, dtype=torch.float64)),
        "complex128-1024": lambda: torch.complex(torch.randn(1024, generator=g, dtype=torch.float64),
                                                 torch.randn(1024, generator=g, dtype=torch.float64)),
        "bf16-257x5": lambda: (torch.randn((257, 5), generator=g) * 0.02).to(torch.bfloat16),
        "u8-buffer-32": lambda: rnd(32 * 2500),
        "numel-0": lambda: torch.empty((3, 0, 2), dtype=torch.float16),
        "bool-4096x7": lambda: torch.randint(0, 2, (4096, 7), generator=g, dtype=torch.uint8).to(torch.bool),
        "int64-3000": lambda: torch.randint(0, 50000, (3000,), generator=g, dtype=torch.int64),
        "fp32-scalar": lambda: torch.tensor(-0.0, dtype=torch.float32),
        "int16-2048x12": lambda: torch.randint(-300, 300, (2048, 12), generator=g, dtype=torch.int16),
    }
    return make[name]().to(_dev())


# name -> (widths argument, the width it means)
SINGLE = {"u8-1000x3": (None, 3), "fp32-4099x3": (None, 12), "complex128-1023": (None, 16), "complex128-1024": (None, 16),
          "bf16-257x5": (None, 10), "u8-buffer-32": (32, 32), "numel-0": (None, 4), "bool-4096x7": (None, 7),
          "int64-3000": (None, 8), "fp32-scalar": (None, 4), "int16-2048x12": (None, 24)}


def _check_item(records, t, w, cr):
    import torch
    n = t.numel() * t.element_size() // w
    assert isinstance(cr, records.CompressedRecords) and cr.dtype == t.dtype and tuple(cr.shape) == tuple(t.shape)
    assert cr.width == w and len(cr.planes) == w
    total = 0
    for p in cr.planes:
        if isinstance(p, dict):
            assert n >= 1024 and sum(int(f.numel()) for f in p.values()) < n
            total += sum(int(f.numel()) for f in p.values())
        else:
            assert isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and int(p.numel()) == n
            total += n
    assert cr.nbytes == total
    if n < 1024:
        assert all(isinstance(p, torch.Tensor) for p in cr.planes)


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_round_trip_is_bit_exact(shafa, records, name):
    import torch
    t = _tensor(name)
    keep = t.clone()
    widths, w = SINGLE[name]
    cr = records.compress_records(t, widths=widths)
    assert len(cr) == 1
    _check_item(records, t, w, cr[0])
    back = records.decompress_records(cr)
    assert len(back) == 1 and _same(back[0], keep) and _same(t, keep), name
    assert _same(records.decompress_records(cr[0])[0], keep)               # a single item, not in a list
    # the raw columns are the numpy columns, and so are split_records' rows
    raw = _bits(keep).cpu().numpy().tobytes()
    n = len(raw) // w
    for j, p in enumerate(cr[0].planes):
        if isinstance(p, torch.Tensor):
            assert p.cpu().numpy().tobytes() == _planes_of(raw, n, w)[j].tobytes(), (name, j)
    rows = records.split_records(t, widths)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (w, n)
    assert rows.cpu().numpy().tobytes() == _planes_of(raw, n, w).tobytes()
    for p in (rows, rows.contiguous()):
        assert _same(records.merge_records(p, t.dtype, t.shape), keep), name
    if name == "fp32-4099x3":
        with pytest.raises(ValueError):
            records.merge_records(rows, t.dtype, (4098, 3))
        with pytest.raises(ValueError):
            records.compress_records(t.t())
        with pytest.raises(ValueError):
            records.compress_records([t, t.cpu()])
        with pytest.raises(ValueError):
            records.compress_records(t, widths=5)
        with pytest.raises(ValueError):
            shafa.compress_tensors(_tensor("complex128-1024"))             # as before: elements of 16 bytes


def test_eleven_tensors_of_five_widths_in_one_call(shafa, records):
    names = ("fp32-4099x3", "numel-0", "u8-1000x3", "complex128-1024", "fp32-scalar", "u8-buffer-32", "bf16-257x5", "int64-3000",
             "complex128-1023", "bool-4096x7", "int16-2048x12")
    widths = [12, None, 3, 16, None, 32, 2, None, 16, 1, 12]
    means = [12, 4, 3, 16, 4, 32, 2, 8, 16, 1, 12]
    assert len({m for m, n in zip(means, names) if n != "numel-0"}) >= 5
    ts = [_tensor(n) for n in names]
    keep = [t.clone() for t in ts]
    crs = records.compress_records(ts, widths=widths, block_size=65536)
    assert len(crs) == 11
    for t, w, cr in zip(ts, means, crs):
        _check_item(records, t, w, cr)
    back = records.decompress_records(crs)
    assert len(back) == 11
    for name, b, k in zip(names, back, keep):
        assert _same(b, k), name
    # the same items in another order and one of them twice
    order = [10, 3, 3, 0, 9]
    for i, b in zip(order, records.decompress_records([crs[i] for i in order])):
        assert _same(b, keep[i]), names[i]


# ---------------------------------------------------------------- 6. what a column is, and what the split is worth
def _rgb(n=262144):
    """RGB uint8 pixels, the channels N(200, 10), N(90, 25) and N(20, 5), rounded and clipped to 0 .. 255"""
    rng = np.random.default_rng(1)
    ch = [np.clip(np.rint(rng.normal(m, s, n)), 0, 255).astype(np.uint8) for m, s in ((200, 10), (90, 25), (20, 5))]
    return np.stack(ch, axis=1)


def _log_records(n=65536):
    """records of 32 bytes: four u32 below 1000, a u64 running timestamp (microseconds, steps below 1000), an fp32 N(0, 1), a
    byte below 4 and three zero bytes"""
    rng = np.random.default_rng(1)
    rec = np.zeros(n, dtype=[("a", "<u4", 4), ("t", "<u8"), ("x", "<f4"), ("k", "u1"), ("z", "u1", 3)])
    assert rec.dtype.itemsize == 32
    rec["a"] = rng.integers(0, 1000, (n, 4))
    rec["t"] = 1_700_000_000_000_000 + np.cumsum(rng.integers(1, 1000, n))
    rec["x"] = rng.normal(0, 1, n)
    rec["k"] = rng.integers(0, 4, n)
    return rec.view(np.uint8).reshape(n, 32)


def _files_bytes(e):
    return sum(int(f.numel()) for f in e.values())


def test_columns_are_ordinary_file_sets(shafa, records):
    t = _to(_rgb(1 << 16))
    raw = t.cpu().numpy().tobytes()
    cr = records.compress_records(t, block_size=65536)[0]
    coded = [j for j, p in enumerate(cr.planes) if isinstance(p, dict)]
    assert coded
    for j in coded:
        col = _planes_of(raw, 1 << 16, 3)[j].tobytes()
        assert shafa.decompress_files(**shafa.plane_files(cr.planes[j])).cpu().numpy().tobytes() == col
        alone = shafa.compress_many(_to(np.frombuffer(col, np.uint8)), [len(col)], block_size=65536)[0]
        assert sorted(alone) == sorted(cr.planes[j])
        for key in alone:
            assert alone[key].cpu().numpy().tobytes() == cr.planes[j][key].cpu().numpy().tobytes(), (j, key)


def test_it_pays(shafa, records):
    """The first two rows of DESIGN 7.24's table, strict inequalities only.  The RGB image by column against the file set of
    its unsplit bytes; the 32-byte records by column against compress_tensors of the same bytes as int64, and that against the
    unsplit bytes.  The measured byte counts are in DESIGN 7.24."""
    import torch
    rgb = _to(_rgb())
    by_col = records.compress_records(rgb)[0]
    assert by_col.width == 3
    unsplit = _files_bytes(shafa.compress_many(rgb.view(-1), [rgb.numel()], block_size=8 << 20)[0])
    print(f"it pays: rgb by column {by_col.nbytes} bytes, unsplit {unsplit} bytes, raw {rgb.numel()} bytes")
    assert by_col.nbytes < unsplit
    assert _same(records.decompress_records(by_col)[0], rgb)

    log = _to(_log_records())
    by_col = records.compress_records(log)[0]
    assert by_col.width == 32
    as_i64 = shafa.compress_tensors(log.view(-1).view(torch.int64))[0]
    unsplit = _files_bytes(shafa.compress_many(log.view(-1), [log.numel()], block_size=8 << 20)[0])
    print(f"it pays: records by column {by_col.nbytes} bytes, as int64 planes {as_i64.nbytes} bytes, unsplit {unsplit} bytes, "
          f"raw {log.numel()} bytes")
    assert by_col.nbytes < as_i64.nbytes < unsplit
    assert _same(records.decompress_records(by_col)[0], log)


def test_corruption_is_reported(shafa, records):
    t = _to(_rgb(1 << 16))
    cr = records.compress_records(t)[0]
    CR = records.CompressedRecords
    j = [j for j, p in enumerate(cr.planes) if isinstance(p, dict)][0]
    entry = dict(cr.planes[j])
    key = ".rle.shaf" if ".rle.shaf" in entry else ".shaf"
    entry[key] = entry[key][:-1]                                           # a truncated .shaf
    planes = list(cr.planes)
    planes[j] = entry
    with pytest.raises(shafa.ShafaError):
        records.decompress_records(CR(cr.dtype, cr.shape, cr.width, planes, cr.nbytes - 1))
    planes[j] = _fill((1 << 16) - 16)                                      # a short column
    with pytest.raises(shafa.ShafaError) as e:
        records.decompress_records(CR(cr.dtype, cr.shape, cr.width, planes, 0))
    assert e.value.code == shafa.FILE_UNRECOGNIZABLE
    planes[j] = shafa.ShafaError(shafa.FILE_TOO_SMALL, "planted")
    with pytest.raises(shafa.ShafaError) as e:
        records.decompress_records(CR(cr.dtype, cr.shape, cr.width, planes, 0))
    assert e.value.code == shafa.FILE_TOO_SMALL
    assert _same(records.decompress_records(cr)[0], t)

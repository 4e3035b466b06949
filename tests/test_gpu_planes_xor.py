"""shafa_hipd_split_planes_xor_dev / shafa_hipd_merge_planes_xor_dev (csrc/planes.hip) and the delta drivers on top against
numpy on the host: the planes of n elements of k bytes against a base are
np.bitwise_xor(raw, base_raw).reshape(n, k).T on the raw bytes; nothing is compared with device code.

The shapes are test_gpu_planes.py's, the smallest at which the kernels can go wrong: a lane transposes 16 elements, a tile is
T = PLANES_TILE elements, and here the element side and the base side each lie at a byte alignment of their own — (0, 0) with
4096 elements or more takes the coalesced pass through LDS, every other pair the direct loads with the base's shift picked apart
from the element side's.  Three host images (element side, base side, plane side) are 0xA5 where no data lies, every region
has 16 guard bytes or more around it, and every comparison is of whole images.  All 256 (element, base) alignment pairs are
test_gpu_every_alignment.py's."""
import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
PAIRS = ((0, 0), (0, 1), (1, 0), (3, 3), (3, 8), (8, 15), (15, 4), (15, 15), (4, 0))    # (element, base) alignment mod 16
FILL = 0xA5
POISON = 0x3C


def _counts(shafa):
    T = shafa.PLANES_TILE
    return (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5)


def _al16(x):
    return (x + 15) // 16 * 16


def _planes_of(raw, n, k):
    return np.frombuffer(raw, np.uint8).reshape(n, k).T


def _xor(raw, base):
    return np.bitwise_xor(np.frombuffer(raw, np.uint8), np.frombuffer(base, np.uint8)).tobytes()


class _Layout:
    """blocks (n elements, element side at alignment a, base side at alignment ab or None: no base) of k-byte elements in three
    host images: `el` the element side, `ba` the base side, `pl` the planes of element XOR base (of the element where the block
    has no base), all FILL where no data lies; every region has 16 guard bytes or more on both sides.  A block without a base
    still has a place in `ba`, filled with POISON: its offset is what a launch must never look at."""

    def __init__(self, k, blocks, seed, a_out=None):
        rng = np.random.default_rng(seed)
        self.k, self.n = k, [n for n, _, _ in blocks]
        self.off, self.boff, self.poff, self.has = [], [], [], [ab is not None for _, _, ab in blocks]
        pos, bpos, ppos = 0, 0, 16
        for n, a, ab in blocks:
            pos = (pos + 16 + 63) // 64 * 64 + (a if a_out is None else a_out)
            self.off.append(pos)
            pos += n * k
            bpos = (bpos + 16 + 63) // 64 * 64 + (ab or 0)
            self.boff.append(bpos)
            bpos += n * k
            for _ in range(k):
                self.poff.append(ppos)
                ppos += _al16(n) + 32
        self.raw = [rng.integers(0, 256, n * k, dtype=np.uint8).tobytes() for n in self.n]
        # a base as a checkpoint's: most bytes the element's own, so that the XOR has zeros and non-zeros both
        self.braw = [np.where(rng.integers(0, 4, n * k) == 0, rng.integers(0, 256, n * k, dtype=np.uint8),
                              np.frombuffer(r, np.uint8)).astype(np.uint8).tobytes() for n, r in zip(self.n, self.raw)]
        self.el = np.full(pos + 80, FILL, np.uint8)
        self.ba = np.full(bpos + 80, FILL, np.uint8)
        self.pl = np.full(ppos + 16, FILL, np.uint8)
        for b, n in enumerate(self.n):
            self.el[self.off[b]:self.off[b] + n * k] = np.frombuffer(self.raw[b], np.uint8)
            self.ba[self.boff[b]:self.boff[b] + n * k] = np.frombuffer(self.braw[b], np.uint8) if self.has[b] else POISON
            x = _xor(self.raw[b], self.braw[b]) if self.has[b] else self.raw[b]
            for j in range(k):
                self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = _planes_of(x, n, k)[j]

    def base_off(self, shafa):
        return [o if h else shafa.PLANES_NO_BASE for o, h in zip(self.boff, self.has)]

    def blank(self, b):
        """block b leaves no trace in the element image or the plane image"""
        n, k = self.n[b], self.k
        self.el[self.off[b]:self.off[b] + n * k] = FILL
        for j in range(k):
            self.pl[self.poff[b * k + j]:self.poff[b * k + j] + n] = FILL


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(_dev())


def _fill(n):
    import torch
    return torch.full((n,), FILL, dtype=torch.uint8, device=_dev())


def _img(t):
    return t.cpu().numpy().tobytes()


def _ids(p):
    return f"el{p[0]}-base{p[1]}"


# ---------------------------------------------------------------- 1. the two kernels, block by block
@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("k", ELEMS)
def test_split_against_numpy(shafa, k, pair):
    import torch
    a, ab = pair
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, n in enumerate(_counts(shafa)):
            L = _Layout(k, [(n, a, ab)], 1000 * k + 100 * a + 10 * ab + i)
            d_el, d_ba, d_pl = _to(L.el), _to(L.ba), _fill(L.pl.size)
            assert (d_el.data_ptr() + L.off[0]) % 16 == a and (d_ba.data_ptr() + L.boff[0]) % 16 == ab
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            bt.split_planes_xor_dev(st, k, d_el, L.off, d_ba, L.boff, [n + 5], d_n, d_pl, L.poff)
            assert bt.finish(st, 1) == (0, [0]), (k, pair, n)
            assert _img(d_pl) == L.pl.tobytes(), (k, pair, n)
            assert _img(d_el) == L.el.tobytes() and _img(d_ba) == L.ba.tobytes(), (k, pair, n)
    finally:
        bt.close()


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("k", ELEMS)
def test_merge_against_numpy_and_round_trip(shafa, k, pair):
    import torch
    a, ab = pair
    a3 = [x for x in (5, 0, 12) if x not in pair][0]                       # a third alignment
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        for i, n in enumerate(_counts(shafa)):
            seed = 2000 * k + 100 * a + 10 * ab + i
            L = _Layout(k, [(n, a, ab)], seed)
            d_n = torch.tensor([n], dtype=torch.int64, device=_dev())
            # the planes numpy made, and the base -> the elements
            d_pl, d_ba, d_out = _to(L.pl), _to(L.ba), _fill(L.el.size)
            bt.merge_planes_xor_dev(st, k, d_pl, L.poff, d_ba, L.boff, [n + 5], d_n, d_out, L.off)
            assert bt.finish(st, 1) == (0, [0]), (k, pair, n)
            assert _img(d_out) == L.el.tobytes(), (k, pair, n)
            assert _img(d_pl) == L.pl.tobytes() and _img(d_ba) == L.ba.tobytes(), (k, pair, n)
            # split -> merge against the same base, back to back on the stream, into a third alignment
            L3 = _Layout(k, [(n, a, ab)], seed, a_out=a3)                  # the same bytes
            assert L3.raw == L.raw and L3.braw == L.braw
            d_el, d_mid, d_back = _to(L.el), _fill(L.pl.size), _fill(L3.el.size)
            assert (d_back.data_ptr() + L3.off[0]) % 16 == a3
            bt.split_planes_xor_dev(st, k, d_el, L.off, d_ba, L.boff, [n], d_n, d_mid, L.poff)
            bt.merge_planes_xor_dev(st, k, d_mid, L.poff, d_ba, L.boff, [n], d_n, d_back, L3.off)
            assert bt.finish(st, 1) == (0, [0]), (k, pair, n)
            assert _img(d_back) == L3.el.tobytes(), (k, pair, n)
            assert _img(d_mid) == L.pl.tobytes(), (k, pair, n)
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. many blocks in one launch, with and without a base
@pytest.mark.parametrize("k", ELEMS)
def test_nine_blocks_mixed_in_one_launch(shafa, k):
    """two blocks without a base (their place in the base image is poisoned and their planes are the plain entry's), an empty
    one, one past its capacity, five with bases at mixed alignments"""
    import torch
    T = shafa.PLANES_TILE
    ns = [17, 0, T + 1, 15, 3 * T + 5, 4100, T - 1, 16, T]
    al = [(3, 8), (0, 0), (0, None), (15, 4), (1, 0), (0, 0), (8, None), (0, 1), (4, 0)]
    L = _Layout(k, [(n, a, ab) for n, (a, ab) in zip(ns, al)], 30 + k)
    nobase, bad = (2, 6), 4
    assert [b for b in range(9) if not L.has[b]] == list(nobase) and ns[1] == 0
    cap = [n + (b % 3) for b, n in enumerate(ns)]
    dn = list(ns)
    dn[bad] = cap[bad] + 1
    boff = L.base_off(shafa)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(16, 1 << 20)
    try:
        d_n = torch.tensor(dn, dtype=torch.int64, device=_dev())
        want = [shafa.OUTSIDE_MODULE if b == bad else 0 for b in range(9)]
        # split: the block past its capacity leaves no trace
        d_el, d_ba, d_pl = _to(L.el), _to(L.ba), _fill(L.pl.size)
        bt.split_planes_xor_dev(st, k, d_el, L.off, d_ba, boff, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        full_pl = L.pl.copy()
        full_el = L.el.copy()
        L.blank(bad)
        got_pl = _img(d_pl)
        assert got_pl == L.pl.tobytes()
        assert _img(d_el) == full_el.tobytes() and _img(d_ba) == L.ba.tobytes()
        # the blocks without a base: what the plain entry writes, byte for byte
        d_plain = _fill(L.pl.size)
        d_n2 = torch.tensor([ns[b] for b in nobase], dtype=torch.int64, device=_dev())
        bt.split_planes_dev(st, k, d_el, [L.off[b] for b in nobase], [cap[b] for b in nobase], d_n2, d_plain,
                            [o for b in nobase for o in L.poff[b * k:(b + 1) * k]])
        assert bt.finish(st, 2) == (0, [0, 0])
        plain = _img(d_plain)
        for b in nobase:
            for j in range(k):
                o = L.poff[b * k + j]
                assert got_pl[o - 16:o + _al16(ns[b]) + 16] == plain[o - 16:o + _al16(ns[b]) + 16], (b, j)
        # merge: the bad block's region stays as it was
        d_pl, d_out = _to(full_pl), _fill(L.el.size)
        bt.merge_planes_xor_dev(st, k, d_pl, L.poff, d_ba, boff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_out) == L.el.tobytes()
        assert _img(d_pl) == full_pl.tobytes() and _img(d_ba) == L.ba.tobytes()
        # no block has a base: the plain entries' result throughout, d_base only has to be an address
        none = [shafa.PLANES_NO_BASE] * 9
        Lp = _Layout(k, [(n, a, None) for n, (a, _) in zip(ns, al)], 30 + k)
        assert Lp.raw == L.raw
        Lp.blank(bad)
        d_pl = _fill(L.pl.size)
        bt.split_planes_xor_dev(st, k, d_el, L.off, d_ba, none, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, 9, raise_on_error=False) == (shafa.OUTSIDE_MODULE, want)
        assert _img(d_pl) == Lp.pl.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. runs of tiles per workgroup
@pytest.mark.parametrize("k", (1, 4))
def test_runs_of_tiles_per_workgroup(shafa, k):
    """test_gpu_planes.py's sizes — 32775 tiles in the capacities: three tiles a workgroup, runs that start in one block and
    end in the next, most tiles behind their block's real size — with the element side and the base at different alignments"""
    import torch
    T = shafa.PLANES_TILE
    ns = [3 * T + 5, T + 1, 20000]
    cap = [3 * T + 5, 1 << 28, 20000]
    L = _Layout(k, [(n, a, ab) for n, (a, ab) in zip(ns, ((1, 8), (3, 0), (0, 15)))], 50 + k)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(4, 1 << 20)
    try:
        d_n = torch.tensor(ns, dtype=torch.int64, device=_dev())
        d_el, d_ba, d_pl, d_out = _to(L.el), _to(L.ba), _fill(L.pl.size), _fill(L.el.size)
        bt.split_planes_xor_dev(st, k, d_el, L.off, d_ba, L.boff, cap, d_n, d_pl, L.poff)
        bt.merge_planes_xor_dev(st, k, d_pl, L.poff, d_ba, L.boff, cap, d_n, d_out, L.off)
        assert bt.finish(st, 3) == (0, [0, 0, 0])
        assert _img(d_pl) == L.pl.tobytes()
        assert _img(d_out) == L.el.tobytes()
        assert _img(d_ba) == L.ba.tobytes()
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. compress_deltas -> decompress_deltas
NUMELS = (0, 17, 1000, 4096, 1 << 16)
DTYPES = ("bfloat16", "float16", "float32", "float64", "int64", "uint8")


def _bits(t):
    return t.reshape(-1).view(__import__("torch").uint8)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(_bits(a), _bits(b))


def _pair(dtype, n, seed, lead=0, base_lead=0):
    """a tensor and its base, n elements of `dtype`, both slices `lead` / `base_lead` elements into their storage.  The base is
    random bytes, so every NaN payload, both zeros and the denormals occur; the tensor is the base with one element in eight
    redrawn, and (floats) a stretch of zeros of the other sign and of NaNs with another payload."""
    import torch
    dt = getattr(torch, dtype)
    k = torch.empty((), dtype=dt).element_size()
    rng = np.random.default_rng(seed)
    braw = rng.integers(0, 256, (n, k), dtype=np.uint8)
    raw = np.where(rng.integers(0, 8, (n, 1)) == 0, rng.integers(0, 256, (n, k), dtype=np.uint8), braw).astype(np.uint8)
    if dt.is_floating_point and n >= 16:
        braw[0:4] = 0                                                      # + 0.0
        raw[0:4] = 0
        raw[0:4, k - 1] = 0x80                                             # - 0.0
        braw[4:8] = 0xFF                                                   # a NaN, every payload bit set
        raw[4:8] = 0xFF
        raw[4:8, 0] = 0xFE                                                 # the same NaN but for one payload bit
        raw[8:10], braw[8:10] = braw[4:6], raw[0:2]                        # a NaN over a zero, a zero over a NaN

    def put(x, lead):
        whole = torch.empty((lead + n + 3) * k, dtype=torch.uint8, device=_dev()).view(dt)
        t = whole[lead:lead + n]
        _bits(t).copy_(torch.from_numpy(x.reshape(-1)))
        assert t.is_contiguous() and t.storage_offset() == lead
        return t

    return put(raw, lead), put(braw, base_lead), raw.tobytes(), braw.tobytes()


def _check_delta(shafa, t, ct, xraw, has_base):
    """the item's type and fields, and every raw plane against numpy's plane of the XOR"""
    import torch
    k, n = t.element_size(), t.numel()
    assert type(ct) is (shafa.CompressedDelta if has_base else shafa.CompressedTensor)
    assert ct.dtype == t.dtype and tuple(ct.shape) == tuple(t.shape) and len(ct.planes) == k
    total = 0
    for j, p in enumerate(ct.planes):
        if isinstance(p, dict):
            assert n >= 1024 and sum(int(f.numel()) for f in p.values()) < n
            total += sum(int(f.numel()) for f in p.values())
            got = shafa.decompress_files(**shafa.plane_files(p))
        else:
            assert isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and int(p.numel()) == n
            total += n
            got = p
        assert got.cpu().numpy().tobytes() == _planes_of(xraw, n, k)[j].tobytes(), j
    assert ct.nbytes == total


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip_is_bit_exact(shafa, dtype):
    import zlib
    pairs = [_pair(dtype, n, 7 * i + len(dtype), lead=(0, 3, 1, 0, 5)[i], base_lead=(0, 1, 0, 7, 5)[i])
             for i, n in enumerate(NUMELS)]
    ts, bases = [p[0] for p in pairs], [p[1] for p in pairs]
    keep, keep_b = [t.clone() for t in ts], [b.clone() for b in bases]
    cts = shafa.compress_deltas(ts, bases)
    assert len(cts) == len(ts)
    for t, ct, (_, _, raw, braw) in zip(ts, cts, pairs):
        _check_delta(shafa, t, ct, _xor(raw, braw), True)
        assert ct.base_crc == zlib.crc32(braw)
    back = shafa.decompress_deltas(cts, bases)
    assert len(back) == len(ts)
    for n, b, k, t, kb, bs in zip(NUMELS, back, keep, ts, keep_b, bases):
        assert _same(b, k) and _same(t, k) and _same(bs, kb), (dtype, n)
    # one item alone, and without the digest on either side
    one = shafa.compress_deltas(ts[3], bases[3], check_base=False)
    assert len(one) == 1 and one[0].base_crc is None
    assert _same(shafa.decompress_deltas(one[0], bases[3])[0], keep[3])
    assert _same(shafa.decompress_deltas(one, [bases[3]], check_base=False)[0], keep[3])


def test_eleven_tensors_three_without_a_base(shafa):
    import torch
    spec = [("float32", 5000), ("float16", 0), ("int64", 4096), ("bfloat16", 65536), ("float32", 1), ("uint8", 4099),
            ("bfloat16", 1000), ("float64", 3000), ("int64", 1024), ("float16", 2049), ("float32", 1155)]
    pairs = [_pair(d, n, 300 + i, lead=i % 4, base_lead=(3 * i) % 5) for i, (d, n) in enumerate(spec)]
    ts = [p[0] for p in pairs]
    bases = [None if i in (2, 5, 9) else p[1] for i, p in enumerate(pairs)]
    keep = [t.clone() for t in ts]
    cts = shafa.compress_deltas(ts, bases, block_size=65536)
    assert len(cts) == 11
    for i, (t, ct, (_, _, raw, braw)) in enumerate(zip(ts, cts, pairs)):
        _check_delta(shafa, t, ct, raw if bases[i] is None else _xor(raw, braw), bases[i] is not None)
    # an item without a base is compress_tensors' item
    for i in (2, 5, 9):
        alone = shafa.compress_tensors(ts[i], block_size=65536)[0]
        assert cts[i].nbytes == alone.nbytes
        assert [sorted(p) if isinstance(p, dict) else None for p in cts[i].planes] == \
               [sorted(p) if isinstance(p, dict) else None for p in alone.planes]
    back = shafa.decompress_deltas(cts, bases)
    assert len(back) == 11
    for i, (b, k) in enumerate(zip(back, keep)):
        assert _same(b, k), spec[i]
    # the plain items alone go through decompress_tensors; another order, one item twice
    for i, b in zip((2, 5, 9), shafa.decompress_tensors([cts[i] for i in (2, 5, 9)])):
        assert _same(b, keep[i]), spec[i]
    order = [10, 3, 2, 3, 0]
    for i, b in zip(order, shafa.decompress_deltas([cts[i] for i in order], [bases[i] for i in order])):
        assert _same(b, keep[i]), spec[i]


def test_bases_back_to_back_are_digested_in_one_call(shafa, monkeypatch):
    """slices of one checkpoint buffer that follow each other without a gap: one crc32 call with `sizes` on either side of
    the round trip; with a gap between two of them, one call per base"""
    import torch
    import zlib
    calls = []
    real = shafa.crc32
    monkeypatch.setattr(shafa, "crc32", lambda d_in, sizes=None, **kw: (calls.append(sizes), real(d_in, sizes, **kw))[1])
    ns = (1000, 17, 4096)
    g = torch.Generator().manual_seed(5)
    whole = torch.randn(sum(ns) + 9, generator=g).to(_dev())
    for gap in (0, 1):
        starts = [3, 3 + ns[0] + gap, 3 + ns[0] + gap + ns[1]]
        bases = [whole[o:o + n] for o, n in zip(starts, ns)]
        ts = [(b * (torch.rand(n, generator=g) < 0.9).to(_dev())).contiguous() for b, n in zip(bases, ns)]
        calls.clear()
        cts = shafa.compress_deltas(ts, bases)
        assert calls == ([[4 * n for n in ns]] if gap == 0 else [None] * 3), gap
        assert [c.base_crc for c in cts] == [zlib.crc32(_bits(b).cpu().numpy().tobytes()) for b in bases]
        calls.clear()
        back = shafa.decompress_deltas(cts, bases)
        assert calls == ([[4 * n for n in ns]] if gap == 0 else [None] * 3), gap
        for t, b in zip(ts, back):
            assert _same(t, b), gap
        calls.clear()
        shafa.decompress_deltas(shafa.compress_deltas(ts, bases, check_base=False), bases)
        assert calls == []


# ---------------------------------------------------------------- 5. what the XOR is worth
def _small_weights(n):
    import torch
    return (torch.randn(n, generator=torch.Generator().manual_seed(1)) * 0.02).to(torch.bfloat16).to(_dev())


@pytest.mark.parametrize("dtype", ("bfloat16", "float32"))
def test_a_tensor_equal_to_its_base(shafa, oracle, dtype):
    """Every plane of the XOR is zeros: each is a file set, none is raw, and the item is below 1/50 of the tensor's bytes.
    The bound is the format's: a run of 255 becomes 3 RLE bytes, 1/85 before Shannon-Fano, and the files of a plane are its
    .rle, the .rle.shaf of that, and the two texts of a few hundred bytes.  The oracle's files for a 1 MiB block of zeros
    are 12 339 + 2 057 + 266 + 260 bytes and the .shaf's header, 1/70 of the block, and 3 087 + 515 + 266 + 260 for the
    256 KiB planes used here, 1/63 (at 64 KiB the two texts bring it to 1/46: the tensor has to be this large).  Twice the
    oracle's ratio is above 1/50, so 1/50 stands; the oracle's own ratio is asserted here too."""
    import torch
    n = 1 << 18
    z = np.zeros(n, np.uint8)
    rle = oracle.rle_encode(z)
    freq = oracle.hist256(rle)
    tab = oracle.sf_build(freq)
    rc, shaf = oracle.sf_encode(rle, tab)
    assert rc == 0
    ref = rle.size + len(oracle.freq_write_block(freq)) + len(oracle.cod_write_block(tab)) + shaf.size + 64
    print(f"oracle, {n} zeros: {ref} bytes with 64 for the .shaf's header, 1/{n / ref:.1f}")
    assert ref * 50 < n
    t = _small_weights(n) if dtype == "bfloat16" else torch.randn(n, generator=torch.Generator().manual_seed(2)).to(_dev())
    base = t.clone()
    ct = shafa.compress_deltas([t], [base])[0]
    print(f"{dtype} equal to its base: {ct.nbytes} bytes of {n * t.element_size()}")
    assert all(isinstance(p, dict) for p in ct.planes)
    assert ct.nbytes * 50 < n * t.element_size()
    assert _same(shafa.decompress_deltas([ct], [base])[0], t)


def test_it_pays(shafa):
    """bf16 weights of standard deviation 0.02, 2^20 of them, as a [1024, 1024] matrix in which one row in sixteen has moved
    by a relative 1e-3 against the base: the item of the XOR against the base is smaller than compress_tensors' item of the
    tensor alone.  Measured on an MI355X: 36 907 bytes for the delta against 1 404 471 for the tensor alone, of 2 097 152 (842 of
    the 65 536 elements of the moved rows differ from the base: a relative 1e-3 seldom crosses a bf16 rounding step)."""
    import torch
    base = _small_weights(1 << 20)
    noise = torch.randn(64, 1024, generator=torch.Generator().manual_seed(3)).to(_dev())
    new = base.clone().view(1024, 1024)
    new[::16] = (new[::16].float() * (1 + 1e-3 * noise)).to(torch.bfloat16)
    new = new.view(-1)
    changed = int((_bits(new).view(torch.int16) != _bits(base).view(torch.int16)).sum())
    delta = shafa.compress_deltas([new], [base])[0]
    alone = shafa.compress_tensors(new)[0]
    print(f"it pays: delta {delta.nbytes} bytes, alone {alone.nbytes} bytes, raw {2 * new.numel()} bytes, "
          f"{changed} elements differ from the base")
    assert delta.nbytes < alone.nbytes
    assert _same(shafa.decompress_deltas([delta], [base])[0], new)


def test_wrong_base(shafa):
    import torch
    t, base, _, _ = _pair("float32", 4096, 99, lead=1, base_lead=2)
    item = shafa.compress_deltas([t], [base])[0]
    wrong = base.clone()
    _bits(wrong)[4 * 1234 + 2] ^= 0x10                                     # one byte of element 1234
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_deltas([item], [wrong])
    assert e.value.code == shafa.FILE_UNRECOGNIZABLE and "item 0" in str(e.value)
    two = shafa.compress_deltas([t, t], [base, base])
    with pytest.raises(shafa.ShafaError) as e:
        shafa.decompress_deltas(two, [base, wrong])
    assert e.value.code == shafa.FILE_UNRECOGNIZABLE and "item 1" in str(e.value)
    # without the digest on both sides the same call hands out a tensor that is wrong in exactly that element
    blind = shafa.compress_deltas([t], [base], check_base=False)[0]
    assert blind.base_crc is None
    got = shafa.decompress_deltas([blind], [wrong], check_base=False)[0]
    diff = (_bits(got).view(-1, 4) != _bits(t).view(-1, 4)).any(dim=1).nonzero().view(-1).tolist()
    assert diff == [1234]
    assert _same(shafa.decompress_deltas([blind], [base])[0], t)
    # an item with a digest, checked or not, against the right base
    assert _same(shafa.decompress_deltas([item], [base], check_base=False)[0], t)
    with pytest.raises(ValueError, match="decompress_deltas"):
        shafa.decompress_tensors(item)
    with pytest.raises(ValueError):
        shafa.decompress_deltas([item], [None])
    with pytest.raises(ValueError):
        shafa.decompress_deltas([item], [base[:-1]])
    with pytest.raises(ValueError):
        shafa.decompress_deltas([item], [base.view(torch.int32)])
    with pytest.raises(ValueError):
        shafa.decompress_deltas(shafa.compress_tensors([t]), [base])

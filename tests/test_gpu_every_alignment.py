"""The word-shifting kernels at all 16 byte alignments: csrc/planes.hip's split and merge (plain, XOR against a base, differences),
csrc/records.hip and csrc/find.hip, against numpy and bytes.find on the host; nothing is compared with device code.

Each of these kernels reads or writes a region "at any byte alignment" with aligned 16-byte words and a shift whose dword part
Q is a template parameter and whose byte part r is a run-time operand of v_alignbyte.  The families' own files choose their
alignments from short lists (0, 1, 3, 8, 15 and the like); here every start 0 .. 15 meets every end (start + n E) mod 16, so
every instantiation and every r runs, with the edge logic — which aligned words may be loaded, which go out whole and which as
single bytes, what a lane hands to the lane behind — at every combination of the two.  shift_class names the instantiation an
address selects, and every test asserts over the real device addresses that all of them occur.

The references, the 0xA5 images compared WHOLE and the pattern-filled guards are the families' own (test_gpu_planes._Layout,
test_gpu_planes_xor._Layout, test_gpu_planes_diff._Layout, test_gpu_find._Run).  All blocks of one (variant, element size) go
through ONE launch per direction: the batch is made for as many blocks as the table has.  The tables are plain functions of
the tile and pass sizes, so tests/test_every_alignment_cpu.py checks without a GPU that they hold what they claim."""
import bisect

import numpy as np
import pytest

import pkgload
import test_gpu_find as fnd
import test_gpu_planes as pln
import test_gpu_planes_diff as dif
import test_gpu_planes_xor as xr
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
ALIGN16 = tuple(range(16))
PASS = 4096                                                                # the elements of one pass of a planes workgroup
WIDTHS = tuple(range(1, 65))
FIND_M = (1, 3, 4, 5, 17, 255)
FIND_TILE = 8192
BORDERS = (32, 2048, 8192)                                                 # find's lane, wave and tile


# ---------------------------------------------------------------- the instantiation an address selects
def shift_class(addr, kind):
    """(Q, r) of the region at `addr`.  kind "split" (planes' split, find_lane, the base side of the XOR kernels):
    switch (sh >> 2), r = sh & 3, sh = addr mod 16.  kind "merge" (merge_tile, merge_tile_diff, shift_at): the shift is
    16 - sh, and sh = 0 has an instantiation of its own, Q = 4."""
    sh = addr % 16
    if kind == "merge":
        return (4 if sh == 0 else ((16 - sh) & 15) >> 2, (16 - sh) & 3)
    assert kind == "split"
    return (sh >> 2, sh & 3)


def all_classes(kind):
    """every class an address can select: 4 x 4 for split; for merge Q = 0 .. 3 with every r but (0, 0), which is sh = 0 and
    so Q = 4 — five values of Q, 16 classes, one for each alignment"""
    return {shift_class(a, kind) for a in range(16)}


def _assert_classes(addrs, kind):
    got = {shift_class(a, kind) for a in addrs}
    assert len(all_classes(kind)) == 16 and got == all_classes(kind), (kind, sorted(all_classes(kind) - got))


# ---------------------------------------------------------------- the block tables (no GPU needed: test_every_alignment_cpu.py)
def _plane_counts(T):
    return tuple(range(34)) + (PASS - 1, PASS, PASS + 1, T - 1, T, T + 1, T + PASS + 17, 2 * T + 5)


def _plane_blocks(T):
    """(n, a): every alignment times every count.  0 .. 33 puts the region's end at every residue mod 16 at every start,
    through up to three units; the large counts take the coalesced pass through LDS (a = 0) and the direct path, end inside a
    pass, and have tiles whose first lane rebuilds the unit in front of it."""
    return [(n, a) for a in ALIGN16 for n in _plane_counts(T)]


def _xor_blocks(T):
    """(n, a, ab or None): all 256 (element, base) alignment pairs at the small counts, the large counts on the pairs where the
    choice between the LDS pass and the direct path differs (a = 0, ab = 0 or a = ab); every seventh block has no base"""
    blocks = [(n, a, ab) for a in ALIGN16 for ab in ALIGN16 for n in (1, 16, 17, 33)]
    blocks += [(n, a, ab) for a in ALIGN16 for ab in ALIGN16 if a == 0 or ab == 0 or a == ab for n in (PASS, PASS + 1, T + 1)]
    return [(n, a, None if b % 7 == 6 else ab) for b, (n, a, ab) in enumerate(blocks)]


def _record_blocks(P):
    """(n, a) for one width, P = records_pass(width)"""
    return [(n, a) for a in ALIGN16 for n in (1, 15, 16, 17, P + 1)]


def _find_sizes(m):
    return sorted({m, m + 1, 33, 2049, FIND_TILE + 1})


def _find_regions(m):
    """(n, a), size-major: region i lies at alignment i mod 16 (test_gpu_find._place)"""
    return [(n, a) for n in _find_sizes(m) for a in ALIGN16]


def _caps(ns):
    return [n + (b % 3) for b, n in enumerate(ns)]


# ---------------------------------------------------------------- comparing whole images
def _same_image(got_t, want, offs, per, blocks, what):
    """the device tensor's bytes are the host image's; else the first wrong byte and the block it belongs to (per: regions a
    block has in this image)"""
    got = got_t.cpu().numpy()
    if got.size == want.size and np.array_equal(got, want):
        return
    assert got.size == want.size, what
    i = int(np.flatnonzero(got != want)[0])
    r = max(bisect.bisect_right(offs, i) - 1, 0)
    b = r // per
    pytest.fail(f"{what}: byte {i} is {int(got[i]):#04x}, not {int(want[i]):#04x}: region {r % per} of block {b} "
                f"(count, alignment ...) = {blocks[b]}, byte {i - offs[r]} of the region")


_cache = {}


def _once(key, make):
    """a layout is computed once and shared; no test changes it"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _batch(shafa, nb):
    import torch
    return torch.cuda.Stream(device=_dev()), shafa.Batch(nb, 1 << 20)


def _dn(ns):
    import torch
    return torch.tensor(ns, dtype=torch.int64, device=_dev())


# ---------------------------------------------------------------- 1. plain planes
def _plain(shafa, k):
    blocks = _plane_blocks(shafa.PLANES_TILE)
    return blocks, _once(("plain", k), lambda: pln._Layout(k, blocks, 9100 + k))


@pytest.mark.parametrize("k", ELEMS)
def test_planes_split(shafa, k):
    blocks, L = _plain(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_el, d_pl = pln._to(L.el), pln._fill(L.pl.size)
        assert [(d_el.data_ptr() + o) % 16 for o in L.off] == [a for _, a in blocks] and d_pl.data_ptr() % 16 == 0
        _assert_classes([d_el.data_ptr() + o for o in L.off], "split")
        bt.split_planes_dev(st, k, d_el, L.off, _caps(L.n), _dn(L.n), d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"split, E = {k}, planes")
        _same_image(d_el, L.el, L.off, 1, blocks, f"split, E = {k}, the input")
    finally:
        bt.close()


@pytest.mark.parametrize("k", ELEMS)
def test_planes_merge_and_round_trip(shafa, k):
    blocks, L = _plain(shafa, k)
    blocks2 = [(n, (a + 9) % 16) for n, a in blocks]
    L2 = _once(("plain+9", k), lambda: pln._Layout(k, blocks2, 9100 + k))  # the same bytes at another alignment
    assert L2.raw == L.raw
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_n, cap = _dn(L.n), _caps(L.n)
        # the planes numpy made -> the elements
        d_pl, d_out = pln._to(L.pl), pln._fill(L.el.size)
        assert [(d_out.data_ptr() + o) % 16 for o in L.off] == [a for _, a in blocks]
        _assert_classes([d_out.data_ptr() + o for o in L.off], "merge")
        bt.merge_planes_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_out, L.el, L.off, 1, blocks, f"merge, E = {k}, elements")
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"merge, E = {k}, the input")
        # split -> merge back to back on the stream into alignment (a + 9) mod 16: every merge class gets device-made planes
        d_el, d_mid, d_back = pln._to(L.el), pln._fill(L.pl.size), pln._fill(L2.el.size)
        assert [(d_back.data_ptr() + o) % 16 for o in L2.off] == [a for _, a in blocks2]
        _assert_classes([d_back.data_ptr() + o for o in L2.off], "merge")
        bt.split_planes_dev(st, k, d_el, L.off, cap, d_n, d_mid, L.poff)
        bt.merge_planes_dev(st, k, d_mid, L.poff, cap, d_n, d_back, L2.off)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_back, L2.el, L2.off, 1, blocks2, f"split -> merge, E = {k}, elements")
        _same_image(d_mid, L.pl, L.poff, k, blocks, f"split -> merge, E = {k}, planes")
    finally:
        bt.close()


# ---------------------------------------------------------------- 2. planes of differences
def _diff_data(b, n, k, rng):
    """block b's n elements as raw bytes.  A third of the blocks random bit patterns (test_gpu_planes_diff's "random"); a third
    a walk that starts 3 below M and steps by up to 300 either way, so it wraps around M again and again (at one byte every
    step does); a third drawn from 0, 1, M/2 - 1, M/2, M - 1: every carry between the packed 8- and 16-bit lanes of pk_add /
    pk_sub, and both ends of the fold"""
    U = dif.UINT[k]
    M = 1 << (8 * k)
    if b % 3 == 0:
        return dif._data("random", n, k, rng)
    if b % 3 == 1:
        steps = rng.integers(-300, 301, n).astype(np.int64).astype(np.uint64)
        if n:
            steps[0] = np.uint64(M - 3)
        return np.cumsum(steps, dtype=np.uint64).astype(U).tobytes()
    edges = np.array([0, 1, M // 2 - 1, M // 2, M - 1], dtype=np.uint64).astype(U)
    return edges[rng.integers(0, 5, n)].tobytes()


def _diff(shafa, k):
    blocks = _plane_blocks(shafa.PLANES_TILE)

    def make():
        rng = np.random.default_rng(9200 + k)
        raw = [_diff_data(b, n, k, rng) for b, (n, _) in enumerate(blocks)]
        return dif._Layout(k, blocks, 0, raw=raw)

    return blocks, _once(("diff", k), make)


@pytest.mark.parametrize("k", ELEMS)
def test_diff_split(shafa, k):
    blocks, L = _diff(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_el, d_pl = dif._to(L.el), dif._fill(L.pl.size)
        assert [(d_el.data_ptr() + o) % 16 for o in L.off] == [a for _, a in blocks] and d_pl.data_ptr() % 16 == 0
        _assert_classes([d_el.data_ptr() + o for o in L.off], "split")
        bt.split_planes_diff_dev(st, k, d_el, L.off, _caps(L.n), _dn(L.n), d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"diff split, E = {k}, planes")
        _same_image(d_el, L.el, L.off, 1, blocks, f"diff split, E = {k}, the input")
    finally:
        bt.close()


@pytest.mark.parametrize("k", ELEMS)
def test_diff_merge_and_round_trip(shafa, k):
    blocks, L = _diff(shafa, k)
    blocks2 = [(n, (a + 9) % 16) for n, a in blocks]
    L2 = _once(("diff+9", k), lambda: dif._Layout(k, blocks2, 0, raw=L.raw))
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_n, cap = _dn(L.n), _caps(L.n)
        d_pl, d_out = dif._to(L.pl), dif._fill(L.el.size)
        assert [(d_out.data_ptr() + o) % 16 for o in L.off] == [a for _, a in blocks]
        _assert_classes([d_out.data_ptr() + o for o in L.off], "merge")
        bt.merge_planes_diff_dev(st, k, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_out, L.el, L.off, 1, blocks, f"diff merge, E = {k}, elements")
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"diff merge, E = {k}, the input")
        d_el, d_mid, d_back = dif._to(L.el), dif._fill(L.pl.size), dif._fill(L2.el.size)
        assert [(d_back.data_ptr() + o) % 16 for o in L2.off] == [a for _, a in blocks2]
        _assert_classes([d_back.data_ptr() + o for o in L2.off], "merge")
        bt.split_planes_diff_dev(st, k, d_el, L.off, cap, d_n, d_mid, L.poff)
        bt.merge_planes_diff_dev(st, k, d_mid, L.poff, cap, d_n, d_back, L2.off)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_back, L2.el, L2.off, 1, blocks2, f"diff split -> merge, E = {k}, elements")
        _same_image(d_mid, L.pl, L.poff, k, blocks, f"diff split -> merge, E = {k}, planes")
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. XOR with a base
def _xor(shafa, k):
    blocks = _xor_blocks(shafa.PLANES_TILE)
    return blocks, _once(("xor", k), lambda: xr._Layout(k, blocks, 9300 + k))


def _xor_addresses(L, d_el, d_ba, blocks):
    assert [(d_el.data_ptr() + o) % 16 for o in L.off] == [a for _, a, _ in blocks]
    based = [(d_ba.data_ptr() + o, ab) for o, (_, _, ab) in zip(L.boff, blocks) if ab is not None]
    assert [p % 16 for p, _ in based] == [ab for _, ab in based]
    _assert_classes([p for p, _ in based], "split")                        # xor_base's own switch
    pairs = {(a, ab) for _, a, ab in blocks if ab is not None}
    assert pairs == {(a, ab) for a in ALIGN16 for ab in ALIGN16}


@pytest.mark.parametrize("k", ELEMS)
def test_xor_split(shafa, k):
    blocks, L = _xor(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_el, d_ba, d_pl = xr._to(L.el), xr._to(L.ba), xr._fill(L.pl.size)
        _xor_addresses(L, d_el, d_ba, blocks)
        _assert_classes([d_el.data_ptr() + o for o in L.off], "split")
        bt.split_planes_xor_dev(st, k, d_el, L.off, d_ba, L.base_off(shafa), _caps(L.n), _dn(L.n), d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"xor split, E = {k}, planes")
        _same_image(d_el, L.el, L.off, 1, blocks, f"xor split, E = {k}, the input")
        _same_image(d_ba, L.ba, L.boff, 1, blocks, f"xor split, E = {k}, the base")
    finally:
        bt.close()


@pytest.mark.parametrize("k", ELEMS)
def test_xor_merge(shafa, k):
    blocks, L = _xor(shafa, k)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_pl, d_ba, d_out = xr._to(L.pl), xr._to(L.ba), xr._fill(L.el.size)
        _xor_addresses(L, d_out, d_ba, blocks)
        _assert_classes([d_out.data_ptr() + o for o in L.off], "merge")
        bt.merge_planes_xor_dev(st, k, d_pl, L.poff, d_ba, L.base_off(shafa), _caps(L.n), _dn(L.n), d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb), k
        _same_image(d_out, L.el, L.off, 1, blocks, f"xor merge, E = {k}, elements")
        _same_image(d_pl, L.pl, L.poff, k, blocks, f"xor merge, E = {k}, the input")
        _same_image(d_ba, L.ba, L.boff, 1, blocks, f"xor merge, E = {k}, the base")
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. records: every width
@pytest.fixture(scope="module")
def records(shafa):
    return pkgload.load_submodule("records")


@pytest.mark.parametrize("w", WIDTHS)
def test_records_split_and_merge(shafa, records, w):
    blocks = _record_blocks(records.records_pass(w))
    L = pln._Layout(w, blocks, 9400 + w)
    nb = len(blocks)
    st, bt = _batch(shafa, nb)
    try:
        d_n, cap = _dn(L.n), _caps(L.n)
        d_el, d_pl = pln._to(L.el), pln._fill(L.pl.size)
        assert [(d_el.data_ptr() + o) % 16 for o in L.off] == [a for _, a in blocks]
        _assert_classes([d_el.data_ptr() + o for o in L.off], "split")
        bt.split_records_dev(st, w, d_el, L.off, cap, d_n, d_pl, L.poff)
        assert bt.finish(st, nb) == (0, [0] * nb), w
        _same_image(d_pl, L.pl, L.poff, w, blocks, f"records split, width {w}, columns")
        _same_image(d_el, L.el, L.off, 1, blocks, f"records split, width {w}, the input")
        d_pl, d_out = pln._to(L.pl), pln._fill(L.el.size)
        assert [(d_out.data_ptr() + o) % 16 for o in L.off] == [a for _, a in blocks]
        _assert_classes([d_out.data_ptr() + o for o in L.off], "merge")
        bt.merge_records_dev(st, w, d_pl, L.poff, cap, d_n, d_out, L.off)
        assert bt.finish(st, nb) == (0, [0] * nb), w
        _same_image(d_out, L.el, L.off, 1, blocks, f"records merge, width {w}, records")
        _same_image(d_pl, L.pl, L.poff, w, blocks, f"records merge, width {w}, the input")
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. find
def _find_starts(n, m, a):
    """the region's first and last possible start, and at every border a match that straddles it (one byte: the byte in front
    of it and the one behind).  In a region of 33, 2049 or tile + 1 bytes the last possible start itself straddles the lane,
    wave or tile border for every m >= 2."""
    starts = [0, n - m]
    for B in BORDERS:
        starts += [B - 1, B] if m == 1 else [B - m // 2 - (a & 1)]
    return starts


@pytest.mark.parametrize("m", FIND_M)
def test_find(shafa, m):
    rng = fnd._rng(9500 + m)
    pat = fnd._rand(rng, m)
    table = _find_regions(m)
    regions = [fnd._planted(rng, n, pat, _find_starts(n, m, a)) for n, a in table]
    slack = [(7 * i) % 23 for i in range(len(regions))]
    r = fnd._Run(shafa, regions, None, pat, slack=slack, aligns=ALIGN16).check(f"m={m}")
    assert r.rc == 0 and not any(r.errs)
    assert [p % 16 for p in r.addr] == [a for _, a in table]
    _assert_classes(r.addr, "split")
    # the planted ones are there: the last possible start in every region that can hold the pattern, and the straddling ones
    for (n, a), reg, (i, c) in zip(table, regions, enumerate(r.counts)):
        if n >= m:
            assert c >= 1 and (i, n - m) in r.hits, (m, n, a)
    for B in BORDERS:
        if m >= 2:
            assert any(o < B < o + m for _, o in r.hits), (m, B)


# ---------------------------------------------------------------- 6. the drivers
DTYPES = ("uint8", "bfloat16", "float32", "int64")                         # one per element size


def _leads(dtype):
    import torch
    k = torch.empty((), dtype=getattr(torch, dtype)).element_size()
    return k, range(16 // k)


def _slices(dtype, n0=1536, kind="walk"):
    """for every lead 0 .. 16 / itemsize - 1 a slice whole[lead:lead + n] of `dtype`: a dtype view starts at a multiple of its
    item size, so these are all the alignments a driver can be handed"""
    k, leads = _leads(dtype)
    ts = [dif._tensor(dtype, n0 + 48 * lead, 9600 + lead, lead=lead, kind=kind)[0] for lead in leads]
    assert [t.data_ptr() % 16 for t in ts] == [lead * k for lead in leads]
    return ts


def test_find_driver_at_every_storage_offset(shafa):
    import torch
    rng = fnd._rng(9601)
    pat = b"dcbaabcdd"
    n = 2 * FIND_TILE + 77
    data = fnd._planted(rng, n, pat, [0, 23, FIND_TILE - 4, 2 * FIND_TILE - 1, n - len(pat)])
    ptrs = []
    for s in ALIGN16:                                                      # the pattern ends right in front and starts right behind
        front = (pat * 2)[len(pat) * 2 - s:]
        host = front + data + pat + bytes(32 - len(pat) - s)
        whole = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(_dev())
        view = whole[s:s + n]
        assert len(front) == s and view.data_ptr() % 16 == s
        ptrs.append(view.data_ptr())
        want = fnd._found(shafa, shafa.find(view, pat), data, pat)
        assert len(want) >= 5, s
    _assert_classes(ptrs, "split")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_drivers_round_trip_at_every_lead(shafa, dtype):
    ts = _slices(dtype)
    keep = [t.clone() for t in ts]
    back = shafa.decompress_tensors(shafa.compress_tensors(ts))
    assert len(back) == len(ts) and all(pln._same(b, k) for b, k in zip(back, keep)), dtype
    back = shafa.decompress_sequences(shafa.compress_sequences(ts))
    assert len(back) == len(ts) and all(pln._same(b, k) for b, k in zip(back, keep)), dtype
    assert all(pln._same(t, k) for t, k in zip(ts, keep)), dtype


@pytest.mark.parametrize("dtype", DTYPES)
def test_delta_driver_round_trip_at_every_lead(shafa, dtype):
    k, leads = _leads(dtype)
    nl = len(leads)
    pairs = [xr._pair(dtype, 1536 + 48 * lead, 9700 + lead, lead=lead, base_lead=(5 * lead + 3) % nl) for lead in leads]
    ts, bases = [p[0] for p in pairs], [p[1] for p in pairs]
    assert [t.data_ptr() % 16 for t in ts] == [lead * k for lead in leads]
    assert sorted(b.data_ptr() % 16 for b in bases) == [lead * k for lead in leads]       # a permutation: 5 is odd
    assert nl == 1 or any(t.data_ptr() % 16 != b.data_ptr() % 16 for t, b in zip(ts, bases))
    keep, keep_b = [t.clone() for t in ts], [b.clone() for b in bases]
    back = shafa.decompress_deltas(shafa.compress_deltas(ts, bases), bases)
    assert len(back) == nl and all(pln._same(b, kp) for b, kp in zip(back, keep)), dtype
    assert all(pln._same(t, kp) for t, kp in zip(ts, keep)) and all(pln._same(b, kp) for b, kp in zip(bases, keep_b)), dtype


@pytest.mark.parametrize("dtype,width", list(zip(DTYPES, (3, 6, 12, 24))))
def test_record_driver_round_trip_at_every_lead(shafa, records, dtype, width):
    ts = _slices(dtype)                                                    # 1536 + 48 lead elements: whole records at each width
    keep = [t.clone() for t in ts]
    items = records.compress_records(ts, widths=width)
    assert all(it.width == width for it in items)
    back = records.decompress_records(items)
    assert len(back) == len(ts) and all(pln._same(b, k) for b, k in zip(back, keep)), (dtype, width)
    assert all(pln._same(t, k) for t, k in zip(ts, keep)), (dtype, width)

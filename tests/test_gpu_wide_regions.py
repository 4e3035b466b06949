"""The seek, find, compare and CRC-32 kernels past one record per thread, against the CPU, with the helpers (slack bytes,
guard words, sentinels) of the files that test them at smaller sizes.

Each family ends in a blocks kernel of 256 threads a block of the file set, thread t holding the records
[t * per, (t + 1) * per) with per = ceil(records / 256), (compare_blocks: t, t + 256, ...), and starts with a tiles kernel
whose workgroups hold ceil(tiles / 16384) consecutive tiles of the call, whatever region they lie in.  A record is a span of
the seek index or an 8 KiB tile, so a thread holds more than one only in a block of more than 256 spans or a region of more
than 2 MiB, and a workgroup more than one tile only in a call of more than 128 MiB.  Those are the shapes here.  The
constants below mirror the kernels'; every test asserts from them, on the CPU, that the shape it is named after occurs
(test_the_wide_shapes_occur needs no GPU).

References: bytes.find in a loop; zlib.crc32; np.flatnonzero(a[:m] != ref[:m]); for the index the cumulative sum of the
oracle table's len[] and the Python walk of the .rle bytes (test_gpu_seek's _walk / _expected); for reads, slices of the
original."""
import bisect
import zlib

import numpy as np
import pytest

import test_gpu_compare as tc
import test_gpu_crc32 as tr
import test_gpu_find as tf
import test_gpu_seek as ts
from test_gpu_rle_measure import _count_calls
from test_gpu_unpack import _dev
from test_gpu_verify_files import _plant

gpu = pytest.mark.gpu

THREADS = 256                       # a blocks kernel's workgroup: a run of records per thread
T = 8192                            # a tile
TILE_WGS = 16384                    # workgroups of a tiles kernel: ceil(tiles / TILE_WGS) tiles each
SPAN_WAVES = 4 * 65536              # seek_spans: a span per wave, grid-stride behind this many
RS_LANES = 64                       # read_spans: spans of one item per workgroup
SPAN = 256


def _per(records):
    return -(-records // THREADS)


def _runs(records):
    """records held by each thread of a blocks kernel"""
    per = _per(records)
    return [max(0, min(records, (t + 1) * per) - min(records, t * per)) for t in range(THREADS)]


# ================================================================ 1. seek index and ranged reads
# (form, bytes, block size, span, spans of block 0).  Mode N: a span is `span` bytes of the block.  The RLE forms: of the
# block's .rle bytes, so the block sizes are those at which oracle.rle_encode of the runs stream gives these counts.
WIDE = [("N", 300000, 257 * SPAN, SPAN, 257), ("N", 300000, 512 * SPAN, SPAN, 512), ("N", 300000, 514 * SPAN, SPAN, 514),
        ("R", 300000, 89807, SPAN, 257), ("R", 200000, 179517, SPAN, 512), ("R", 200000, 180199, SPAN, 514),
        ("rle+freq", 300000, 89807, SPAN, 257), ("rle+freq", 200000, 179517, SPAN, 512),
        ("rle+freq", 200000, 180199, SPAN, 514),
        ("N", 655360 + 70000, 655360, 1024, 640), ("R", 655360 + 70000, 655360, 1024, 468)]     # the defaults: -b K, span 1024
WIDE_IDS = [f"{f}-{ns}x{s}" for f, _, _, s, ns in WIDE]


def _wide_ranges(starts, span):
    """the whole file, every whole block, and 65 * span, 128 * span + 1 and 3 bytes from 3 bytes in front of every multiple
    of 64 * span inside a block (starts: the decoded offsets of the blocks, and the decoded size)"""
    out = [(0, starts[-1])]
    for s0, s1 in zip(starts, starts[1:]):
        out.append((s0, s1 - s0))
        for at in range(s0 + RS_LANES * span, s1, RS_LANES * span):
            out += [(at - 3, 65 * span), (at - 3, 128 * span + 1), (at - 3, 3)]
    return out


def _ck_offsets(blocks, span, is_rle):
    """per block the decoded offsets of its checkpoints, from the CPU"""
    words, table = ts._expected(blocks, span, is_rle)
    return [[w[1] for w in words[f:f + max(1, -(-n // span))]] for _, n, f in table]


def _covered(starts, offs, ranges):
    """spans of one block that each (range, block) item covers: from the last checkpoint at or in front of its first byte to
    the last one in front of its end"""
    out = []
    for o, k in ranges:
        lo, hi = min(o, starts[-1]), min(o + k, starts[-1])
        for b, (s0, s1) in enumerate(zip(starts, starts[1:])):
            l, h = max(lo, s0) - s0, min(hi, s1) - s0
            if l < h:
                out.append(bisect.bisect_left(offs[b], h) - bisect.bisect_right(offs[b], l) + 1)
    return out


def _check_wide_reads(shafa, idx, data, kw, blocks, starts, span, is_rle, seeded):
    ranges = _wide_ranges(starts, span)
    cover = _covered(starts, _ck_offsets(blocks, span, is_rle), ranges)
    assert any(RS_LANES < c <= 2 * RS_LANES for c in cover) and max(cover) > 2 * RS_LANES      # two workgroups, and more
    ts._check_reads(shafa, idx, data, kw, ranges + seeded)


@gpu
@pytest.mark.parametrize("form,n,bs,span,ns0", WIDE, ids=WIDE_IDS)
def test_blocks_of_more_than_256_spans(shafa, oracle, form, n, bs, span, ns0):
    data, kw, blocks = ts._sets(shafa, oracle, n, bs)[form]
    ns = [-(-len(sfb) // span) for sfb, _ in blocks]
    assert ns[0] == ns0 > THREADS and _per(ns[-1]) == 1, ns                # a wide block and a short last one in one launch
    assert {_per(c[4]) for c in WIDE if c[0] == form and c[3] == SPAN} == {2, 3}
    held = _runs(ns0)
    if ns0 == 257:
        assert held[:128] == [2] * 128 and held[128] == 1 and not any(held[129:])
    elif ns0 == 512:
        assert held == [2] * THREADS
    elif ns0 == 514:
        assert held[:171] == [3] * 171 and held[171] == 1 and not any(held[172:])
    else:
        assert span == 1024 and bs == 655360 and _per(ns0) == (3 if form == "N" else 2)
    idx = shafa.build_index(span=span, **kw)
    ts._check_index(idx, blocks, span, form != "N")
    starts = list(range(0, n, bs)) + [n]
    _check_wide_reads(shafa, idx, data, kw, blocks, starts, span, form != "N", ts._ranges(n, bs, span, 7 + ns0))


# ---------------------------------------------------------------- RLE states inside a run and across waves, by hand
HAND_NS = 514
STATE1 = (4, 6, 384)                # checkpoints a triple's symbol byte follows: {0 | s, c}
STATE2 = (5, 9, 192)                # checkpoints a triple's count byte follows: {0, s | c}; the count of the last two is 0
STRETCH = (30, 33)                  # spans of nothing but {0, 5, 255}


def _hand_wide_blocks():
    rng = np.random.default_rng(6)
    lit = lambda k: rng.integers(1, 256, k).astype(np.uint8)
    a = lit(HAND_NS * SPAN)
    for j in STATE1:
        a[j * SPAN - 1:j * SPAN + 2] = (0, 10 + j % 7, 40 + j % 9)
    for j in STATE2:
        a[j * SPAN - 2:j * SPAN + 1] = (0, 20 + j % 7, 41 if j == 5 else 0)
    a[STRETCH[0] * SPAN:STRETCH[1] * SPAN] = np.tile(np.array([0, 5, 255], dtype=np.uint8), SPAN)
    return [a, lit(100)]


def _span_sums(seg):
    """what a piece of .rle adds to the decoded offset, per entry state"""
    out = []
    for state in (0, 1, 2):
        off = 0
        for v in seg.tolist():
            if state == 0:
                off, state = (off + 1, 0) if v else (off, 1)
            elif state == 1:
                state = 2
            else:
                off, state = off + (v if v else 1), 0
        out.append(off)
    return out


def _hand_wide_shapes():
    a = _hand_wide_blocks()[0]
    per = _per(HAND_NS)
    cks = ts._walk(a, SPAN)[0]
    assert len(cks) == HAND_NS and per == 3
    assert [cks[j][0] for j in STATE1] == [1, 1, 1] and [cks[j][0] for j in STATE2] == [2, 2, 2]
    assert [cks[j][1] for j in STATE2] == [20 + j % 7 for j in STATE2]                        # the pending symbols
    # inside a thread's run; on its first span; on the first span of a wave
    assert STATE1[0] % per and STATE2[0] % per and not STATE1[1] % per and not STATE2[1] % per
    assert STATE2[2] == 64 * per * 1 and STATE1[2] == 64 * per * 2 and STATE1[2] < HAND_NS
    assert a[STATE2[1] * SPAN] == 0 and a[STATE2[2] * SPAN] == 0                             # a count byte of 0 behind state 2
    # the stretch is one thread's whole run: entered in S0, its second span in S1, its third in S2, and what each span adds
    # depends on the state it is entered in
    lo, hi = STRETCH
    assert lo // per == (hi - 1) // per and hi - lo == per and [cks[j][0] for j in range(lo, hi)] == [0, 1, 2]
    assert cks[hi - 1][1] == 5 and a[(hi - 1) * SPAN] == 255
    for j in range(lo, hi):
        assert len(set(_span_sums(a[j * SPAN:(j + 1) * SPAN]))) == 3, j
    assert cks[hi][2] - cks[lo][2] == 255 * SPAN and cks[hi][0] == 0


@pytest.fixture(scope="module")
def hand_wide(shafa):
    return ts._hand_files(shafa, _hand_wide_blocks())


@gpu
@pytest.mark.parametrize("form", ["rle+freq", "R"])
def test_hand_made_states_inside_a_run(shafa, hand_wide, form):
    _hand_wide_shapes()
    blocks, data, kw_rle, kw_sf, lens = hand_wide
    kw = kw_rle if form == "rle+freq" else kw_sf
    assert len(lens) == 2
    idx = shafa.build_index(span=SPAN, **kw)
    eight = np.full(256, 8, dtype=np.int64)
    pairs = [(b, eight if form == "rle+freq" else l) for b, l in zip(blocks, lens)]
    ts._check_index(idx, pairs, SPAN, True)
    starts = [0, len(ts._rld(blocks[0])), len(data)]
    assert idx.starts == starts
    c = ts._walk(blocks[0], SPAN)[0]
    inside = [(c[STRETCH[0]][2] + 254, 100), (c[STRETCH[0] + 1][2] + 300, 100), (c[STRETCH[0] + 2][2] - 50, 100)]
    _check_wide_reads(shafa, idx, data, kw, pairs, starts, SPAN, True, inside + ts._ranges(len(data), 4096, SPAN, 3))


@gpu
def test_overwritten_payload_under_items_of_several_workgroups(shafa, oracle, monkeypatch):
    form, n, bs, span, ns0 = WIDE[5]
    data, kw, blocks = ts._sets(shafa, oracle, n, bs)[form]
    idx = shafa.build_index(span=span, **kw)
    starts = list(range(0, n, bs)) + [n]
    ranges = _wide_ranges(starts, span) + ts._ranges(n, bs, span, 5)[:40]
    assert max(_covered(starts, _ck_offsets(blocks, span, True), ranges)) > 2 * RS_LANES
    ts._overwrite_payloads(shafa, monkeypatch, form, kw, idx, n, ranges, [0])             # block 0, the wide one


# ---------------------------------------------------------------- more spans in one call than seek_spans has waves
BS8 = 8 << 20
N64 = (64 << 20) + (256 << 10)
_WIDE64 = {}


def _wide64(shafa):
    """form -> (original bytes, the same on the device, file arguments) of 64 MiB + 256 KiB in 8 MiB blocks, made once: mode N
    from a Zipf stream, mode R from runs short enough (a third of the bytes stand alone) that the .rle is longer than the
    input"""
    import torch
    if not _WIDE64:
        zt = ts._synth().zipf_table(1.2)
        rng = np.random.default_rng(64)
        plain = zt[rng.integers(0, 65536, N64, dtype=np.uint16)]
        k = (4 << 20) + 4099                                          # a piece that no block size divides
        piece = np.repeat(zt[rng.integers(0, 65536, k, dtype=np.uint16)], rng.geometric(0.8, k))[:k]
        runs = np.resize(piece, N64)
        d_plain, d_runs = torch.from_numpy(plain).to(_dev()), torch.from_numpy(runs).to(_dev())
        fp = shafa.compress_files(d_plain, BS8)
        fr = shafa.compress_files(d_runs, BS8, force_rle=True)
        assert ".shaf" in fp and ".rle.shaf" in fr
        _WIDE64["N"] = (plain, d_plain, dict(shaf=fp[".shaf"], cod=fp[".cod"]))
        _WIDE64["R"] = (runs, d_runs, dict(shaf=fr[".rle.shaf"], cod=fr[".rle.cod"]))
    return _WIDE64


def _one_wide_call(calls, nsym):
    """the index was built by ONE seek_index_dev call of more spans than the launch has waves; its last waves' second spans
    are real ones"""
    assert len(calls) == 1, len(calls)
    caps, span = [int(c) for c in calls[0][3]], calls[0][6]
    assert span == SPAN and len(caps) == len(nsym) and all(c >= n for c, n in zip(caps, nsym))
    base, real = 0, 0                                                 # spans are numbered from the capacities
    for c, n in zip(caps, nsym):
        real += max(0, base + -(-n // span) - max(base, SPAN_WAVES))
        base += -(-c // span)
    assert base > SPAN_WAVES and real >= 1000, (base, real)


@gpu
def test_seek_spans_grid_stride_mode_n(shafa, oracle, monkeypatch):
    plain, _, kw = _wide64(shafa)["N"]
    calls = _count_calls(shafa, monkeypatch, "seek_index_dev")
    idx = shafa.build_index(span=SPAN, max_bytes=1 << 32, **kw)
    parts = ts._blocks(plain, BS8)
    _one_wide_call(calls, [len(b) for b in parts])
    ts._check_index(idx, [(b, ts._lens(oracle.sf_build(oracle.hist256(b)))) for b in parts], SPAN, False)
    ts._check_reads(shafa, idx, plain, kw, ts._ranges(N64, 65536, SPAN, 11))


@gpu
def test_seek_spans_grid_stride_mode_r(shafa, oracle, monkeypatch):
    runs, _, kw = _wide64(shafa)["R"]
    calls = _count_calls(shafa, monkeypatch, "seek_index_dev")
    idx = shafa.build_index(span=SPAN, max_bytes=1 << 32, **kw)
    parts = ts._blocks(runs, BS8)
    rle_n = [len(oracle.rle_encode(b)) for b in parts]
    _one_wide_call(calls, rle_n)
    assert idx.decoded_size == N64 and [b.decoded_size for b in idx.blocks] == [len(b) for b in parts]
    assert [b.n_symbols for b in idx.blocks] == rle_n and all(b.indexed for b in idx.blocks)
    offs = idx.checkpoints.cpu().numpy()[1::2]
    assert offs.size == sum(-(-n // SPAN) for n in rle_n)
    for b, n in zip(idx.blocks, rle_n):
        o = offs[b.first_checkpoint:b.first_checkpoint + -(-n // SPAN)]
        assert o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] <= b.decoded_size, b
    ts._check_reads(shafa, idx, runs, kw, ts._ranges(N64, 65536, SPAN, 12))


# ================================================================ the 192 MiB of three full regions
TILES3 = (8193, 8191, 8192)
_BIG = []


def _big():
    """24576 tiles of random bytes, made once and never written, and its three regions"""
    if not _BIG:
        x = np.random.default_rng(192).integers(0, 256, sum(TILES3) * T, dtype=np.uint8)
        x.setflags(write=False)
        _BIG.append(x)
    cuts = [0] + list(np.cumsum(TILES3) * T)
    return _BIG[0], [_BIG[0][a:z] for a, z in zip(cuts, cuts[1:])]


def _two_tiles_a_workgroup(caps):
    """the call's tiles are numbered from the capacities: two to a workgroup, and one workgroup holds the last tile of
    region 0 and the first of region 1"""
    tiles = [-(-c // T) for c in caps]
    assert tuple(tiles) == TILES3
    per_wg = -(-sum(tiles) // TILE_WGS)
    assert per_wg == 2
    wg = (tiles[0] - 1) // per_wg
    assert (wg * per_wg, wg * per_wg + 1) == (tiles[0] - 1, tiles[0])


# ================================================================ 2. find
FIND_SIZES = (256 * T + 1, 512 * T, 512 * T + 1)
FIND_BORDERS = (1, 2, 3, 4, 5, 6, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512)
CHAIN5 = [1, 1, 1, 1, 0]


def _find_case(rot, m):
    """five regions cut from one stream: the three sizes at the alignments 0, 1 and 17 (rot: which size at which), two of
    100 bytes between; the pattern lies across tile borders of every region, across seams, and at the end of the last region
    -> (regions, pattern, the planted starts in the stream, the cuts)"""
    rng = tf._rng(500 + 10 * rot + m)
    pat = tf._rand(rng, m)
    order = [FIND_SIZES[(rot + k) % 3] for k in range(3)]
    sizes = [order[0], order[1], 100, 100, order[2]]
    assert [tf.ALIGN[i % 5] for i in (0, 1, 4)] == [0, 1, 17]
    cuts = [0] + [int(c) for c in np.cumsum(sizes)]
    whole = bytearray(tf._rand(rng, cuts[-1]))
    starts = []
    for a, n in zip(cuts, sizes):
        starts += [a + B * T - m // 2 for B in FIND_BORDERS if B * T - m // 2 + m <= n]
    starts += [c - m // 2 for c in (cuts[1:-1] if m <= 64 else cuts[1:3])]       # A | B; B | 100 | 100 (| C)
    starts.append(cuts[-1] - m)                                                  # ends with the last region
    for s in starts:
        whole[s:s + m] = pat
    return [bytes(whole[a:z]) for a, z in zip(cuts, cuts[1:])], pat, sorted(set(starts)), cuts


def _find_shapes():
    tiles = [-(-n // T) for n in FIND_SIZES]
    assert tiles == [257, 512, 513] and [_per(t) for t in tiles] == [2, 2, 3]
    # borders between two threads' runs (2 j and 3 j) and between two waves' (64 runs)
    assert {2, 4, 6, 128, 256, 512} <= set(FIND_BORDERS) and {3, 6, 129, 384} <= set(FIND_BORDERS)
    assert 64 * 2 * 2 in FIND_BORDERS and 64 * 3 * 2 in FIND_BORDERS and 64 * 2 * 2 < tiles[1] and 64 * 3 * 2 < tiles[2]


@gpu
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_find_regions_of_more_than_256_tiles(shafa, rot):
    _find_shapes()
    for m in (33, 256):
        regions, pat, starts, cuts = _find_case(rot, m)
        for flags in (None, CHAIN5):
            r = tf._Run(shafa, regions, flags, pat).check((m, flags))
            assert r.rc == 0 and not any(r.errs)
            found = {cuts[reg] + o for reg, o in r.hits}
            if flags:
                assert set(starts) <= found and cuts[1] - m // 2 in found              # the seam of the two large regions
            else:
                assert len(found) >= len(starts) - 4 and cuts[1] - m // 2 not in found
            tf._Run(shafa, regions, flags, pat, max_hits=len(r.want) // 2).check((m, flags, "max_hits below"))
    # the last stream again: a match in every tile, all reported, and half of them
    big = [i for i in range(5) if len(regions[i]) > T]
    for flags, max_hits in ((None, None), (CHAIN5, 300000)):
        r = tf._Run(shafa, regions, flags, b"ab", max_hits=max_hits).check(("ab", flags))
        assert r.total > 2 * 300000 and r.max_hits == (max_hits or r.total + 3)
        with_hit = {(reg, o // T) for reg, o in r.hits}
        for i in big:
            assert all((i, t) in with_hit for t in range(len(regions[i]) // T)), i


@gpu
def test_find_two_tiles_a_workgroup_on_full_regions(shafa):
    whole, regs = _big()
    pat = b"\x5a\xc3\x17"
    n0 = len(regs[0])
    _two_tiles_a_workgroup([len(r) for r in regs])
    x = whole.copy()
    at = np.unique(np.random.default_rng(5).integers(0, x.size - 3, 1000) // 8 * 8)
    for k in range(3):
        x[at + k] = pat[k]
    x[n0 - 3:n0] = list(pat)                                             # the last bytes of region 0's last tile
    x[n0:n0 + 3] = list(pat)                                             # the first bytes of region 1
    y = x.copy()
    y[n0 - 1:n0 + 2] = list(pat)                                         # across that seam
    cut = lambda v: [v[a:z].tobytes() for a, z in ((0, n0), (n0, n0 + len(regs[1])), (n0 + len(regs[1]), v.size))]
    r = tf._Run(shafa, cut(x), None, pat).check("x")
    assert [c == len(g) for c, g in zip(r.cap, regs)] == [True] * 3     # full: n = cap
    assert (0, n0 - 3) in r.hits and (1, 0) in r.hits and at.size > 990
    assert at.size + 2 < len(r.hits) < at.size + 40                     # the planted ones and a dozen of chance
    r = tf._Run(shafa, cut(y), None, pat).check("y")
    assert (0, n0 - 1) not in r.hits
    r = tf._Run(shafa, cut(y), [1, 1, 0], pat).check("y, chained")
    assert (0, n0 - 1) in r.hits


# ================================================================ 3. compare
CMP_SIZES = (257 * T + 5, 600 * T)
CMP_REF_N = 256 * T + 100


def _cmp_places(n):
    """what differs -> the offsets; tile j is read by thread j % 256 on its trip j // 256"""
    same = (44, 300) if n > 300 * T else (0, 256)
    two = (261, 200) if n > 261 * T else (256, 200)
    assert same[0] % THREADS == same[1] % THREADS and same[0] // THREADS == 0 and same[1] // THREADS == 1
    assert two[0] % THREADS < two[1] % THREADS and two[0] // THREADS == 1 and two[1] // THREADS == 0
    return {"none": (), "tile 256": (256 * T + 3,), "one thread's two trips": (same[1] * T + 9, same[0] * T + 7),
            "two threads": (two[0] * T + 1, two[1] * T + 8000), "the last byte": (n - 1,)}


def _cmp_blocks():
    blocks, labels, wants = [], [], []
    for n in CMP_SIZES:
        x = tc._data(700 + n % 97, n + 48)
        for al in (0, tc.REF_VIEW):
            for what, at in _cmp_places(n).items():
                blocks.append(tc._Blk(x[:n], tc._flip(x[:n], *at), al) if al else tc._Blk(tc._flip(x[:n], *at), x[:n], al))
                labels.append((n, al, what))
                wants.append(min(at) if at else n)
            # ref ends past 2 MiB, inside a; a differs from what follows ref just behind its end
            blocks.append(tc._Blk(tc._flip(x[:n], CMP_REF_N + 1), x[:CMP_REF_N], al, ref_tail=x[CMP_REF_N:CMP_REF_N + 40]))
            labels.append((n, al, "behind ref_n"))
            wants.append(CMP_REF_N)
    return blocks, labels, wants


@gpu
def test_compare_regions_of_more_than_256_tiles(shafa):
    assert CMP_REF_N > 256 * T and all(-(-n // T) > THREADS for n in CMP_SIZES)
    blocks, labels, wants = _cmp_blocks()
    assert [k.want() for k in blocks] == wants                          # numpy, and where the differences were put
    tc._check(shafa, blocks, labels)


@gpu
def test_compare_two_tiles_a_workgroup(shafa):
    regs = [np.minimum(r, 0xFD) for r in _big()[1]]                     # below the fill bytes
    _two_tiles_a_workgroup([len(r) for r in regs])
    n = [len(r) for r in regs]
    refs = [regs[0], tc._flip(regs[1], 5), tc._flip(regs[2], n[2] - 7)]  # region 1's first tile, region 2's last
    blocks = [tc._Blk(a, r, al) for a, r, al in zip(regs, refs, (0, 3, 9))]
    assert [k.want() for k in blocks] == [n[0], 5, n[2] - 7] and (n[2] - 7) // T == TILES3[2] - 1
    tc._check(shafa, blocks, ["equal", "first tile", "last tile"])
    blocks = [tc._Blk(a, a, al) for a, al in zip(regs, (0, 3, 9))]
    assert [k.want() for k in blocks] == n
    tc._check(shafa, blocks, ["equal"] * 3)


@gpu
@pytest.mark.parametrize("form", ["N", "R"])
def test_verify_files_differs_past_2_mib_of_a_block(shafa, form):
    data, d_in, kw = _wide64(shafa)[form]
    pos = BS8 + 256 * T + 1                                             # tile 256 of block 1: thread 0's second trip
    assert (pos - BS8) // T == THREADS and BS8 // T > THREADS and pos < 2 * BS8
    assert shafa.verify_files(d_in, decode_rle=form == "R", **kw) == shafa.Verify(True, None, N64)
    bad = _plant(d_in, pos)
    assert np.flatnonzero(bad.cpu().numpy() != data).tolist() == [pos]
    assert shafa.verify_files(bad, decode_rle=form == "R", **kw) == shafa.Verify(False, pos, N64)


# ================================================================ 4. CRC-32
CRC_LENGTHS = (513 * T, 600 * T + 1, 1024 * T)


def _crc_shapes():
    tiles = [-(-n // T) for n in CRC_LENGTHS]
    assert [_per(t) for t in tiles] == [3, 3, 4]
    assert [_per(t) * THREADS - t for t in tiles] == [255, 167, 0]                            # lead: records not there


@gpu
@pytest.mark.parametrize("kinds", [("random",), ("zeros", "ones")], ids=["random", "zeros-ones"])
def test_crc_regions_of_more_than_512_tiles(shafa, kinds):
    _crc_shapes()
    whole = _big()[0]
    blocks, labels = [], []
    for kind in kinds:
        for n in CRC_LENGTHS:
            for al in (0, 1, 7, 15) if kind == "random" else (0, 7):
                cap = n + (n + al) % 3 * 9                              # exact regions and regions with slack behind d_in_n
                at = (n + 7919 * al) % 100003
                blocks.append(tr._Blk(whole[at:at + cap] if kind == "random" else tr._content(kind, cap, 0), al, n=n, cap=cap))
                labels.append((kind, n, al))
    tr._check(shafa, blocks, labels)


@gpu
def test_crc_two_tiles_a_workgroup_and_the_combine(shafa):
    whole, regs = _big()
    _two_tiles_a_workgroup([len(r) for r in regs])
    blocks = [tr._Blk(r, al) for r, al in zip(regs, (0, 5, 15))]
    got = tr._check(shafa, blocks, list(range(3)))
    crc, n = tr._combine(shafa, got, [len(r) for r in regs], [0, 1], [3, 2])
    assert n == [whole.size, len(regs[1]) + len(regs[2])]
    assert crc == [zlib.crc32(whole), zlib.crc32(whole[len(regs[0]):])]


# ================================================================ the arithmetic alone
def test_the_wide_shapes_occur():
    """what needs no GPU of the assertions above: the runs of the blocks kernels, the hand-made .rle's checkpoints, the
    borders the patterns are planted across, the trips of compare_blocks, the pairs of the tiles kernels"""
    assert _runs(257)[127:130] == [2, 1, 0] and _runs(512) == [2] * THREADS and _runs(514)[170:173] == [3, 1, 0]
    assert _per(640) == 3 and _per(468) == 2 and _per(8192) == 32
    _hand_wide_shapes()
    _find_shapes()
    for n in CMP_SIZES:
        _cmp_places(n)
    blocks, labels, wants = _cmp_blocks()
    assert [k.want() for k in blocks] == wants and len(blocks) == 24
    _crc_shapes()
    _two_tiles_a_workgroup([t * T for t in TILES3])
    # mode N of the grid-stride set: 8 blocks of 32768 spans fill the launch's waves, the ninth block's spans come behind
    assert 8 * (BS8 // SPAN) == SPAN_WAVES and (N64 - 8 * BS8) // SPAN == 1024
    for m in (33, 256):
        regions, pat, starts, cuts = _find_case(1, m)
        whole = b"".join(regions)
        assert all(whole[s:s + m] == pat for s in starts) and len(starts) >= 40
        assert sorted(len(r) for r in regions if len(r) > T) == sorted(FIND_SIZES)

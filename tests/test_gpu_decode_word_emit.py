"""sfd_wstage<0, false, true> (sf_decode.hip, ws_walk1): the symbol pass of a launch whose codes all fit a 10-bit window, few of
them per window (sym1_pays: Zipf-like and uniform data), takes ONE symbol per look-up.  A lane gathers its symbols in words of its own frame, moves every finished word into the image's frame
with the word before it (by (4 - x & 3) & 3 bytes, x = the lane's first image byte) and stores it plainly; only the words at
both ends of its run, which it shares with its neighbours, are ORed.  What can go wrong is the placement: a lane phase x & 3,
a word stored plainly over a neighbour's bytes, a first or last piece of a shape that was not thought of, the two kept pieces
between rounds and tiles.  So the cases vary the output alignment, the symbols per chunk (code-length classes), and where a
stream ends; the classes with codes of 11 and 12 bits or of at most 4 bits keep the three-codes walk (sfd_wstage<0, false>) and
go through the same cases.  Every one compares the decoded bytes and the return code with the ORACLE's sf_decode of the same stream,
for sf_decode_speculate 1 and 2; the bytes around every block's output must stay untouched.

The launcher hands a workgroup 16 tiles (kept pieces between tiles, the prefetch) only when ceil(max_tiles / 16) * nblocks >=
2048: the launches here have NBLOCKS blocks, a few of 3 to 40 tiles among small ones (as in test_gpu_decode_counted_wait.py)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from test_gpu_parity import first_diff, to_shafa_table

pytestmark = pytest.mark.gpu

TILE = 8192                       # stream bytes per tile (DTILE)
TILE_BITS = TILE * 8
CHUNK_BITS = 256                  # stream bits per lane
NBLOCKS = 690                     # ceil(33 .. 40 / 16) * 690 = 2070 workgroups: 16 tiles per workgroup
MODES = (1, 2)


@pytest.fixture()
def spec(shafa):
    shafa.lib().shafa_hip_init(0)
    yield shafa
    shafa.set_option("sf_decode_speculate", 1)


# ---------------------------------------------------------------- tables (the host's Module T on chosen histograms) and data
def module_t(shafa, freq):
    """the host's Module T on a histogram -> the table in the oracle's type"""
    t = shafa.sf_build_codes(np.asarray(freq, dtype=np.uint64))
    o = oracle_lib.CodeTable()
    C.memmove(C.byref(o), C.byref(t), C.sizeof(o))
    return o


def dyadic_hist(lens):
    """{symbol: length} with Kraft sum 1 -> the histogram 2^(Lmax - length): Shannon-Fano's halvings are exact on it"""
    assert sum(Fraction(1, 1 << l) for l in lens.values()) == 1
    top = max(lens.values())
    f = np.zeros(256, dtype=np.uint64)
    for s, l in lens.items():
        f[s] = 1 << (top - l)
    return f


def chain_lens(k, deepest):
    """2^k - 1 symbols of k bits, one each of k + 1 .. deepest - 1 bits, two of `deepest` bits"""
    lens = {s: k for s in range((1 << k) - 1)}
    s = len(lens)
    for l in range(k + 1, deepest):
        lens[s] = l
        s += 1
    lens[s] = lens[s + 1] = deepest
    return lens


def draw(seed, n, symbols):
    return np.asarray(symbols, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(symbols), size=n)]


_classes = {}


def code_class(name, shafa, oracle):
    """name -> (table, source symbols, sf_decode_speculate modes), built once.
    lmax10: Zipf(1.2) mod 256, the headline's shape (three one-symbol look-ups per fetch).  lmax11, lmax12: only two such
    look-ups would fit a fetch: the three-codes walk; symbols drawn evenly, so that a long code comes every few dozen symbols.
    lmax4 (two whole codes per window: the three-codes walk as well): codes of 1 .. 4 bits in
    stretches of mostly 1-bit codes (up to 256 symbols per chunk, 65 536 per tile: more than the image, which is sized for
    the block's average, so several rounds with kept pieces) and stretches of 3- and 4-bit codes (64 to 85 per chunk).
    rounds: a 3-bit code among codes of 8 .. 10 bits (1.02 whole codes per window: a table the one-symbol walk takes), in
    stretches of all symbols (8 200 per tile, 13 tiles) and stretches of the 3-bit code alone (21 845 per tile, 4 tiles): the
    image is sized for the densest block's average, 12 000 per tile, so the dense tiles go in two rounds with kept pieces.
    uniform: uniform bytes, codes of 7 .. 9 bits, about 30 symbols per chunk (speculates only when told to: mode 2)."""
    if name in _classes:
        return _classes[name]
    if name == "lmax10":
        import golden.make_golden as mg
        src = oracle.gen_bytes(4243, 41 * 11000, mg.zipf_mod256_table(1.2))
        tab = module_t(shafa, oracle.hist256(src) + np.uint64(1))
        assert tab.lens().min() >= 1 and tab.lens().max() == 10
    elif name in ("lmax11", "lmax12"):
        lens = chain_lens(6, int(name[4:]))
        tab = module_t(shafa, dyadic_hist(lens))
        assert {s: int(tab.lens()[s]) for s in lens} == lens and tab.lens().sum() == sum(lens.values())
        src = draw(len(name) + 11, 41 * 11000, sorted(lens))
    elif name == "lmax4":
        lens = {7: 1, 9: 2, 200: 3, 201: 4, 255: 4}
        tab = module_t(shafa, dyadic_hist(lens))
        assert {s: int(tab.lens()[s]) for s in lens} == lens
        rng = np.random.default_rng(404)
        parts = []
        for i in range(28):
            if i % 2 == 0:
                p = np.full(150000, 7, dtype=np.uint8)
                p[rng.random(p.size) < 0.03] = 9
            else:
                p = draw(500 + i, 30000, (200, 201, 255))
            parts.append(p)
        src = np.concatenate(parts)
    elif name == "rounds":
        lens = {s: 8 for s in range(223)}
        lens.update({250: 3, 251: 9, 252: 10, 253: 10})
        tab = module_t(shafa, dyadic_hist(lens))
        assert {s: int(tab.lens()[s]) for s in lens} == lens
        parts = []
        for i in range(8):
            parts.append(draw(600 + i, 120000, sorted(lens)) if i % 2 == 0 else np.full(100000, 250, dtype=np.uint8))
        src = np.concatenate(parts)
    elif name == "uniform":
        src = oracle.gen_bytes(78, 43 * 8192, None)
        tab = module_t(shafa, oracle.hist256(src))
        assert tab.lens().min() >= 7 and tab.lens().max() <= 9
    else:
        raise KeyError(name)
    _classes[name] = (tab, src, (2,) if name == "uniform" else MODES)
    return _classes[name]


CLASSES = ("lmax10", "lmax11", "lmax12", "lmax4", "rounds", "uniform")


def starts_of(data, lens):
    """bit position at which each symbol's code starts, and the stream's length in bits"""
    ends = np.cumsum(lens[data].astype(np.int64))
    return ends - lens[data], int(ends[-1])


def cut_to_tiles(data, lens, tiles, last_bytes=TILE - 64):
    """the longest prefix of `data` whose stream has `tiles` tiles, the last one filled up to `last_bytes` bytes"""
    ends = np.cumsum(lens[data].astype(np.int64))
    n = int(np.searchsorted(ends, ((tiles - 1) * TILE + last_bytes) * 8, side="right"))
    assert 0 < n < data.size and ends[n - 1] > (tiles - 1) * TILE_BITS
    return data[:n]


def cut_behind(data, lens, bit, k):
    """the prefix of `data` that ends with the k-th symbol whose code starts at or behind stream bit `bit`"""
    st, _ = starts_of(data, lens)
    n = int(np.searchsorted(st, bit, side="left")) + k
    assert k <= n < data.size
    return data[:n]


# ---------------------------------------------------------------- one launch
_refs = {}


def reference(oracle, data, tab):
    """the oracle's stream of `data` and the oracle's own decode of that stream (what every comparison is made with), computed
    once per slice of a class's source (the classes keep their sources and tables alive, so addresses identify them)"""
    key = (data.__array_interface__["data"][0], data.size, id(tab))
    if key not in _refs:
        rc, e = oracle.sf_encode(data, tab)
        assert rc == 0
        rc, w = oracle.sf_decode(e, tab, data.size)
        assert rc == 0 and w.tobytes() == data.tobytes()
        e.setflags(write=False)
        w.setflags(write=False)
        _refs[key] = (e, w, data)
    return _refs[key][:2]


def run_launch(shafa, oracle, uniq, order, mode, shift=0):
    """uniq: (data, table); order: one index into uniq per block of the launch; shift: the output region starts `shift` bytes
    into its allocation (the C API wants every block's offset in the region to be a multiple of 16, so the region's start
    is what sets a block's address mod 16).
    Returns a list of problems (empty = every block equals the oracle's decode and nothing else was written)."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    enc, want = [], []
    for data, tab in uniq:
        e, w = reference(oracle, data, tab)
        enc.append(e)
        want.append(w)
    stabs = [to_shafa_table(shafa, u[1]) for u in uniq]
    off, pos, ooff, opos = [], 0, [], 32
    for k in order:
        off.append(pos)
        pos += (enc[k].size + 15) // 16 * 16
        ooff.append(opos)
        opos += (want[k].size + 15) // 16 * 16 + 48
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, k in zip(off, order):
        host[o:o + enc[k].size] = enc[k]
    d_in = torch.from_numpy(host).to(dev)
    d_all = torch.full((opos + 64 + shift,), 0xEE, dtype=torch.uint8, device=dev)
    d_out = d_all[shift:]
    bt = shafa.Batch(len(order), max(e.size for e in enc))
    torch.cuda.synchronize()
    shafa.set_option("sf_decode_speculate", mode)
    bt.sf_decode(st, d_in, off, [enc[k].size for k in order], [stabs[k] for k in order], [want[k].size for k in order],
                 d_out, ooff)
    rc, errs = bt.finish(st, len(order), raise_on_error=False)
    out = d_all.cpu().numpy()[shift:]
    bt.close()
    bad = []
    if not (d_all[:shift + ooff[0]].cpu().numpy() == 0xEE).all():
        bad.append(f"mode {mode}: wrote in front of the first block")
    for i, k in enumerate(order):
        n = want[k].size
        if errs[i]:
            bad.append(f"mode {mode} block {i} (kind {k}): error {errs[i]}, oracle 0")
            continue
        got = out[ooff[i]:ooff[i] + n]
        if got.tobytes() != want[k].tobytes():
            bad.append(f"mode {mode} block {i} (kind {k}, n={n}, out {ooff[i] + shift} mod 16 = {(ooff[i] + shift) % 16}): "
                       f"{first_diff(got, want[k])}")
        end = ooff[i] + n
        nxt = ooff[i + 1] if i + 1 < len(order) else end + 48
        if not (out[end:nxt] == 0xEE).all():
            bad.append(f"mode {mode} block {i} (kind {k}): wrote past its n_symbols")
    return bad


def launch_order(nbig, nsmall_kinds):
    """the large blocks (kinds 0 .. nbig - 1) spread among NBLOCKS - nbig small ones (the kinds behind them, in turn)"""
    order = [nbig + (i % nsmall_kinds) for i in range(NBLOCKS)]
    for b in range(nbig):
        order[7 + b * (NBLOCKS // nbig - 1)] = b
    assert sorted(set(order)) == list(range(nbig + nsmall_kinds))
    return order


SMALL = (1, 3, 15, 700, 2999)      # symbols of the small blocks


def big_and_small(tab, src, bigs):
    return [(b, tab) for b in bigs] + [(src[50:50 + n], tab) for n in SMALL]


# ---------------------------------------------------------------- output alignment
@pytest.mark.parametrize("shift", range(16))
@pytest.mark.parametrize("mode", MODES)
def test_output_alignment(oracle, spec, mode, shift):
    """Blocks of n, n + 1, n + 2, n + 3 and n + 13 symbols (3 to 4 tiles each), their outputs at every address mod 16: the
    output region starts at each of 16 consecutive byte addresses (block offsets inside it are multiples of 16, as the C
    API asks).  A 17-tile and a 33-tile block make the launcher hand out 16 tiles per workgroup, so the pieces kept between
    tiles occur too.  Every lane phase x & 3 with every first and last piece."""
    tab, src, _ = code_class("lmax10", spec, oracle)
    lens = tab.lens()
    n = cut_to_tiles(src, lens, 3, last_bytes=4000).size
    bigs = [src[7 * i:7 * i + n + (0, 1, 2, 3, 13)[i % 5]] for i in range(16)]
    bigs += [cut_to_tiles(src, lens, 17), cut_to_tiles(src[33:], lens, 33, last_bytes=3001)]
    uniq = big_and_small(tab, src, bigs)
    order = launch_order(len(bigs), len(SMALL))
    bad = run_launch(spec, oracle, uniq, order, mode, shift)
    assert not bad, "\n".join(bad[:12])


# ---------------------------------------------------------------- code-length classes and ends
def class_blocks(tab, src):
    """One class's blocks: 3, 16 + 1 and 40 tiles; exactly one tile; the stream ends 1, 2 and 3 symbols past a chunk boundary
    (in tile 3 of 4); inside the first chunk of a tile; the last tile has fewer than four symbols."""
    lens = tab.lens()
    bigs = [cut_to_tiles(src, lens, 3), cut_to_tiles(src[11:], lens, 17), cut_to_tiles(src[5:], lens, 40, last_bytes=2999)]
    one = cut_to_tiles(src[3:], lens, 1, last_bytes=TILE)
    _, bits = starts_of(one, lens)
    assert TILE_BITS - 16 < bits <= TILE_BITS
    bigs.append(one)
    edge = 3 * TILE_BITS + 77 * CHUNK_BITS
    bigs += [cut_behind(src[13:], lens, edge, k) for k in (1, 2, 3)]
    first_chunk = cut_behind(src[17:], lens, 4 * TILE_BITS, 2)
    st, bits = starts_of(first_chunk, lens)
    assert 4 * TILE_BITS < bits < 4 * TILE_BITS + CHUNK_BITS
    bigs.append(first_chunk)
    few = cut_behind(src[19:], lens, 5 * TILE_BITS, 3)
    st, bits = starts_of(few, lens)
    assert 1 <= int((st >= 5 * TILE_BITS).sum()) < 4
    bigs.append(few)
    return bigs


@pytest.mark.parametrize("name", CLASSES)
def test_code_length_classes_and_ends(oracle, spec, name):
    tab, src, modes = code_class(name, spec, oracle)
    assert tab.lens().max() <= 12                        # sfd_wstage<0, false> or <0, false, true>
    bigs = class_blocks(tab, src)
    uniq = big_and_small(tab, src, bigs)
    order = launch_order(len(bigs), len(SMALL))
    for mode in modes:
        bad = run_launch(spec, oracle, uniq, order, mode, shift=5 * mode)
        assert not bad, "\n".join(bad[:12])


def test_rounds_happen(oracle, spec):
    """the premise of the lmax4 class: some tiles hold more symbols than a 64 KiB LDS leaves for the image; of the rounds
    class: some tiles hold more than the 14.4 KiB that the 26.25 KiB step leaves, which the blocks' averages stay under"""
    tab, src, _ = code_class("lmax4", spec, oracle)
    st, bits = starts_of(src, tab.lens())
    per_tile = np.bincount(st // TILE_BITS)
    assert per_tile.max() > 56000 and per_tile.min() < 30000
    tab, src, _ = code_class("rounds", spec, oracle)
    for blk in class_blocks(tab, src):
        st, bits = starts_of(blk, tab.lens())
        assert blk.size / -(-bits // TILE_BITS) < 12500
    st, bits = starts_of(cut_to_tiles(src[5:], tab.lens(), 40, last_bytes=2999), tab.lens())
    assert np.bincount(st // TILE_BITS).max() > 21000


@pytest.mark.parametrize("mode", MODES)
def test_one_tile_per_workgroup(oracle, spec, mode):
    """690 blocks of at most one tile: a workgroup gets one tile and never runs the tile loop"""
    tab, src, _ = code_class("lmax10", spec, oracle)
    sizes = (1, 2, 3, 4, 5, 17, 255, 256, 257, 1000, 4099, 9000)
    uniq = [(src[3 * i:3 * i + n], tab) for i, n in enumerate(sizes)]
    order = [i % len(sizes) for i in range(NBLOCKS)]
    bad = run_launch(spec, oracle, uniq, order, mode, shift=7 * mode)
    assert not bad, "\n".join(bad[:12])


# ---------------------------------------------------------------- damage
@pytest.mark.parametrize("name", CLASSES)
def test_damaged_streams_equal_the_oracle(oracle, spec, name):
    """one truncated stream (with the announced count, and with the count that fits) and one with a flipped bit per class:
    the oracle's return code and, where that is success, the oracle's bytes"""
    tab, src, modes = code_class(name, spec, oracle)
    t = to_shafa_table(spec, tab)
    lens = tab.lens()
    data = cut_to_tiles(src[23:], lens, 5, last_bytes=1234)
    rc, enc = oracle.sf_encode(data, tab)
    assert rc == 0
    ends = np.cumsum(lens[data].astype(np.int64))
    cut = 3 * TILE + 1701
    fit = int(np.searchsorted(ends, cut * 8, side="right"))
    flipped = enc.copy()
    flipped[2 * TILE + 999] ^= np.uint8(0x10)
    cases = [("truncated", enc[:cut].copy(), data.size), ("truncated, the symbols that fit", enc[:cut].copy(), fit),
             ("flipped bit", flipped, data.size)]
    for mode in modes:
        spec.set_option("sf_decode_speculate", mode)
        for what, bad, nsym in cases:
            want_rc, want = oracle.sf_decode(bad, tab, nsym)
            got_rc, got = spec.sf_decode(bad, t, nsym, raw_rc=True)
            assert got_rc == want_rc, f"{name} mode {mode} {what}: rc {got_rc}, oracle {want_rc}"
            if want_rc == 0:
                assert got.tobytes() == want.tobytes(), f"{name} mode {mode} {what}: {first_diff(got, want)}"

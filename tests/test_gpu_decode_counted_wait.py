"""sfd_wstage's tile loop (sf_decode.hip): a workgroup decodes up to 16 tiles in a row, asks for the next tile's rows while it
decodes, and leaves the image stores of a tile in flight while it waits for those rows (a counted vmcnt).  A wrong count or a
missed wait shows as stale rows (wrong symbols from a workgroup's second tile on) or as image pieces that are lost or doubled,
so every case here runs the loop for real: the launcher hands out 16 tiles per workgroup only when
ceil(max_tiles / 16) * nblocks >= 2048, hence launches of NBLOCKS blocks of which a few are large and the rest are small.

Everything goes through the C ABI (Batch.sf_decode = shafa_hipd_sf_decode) and is compared with the ORACLE's decode of the
same stream, never with the library itself; the bytes around every block's output must stay untouched."""
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_parity import first_diff, to_shafa_table

pytestmark = pytest.mark.gpu

TILE = 8192                       # stream bytes per tile (DTILE)
TILE_BITS = TILE * 8
NBLOCKS = 690                     # ceil(33 / 16) * 690 = 2070 workgroups: 16 tiles per workgroup
BIG_TILES = (1, 2, 15, 16, 17, 33)
assert (max(BIG_TILES) + 15) // 16 * NBLOCKS >= 2048


@pytest.fixture()
def spec(shafa):
    shafa.lib().shafa_hip_init(0)
    yield shafa
    shafa.set_option("sf_decode_speculate", 1)


# ---------------------------------------------------------------- tables and data
def hand_table(oracle, lens):
    """{symbol: code length} (Kraft sum 1) -> the canonical code, written as a .cod block and parsed by the oracle."""
    assert sum(Fraction(1, 1 << l) for l in lens.values()) == 1
    fields, code, prev = [""] * 256, 0, None
    for l, s in sorted((l, s) for s, l in lens.items()):
        if prev is not None:
            code = (code + 1) << (l - prev)
        fields[s] = format(code, "0%db" % l)
        prev = l
    rc, t = oracle.cod_parse_block(";".join(fields).encode())
    assert rc == 0
    return t


def chain_lens(k, deepest):
    """2^k - 1 symbols of k bits, one each of k + 1 .. deepest - 1 bits, two of `deepest` bits: complete, and a uniform draw
    over the symbols meets a long code every few dozen symbols."""
    lens = {s: k for s in range((1 << k) - 1)}
    s = len(lens)
    for l in range(k + 1, deepest):
        lens[s] = l
        s += 1
    lens[s] = lens[s + 1] = deepest
    return lens


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


def with_residue(data, lens, tile, r):
    """`data` behind a few copies of the symbol with the shortest code (each adds a symbol in front of stream tile `tile` and
    pushes less than one out of it), so that the symbols whose codes start in front of that tile number r mod 16: the
    workgroup that starts at the tile then finds its first image piece misaligned by r bytes (block outputs are 16-byte
    aligned)"""
    used = np.nonzero(lens)[0]
    short = used[np.argmin(lens[used])]
    for j in range(96):
        d = np.concatenate([np.full(j, short, dtype=np.uint8), data])
        st, _ = starts_of(d, lens)
        if int(np.searchsorted(st, tile * TILE_BITS, side="left")) % 16 == r:
            return d
    raise AssertionError("no prefix gives the residue")


def draw(seed, n, symbols):
    return np.asarray(symbols, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(symbols), size=n)]


# ---------------------------------------------------------------- one launch
def run_launch(shafa, oracle, uniq, order, mode):
    """uniq: (data, table, padding bytes behind the stream); order: one index into uniq per block of the launch.
    Returns a list of problems (empty = every block equals the oracle's decode and nothing else was written)."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    enc, want = [], []
    for data, tab, pad in uniq:
        rc, e = oracle.sf_encode(data, tab)
        assert rc == 0
        e = np.concatenate([e, np.zeros(pad, dtype=np.uint8)])
        rc, w = oracle.sf_decode(e, tab, data.size)            # the reference for the comparison: the oracle's own decode
        assert rc == 0 and w.tobytes() == data.tobytes()
        enc.append(e)
        want.append(w)
    stabs = [to_shafa_table(shafa, u[1]) for u in uniq]
    off, pos, ooff, opos = [], 0, [], 16
    for k in order:
        off.append(pos)
        pos += (enc[k].size + 15) // 16 * 16
        ooff.append(opos)
        opos += (want[k].size + 15) // 16 * 16 + 48
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, k in zip(off, order):
        host[o:o + enc[k].size] = enc[k]
    d_in = torch.from_numpy(host).to(dev)
    d_out = torch.full((opos + 64,), 0xEE, dtype=torch.uint8, device=dev)
    bt = shafa.Batch(len(order), max(e.size for e in enc))
    torch.cuda.synchronize()
    shafa.set_option("sf_decode_speculate", mode)
    bt.sf_decode(st, d_in, off, [enc[k].size for k in order], [stabs[k] for k in order], [want[k].size for k in order],
                 d_out, ooff)
    rc, errs = bt.finish(st, len(order), raise_on_error=False)
    out = d_out.cpu().numpy()
    bt.close()
    bad = []
    if not (out[:16] == 0xEE).all():
        bad.append(f"mode {mode}: wrote in front of the first block")
    for i, k in enumerate(order):
        n = want[k].size
        if errs[i]:
            bad.append(f"mode {mode} block {i} (kind {k}): error {errs[i]}")
            continue
        got = out[ooff[i]:ooff[i] + n]
        if got.tobytes() != want[k].tobytes():
            bad.append(f"mode {mode} block {i} (kind {k}, n={n}): {first_diff(got, want[k])}")
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


def check_one_table(shafa, oracle, tab, source, mode, small=(700, 3000)):
    """blocks of 1, 2, 15, 16, 17 and 33 tiles of one table's stream in one launch, among small ones: the workgroups of one
    grid leave their loops after different numbers of tiles.  The 33-tile block ends inside a tile."""
    lens = tab.lens()
    uniq = [(cut_to_tiles(source, lens, t, last_bytes=2999 if t == 33 else TILE - 64), tab, 0) for t in BIG_TILES]
    uniq += [(source[100:100 + n], tab, 0) for n in small]
    bad = run_launch(shafa, oracle, uniq, launch_order(len(BIG_TILES), len(small)), mode)
    assert not bad, "\n".join(bad[:12])


# ---------------------------------------------------------------- the cases
def test_headline_table_alignments_padding_and_dense(oracle, spec):
    """Zipf(1.2) mod 256 with one table (codes of 3 .. 10 bits: one round per tile, 2 or 3 pieces per lane; sfd_wstage<0, false>):
    tiles per workgroup 1, 2, 15, 16, 16 + 1, 16 + 16 + 1; four 17-tile blocks whose second workgroup starts 0, 1, 8 and 15
    bytes into a 16-byte piece; a block that ends inside a tile; a block with 20 000 bytes of padding behind its last code
    (tot_c < total in the tile the symbols end in, whole tiles of padding behind it); a dense block (2-bit codes mostly:
    WS_NST pieces per lane and a second pass of the read-out); small blocks with 0 or 1 piece per lane."""
    import golden.make_golden as mg
    src = oracle.gen_bytes(4242, 34 * 11000 + 4096, mg.zipf_mod256_table(1.2))
    tab = oracle.sf_build(oracle.hist256(src) + np.uint64(1))
    lens = tab.lens()
    assert lens.min() >= 1 and lens.max() <= 12
    uniq = [(cut_to_tiles(src, lens, t), tab, 0) for t in (1, 2, 15, 16, 33)]
    for r in (0, 1, 8, 15):
        d = with_residue(cut_to_tiles(src[r * 37:], lens, 17), lens, 16, r)
        st, bits = starts_of(d, lens)
        assert np.searchsorted(st, 16 * TILE_BITS) % 16 == r and 16 * TILE_BITS < bits <= 17 * TILE_BITS
        uniq.append((d, tab, 0))
    uniq.append((cut_to_tiles(src, lens, 18, last_bytes=3001), tab, 0))               # ends inside a tile
    uniq.append((cut_to_tiles(src, lens, 3, last_bytes=5000), tab, 20000))            # padding: 2 more tiles and a bit
    rng = np.random.default_rng(9)
    dense = rng.integers(1, 6, size=900000, dtype=np.uint8)
    dense[rng.random(dense.size) < 0.6] = 0
    dtab = oracle.sf_build(oracle.hist256(dense))
    uniq.append((cut_to_tiles(dense, dtab.lens(), 17), dtab, 0))
    nbig = len(uniq)
    uniq += [(src[50:50 + n], tab, 0) for n in (1, 15, 700, 4000)]
    bad = run_launch(spec, oracle, uniq, launch_order(nbig, 4), 1)
    assert not bad, "\n".join(bad[:12])


def test_one_bit_codes_rounds(oracle, spec):
    """two symbols, 1-bit codes: 65 536 symbols per tile, more than the largest image holds — several rounds per tile, each
    round's read-out in several passes of WS_NST stores per lane, the last pass partly empty"""
    src = draw(11, 34 * 65536, (3, 203))
    tab = oracle.sf_build(oracle.hist256(src))
    assert sorted(tab.lens()[[3, 203]]) == [1, 1]
    check_one_table(spec, oracle, tab, src, 1, small=(5000, 60000))


def test_uniform_codes_speculating(oracle, spec):
    """uniform bytes (codes of 8 and 9 bits, a 7-bit one among them) with sf_decode_speculate = 2: the speculating kernels run and stand where their
    entries verify, the blocks take the exact kernels otherwise; the symbol pass is the same one behind both"""
    src = oracle.gen_bytes(77, 34 * 8192 + 4096)
    tab = oracle.sf_build(oracle.hist256(src))
    lens = tab.lens()
    assert lens.min() >= 7 and lens.max() <= 9
    check_one_table(spec, oracle, tab, src, 2)


@pytest.mark.parametrize("deepest", [13, 16, 32])
def test_long_code_classes(oracle, spec, deepest):
    """hand-made complete tables whose longest codes have 13 bits (sfd_wstage<0, true>), 16 bits (<1, true>) and 32 bits
    (<2, true>, with every length from 7 to 31 in between)"""
    lens = chain_lens(6, deepest)
    tab = hand_table(oracle, lens)
    assert tab.lens().max() == deepest
    src = draw(100 + deepest, 34 * 12000, sorted(lens))
    check_one_table(spec, oracle, tab, src, 1)

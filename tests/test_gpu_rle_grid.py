"""The RLE launchers cut their own grids (csrc/internal.hpp grid_slices): a call's blocks go to the device in
consecutive runs whose (rows of the largest block) x (blocks) stays within "rle_grid_rows", a block above it alone.  The
default limit is far above anything a quick test reaches, so the option is lowered here: every result — bytes, sizes,
histograms, error words — must equal the oracle's and the same call's at the default limit.  Inputs are runs_stream with a
stretch of zeros and a long run laid across the 8 KiB borders, so that both of the decoder's look-backs and the encoder's
carry cross tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 8192
MIX = [1, 3, 2, 0, 5, 1, 1, 4]          # tiles of 8 KiB per block; at limit 8: runs [0,2) [2,4) [4,5) [5,7) [7,8)
THIST = 32768


@pytest.fixture
def grid_rows(shafa):
    """set the limit; the default is back whatever the test does"""
    try:
        yield lambda v: shafa.set_option("rle_grid_rows", v)
    finally:
        shafa.set_option("rle_grid_rows", 0)


def _raw(seed, n):
    """runs_stream with zeros across the first 8 KiB border and a run of 600 across the second"""
    import golden.make_golden as mg
    a = mg.runs_stream(seed, n, mg.zipf_table(1.2)).copy()
    a[TILE - 300:TILE + 300] = 0
    a[2 * TILE - 100:2 * TILE + 500] = 7
    return a


def _token_ends(rle):
    """the positions behind every token of a well-formed RLE stream"""
    ends, i, n = [], 0, len(rle)
    while i < n:
        i += 3 if rle[i] == 0 else 1
        ends.append(i)
    assert ends[-1] == n
    return np.array(ends)


def _rle_input(oracle, seed, tiles):
    """an RLE stream of exactly `tiles` tiles of 8 KiB: the oracle's encoding of _raw, cut at token ends, with 40 triples of zeros
    (0 0 255: no two non-zero bytes in a row, so the tile behind them has to look back for its entry state) across the
    first 8 KiB border"""
    if not tiles:
        return np.zeros(0, dtype=np.uint8)
    rle = oracle.rle_encode(_raw(seed, 4 * tiles * TILE))
    ends = _token_ends(rle)
    want = tiles * TILE - 37
    if tiles == 1:
        out = rle[:ends[ends <= want][-1]]
    else:
        zeros = np.tile(np.array([0, 0, 255], dtype=np.uint8), 40)
        a = ends[ends <= TILE - 60][-1]
        z = ends[ends <= a + want - (a + zeros.size)][-1]
        out = np.concatenate([rle[:a], zeros, rle[a:z]])
    assert (out.size + TILE - 1) // TILE == tiles
    return out


@pytest.fixture(scope="module")
def dec_case(oracle):
    """the decoder's blocks and the oracle's (code, bytes) for each, computed once"""
    blocks = [_rle_input(oracle, 300 + i, t) for i, t in enumerate(MIX)]
    want = [oracle.rle_decode(b) for b in blocks]
    assert all(rc == 0 for rc, _ in want)
    return blocks, want


@pytest.fixture(scope="module")
def enc_case(oracle):
    """the encoder's blocks — 8192 k + 5 bytes, one of three 4 KiB tiles, one empty — and the oracle's RLE bytes"""
    sizes = [TILE * k + 5 for k in MIX] + [3 * 4096, 0]
    blocks = [_raw(400 + i, n) for i, n in enumerate(sizes)]
    return blocks, [oracle.rle_encode(b) if b.size else np.zeros(0, dtype=np.uint8) for b in blocks]


def _layout(sizes, pad=32):
    off, pos = [], 0
    for n in sizes:
        off.append(pos)
        pos += (n + 15) // 16 * 16 + pad
    return off, pos + 16


def _upload(blocks):
    import torch
    off, pos = _layout([b.size for b in blocks])
    host = np.zeros(pos, dtype=np.uint8)
    for o, b in zip(off, blocks):
        host[o:o + b.size] = b
    return torch.from_numpy(host).to("cuda:0"), off


def _decode(shafa, blocks, caps, dev, d_in_n=None):
    """one rle_decode (dev: rle_decode_dev, sizes d_in_n or the blocks' own) -> (the whole output buffer, sizes, error words)"""
    import torch
    st = torch.cuda.Stream(device="cuda:0")
    d_in, off = _upload(blocks)
    sizes = [b.size for b in blocks]
    ooff, opos = _layout(caps)
    d_out = torch.full((opos,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_n = torch.full((len(blocks),), -1, dtype=torch.int64, device="cuda:0")
    bt = shafa.Batch(len(blocks), max(max(sizes), max(caps), 16))
    try:
        torch.cuda.synchronize()
        if dev:
            d_sizes = torch.tensor(sizes if d_in_n is None else d_in_n, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            bt.rle_decode_dev(st, d_in, off, sizes, d_sizes, d_out, ooff, caps, d_n)
        else:
            bt.rle_decode(st, d_in, off, sizes, d_out, ooff, caps, d_n)
        _, errs = bt.finish(st, len(blocks), raise_on_error=False)
    finally:
        bt.close()
    return d_out.cpu().numpy(), ooff, [int(x) for x in d_n.cpu().numpy()], errs


def _check_decoded(got, want, skip=()):
    out, ooff, n, errs = got
    for b, (rc, w) in enumerate(want):
        if b in skip:
            continue
        assert errs[b] == rc and n[b] == w.size, (b, errs[b], n[b], w.size)
        assert out[ooff[b]:ooff[b] + w.size].tobytes() == w.tobytes(), f"block {b}"
        assert (out[ooff[b] + (w.size + 15) // 16 * 16:][:16] == 0xEE).all(), f"block {b} wrote past its bytes"


def _same(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("dev", [False, True], ids=["rle_decode", "rle_decode_dev"])
def test_decode_in_runs(shafa, dec_case, grid_rows, dev):
    blocks, want = dec_case
    caps = [w.size for _, w in want]
    default = _decode(shafa, blocks, caps, dev)
    grid_rows(8)
    cut = _decode(shafa, blocks, caps, dev)
    _check_decoded(cut, want)
    _same(cut, default)


def test_decode_dev_errors_in_a_later_run(shafa, oracle, dec_case, grid_rows):
    """block 5 (run 4 of 5) names more bytes than its capacity, block 7 (run 5) has too little room"""
    blocks, want = dec_case
    caps = [w.size for _, w in want]
    caps[7] = caps[7] // 2 // 16 * 16
    d_in_n = [b.size for b in blocks]
    d_in_n[5] += 1
    default = _decode(shafa, blocks, caps, True, d_in_n)
    grid_rows(8)
    cut = _decode(shafa, blocks, caps, True, d_in_n)
    _check_decoded(cut, want, skip=(5, 7))
    assert cut[3][5] == shafa.OUTSIDE_MODULE and cut[2][5] == 0
    assert cut[3][7] == oracle.rle_decode(blocks[7], cap=caps[7])[0] == shafa.LACK_OF_MEMORY
    _same(cut, default)


def _tile_hist(b):
    nt = (b.size + THIST - 1) // THIST
    return np.stack([np.bincount(b[t * THIST:(t + 1) * THIST], minlength=256) for t in range(nt)]).astype(np.uint16) \
        if nt else np.zeros((0, 256), dtype=np.uint16)


def _encode(shafa, blocks, tiles):
    """one rle_encode with d_freq (tiles: rle_encode_tiles) -> (output buffer, offsets, sizes, error words, histograms, tile
    histograms' buffer and offsets)"""
    import torch
    st = torch.cuda.Stream(device="cuda:0")
    d_in, off = _upload(blocks)
    sizes = [b.size for b in blocks]
    caps = [2 * n + 16 for n in sizes]
    ooff, opos = _layout(caps)
    toff, tpos = _layout([shafa.tile_hist_bytes(c) for c in caps])
    d_out = torch.full((opos,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_th = torch.full((tpos,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_n = torch.full((len(blocks),), -1, dtype=torch.int64, device="cuda:0")
    d_freq = torch.full((len(blocks) * 256,), -1, dtype=torch.int64, device="cuda:0")
    bt = shafa.Batch(len(blocks), max(caps))
    try:
        torch.cuda.synchronize()
        if tiles:
            bt.rle_encode_tiles(st, d_in, off, sizes, d_out, ooff, caps, d_n, d_freq, d_th, toff)
        else:
            bt.rle_encode(st, d_in, off, sizes, d_out, ooff, caps, d_n, d_freq)
        _, errs = bt.finish(st, len(blocks), raise_on_error=False)
    finally:
        bt.close()
    return (d_out.cpu().numpy(), ooff, [int(x) for x in d_n.cpu().numpy()], errs,
            d_freq.cpu().numpy().astype(np.uint64).reshape(len(blocks), 256), d_th.cpu().numpy(), toff)


def _check_encoded(oracle, got, want, tiles):
    out, ooff, n, errs, freq, th, toff = got
    assert errs == [0] * len(want)
    for b, w in enumerate(want):
        assert n[b] == w.size and out[ooff[b]:ooff[b] + w.size].tobytes() == w.tobytes(), f"block {b}"
        assert np.array_equal(freq[b], oracle.hist256(w) if w.size else np.zeros(256, dtype=np.uint64)), f"block {b}"
        if tiles:
            t = _tile_hist(w)
            assert np.array_equal(th[toff[b]:toff[b] + t.size * 2].view(np.uint16).reshape(t.shape), t), f"block {b}"


def _same_encoded(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and a[5].tobytes() == b[5].tobytes()


@pytest.mark.parametrize("tiles", [False, True], ids=["rle_encode", "rle_encode_tiles"])
def test_encode_in_runs(shafa, oracle, enc_case, grid_rows, tiles):
    """rows are pairs of 4 KiB tiles, k + 1 for 8192 k + 5 bytes: at limit 8 the ten blocks take six runs, the largest alone"""
    blocks, want = enc_case
    default = _encode(shafa, blocks, tiles)
    grid_rows(8)
    cut = _encode(shafa, blocks, tiles)
    _check_encoded(oracle, cut, want, tiles)
    _same_encoded(cut, default)


def test_every_block_its_own_run_and_one_block_calls(shafa, oracle, dec_case, enc_case, grid_rows):
    blocks, want = dec_case
    caps = [w.size for _, w in want]
    eblocks, ewant = enc_case
    for limit in (1, 8):
        grid_rows(limit)
        if limit == 1:
            for dev in (False, True):
                _check_decoded(_decode(shafa, blocks, caps, dev), want)
            _check_encoded(oracle, _encode(shafa, eblocks, True), ewant, True)
        for dev in (False, True):                   # the five-tile block alone: above the limit both times
            _check_decoded(_decode(shafa, blocks[4:5], caps[4:5], dev), want[4:5])
        _check_encoded(oracle, _encode(shafa, eblocks[4:5], True), ewant[4:5], True)


def test_drivers(shafa, grid_rows):
    """compress_many -> decompress_many with forced RLE over blocks of 16 KiB (two rows each for the encoder): at limit 8 every
    chain of the drivers takes several runs; the file sets and the decoded bytes are the default limit's"""
    import golden.make_golden as mg
    import torch
    zt = mg.zipf_table(1.2)
    files = [mg.runs_stream(500 + i, n, zt) for i, n in enumerate([40000, 1500, 70001, 24576 + 3, 9000])]
    d_in = [torch.from_numpy(f).to("cuda:0") for f in files]

    def round_trip():
        sets = shafa.compress_many(d_in, block_size=16384, force_rle=True)
        assert all(isinstance(s, dict) and ".rle.shaf" in s for s in sets)
        back = shafa.decompress_many([{"shaf": s[".rle.shaf"], "cod": s[".rle.cod"]} for s in sets] +
                                     [{"rle": s[".rle"], "freq": s[".rle.freq"]} for s in sets])
        return ([{k: v.cpu().numpy().tobytes() for k, v in s.items()} for s in sets],
                [t.cpu().numpy().tobytes() for t in back])

    default = round_trip()
    grid_rows(8)
    cut = round_trip()
    assert cut[0] == default[0] and cut[1] == default[1]
    assert cut[1] == [f.tobytes() for f in files] * 2


def test_option(shafa, grid_rows):
    with pytest.raises(shafa.ShafaError) as e:
        grid_rows(-1)
    assert e.value.code == shafa.OUTSIDE_MODULE
    grid_rows(5)
    grid_rows(0)
    assert shafa.lib().shafa_hip_set_option(b"rle_grid_rows", 0) == shafa.SUCCESS

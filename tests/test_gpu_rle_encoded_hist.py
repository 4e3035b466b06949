"""The RLE histogram pass (shafa_hipd_rle_encoded_hist_dev, csrc/rle_encode_hist.hip): d_freq equals np.bincount of the
oracle's RLE bytes and d_out_n their number, block by block.

1. run shapes (lengths around the literal / triple rule and around 255 and 510; the symbols whose counts coincide) at every
   position against a lane, a wave and a tile border; runs over whole tiles; blocks of one run; block sizes around a lane and
   a tile; a last lane of 1 .. 31 bytes with its last byte repeated behind the block;
2. a launch of 19 ragged blocks; one 8 MiB block among 3 000 blocks of 1 KiB;
3. a block past its capacity fails alone; d_freq filled with garbage is overwritten (every test pre-fills it);
4. the call only enqueues;
5. every golden session's input at its session's block size;
6. one block of 64 MiB against rle_encode_tiles' d_freq;
7. fuzz: 300 blocks against the oracle and against rle_encode's d_freq."""
import numpy as np
import pytest

from test_gpu_pack import F_CASES
from test_gpu_rle_encoded_size import _session_blocks
from test_gpu_rle_measure import SENT, TILE, _al16, _Blocks, _run_heavy
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

M64 = 64 << 20


def _hist(shafa, blk, bt=None, st=None):
    """one pass over blk, d_out_n and d_freq pre-filled with garbage -> (sizes, counts nb x 256, codes)"""
    import torch
    nb = len(blk.n)
    own = bt is None
    bt = bt or shafa.Batch(nb, 1 << 20)
    st = st or torch.cuda.Stream(device=_dev())
    try:
        d_size = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        d_freq = torch.full((nb * 256,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_encoded_hist_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size, d_freq)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        return d_size.cpu().numpy().view(np.uint64).tolist(), d_freq.cpu().numpy().view(np.uint64).reshape(nb, 256), errs
    finally:
        if own:
            bt.close()


def _want(oracle, blocks):
    enc = [oracle.rle_encode(b) for b in blocks]
    return [len(e) for e in enc], np.stack([np.bincount(e, minlength=256).astype(np.uint64) for e in enc])


def _check(oracle, shafa, blocks, caps=None, what=""):
    want_n, want_f = _want(oracle, blocks)
    got_n, got_f, rc = _hist(shafa, _Blocks(blocks, caps))
    assert not any(rc), (what, rc[:10])
    bad = [i for i in range(len(blocks)) if got_n[i] != want_n[i] or not (got_f[i] == want_f[i]).all()]
    assert not bad, f"{what}: blocks {bad[:10]}; first: {blocks[bad[0]].size} bytes, size {got_n[bad[0]]} for {want_n[bad[0]]}, " \
                    f"bins {np.flatnonzero(got_f[bad[0]] != want_f[bad[0]])[:8].tolist()}"
    assert all(int(got_f[i].sum()) == got_n[i] for i in range(len(blocks)))


# ---------------------------------------------------------------- 1. shapes and positions
SHAPES = [(65, L) for L in (1, 3, 4, 5, 254, 255, 256, 258, 259, 510, 511)] + \
         [(0, 7), (1, 7), (7, 7), (255, 255), (255, 256), (0, 255), (0, 1), (0, 3), (0, 256)]


def _noise(rng, n, avoid):
    x = rng.integers(1, 255, n, dtype=np.uint8)                        # no zeros, no 255
    x[x == avoid] = 254 if avoid != 254 else 253
    return x


def test_run_shapes_at_every_border(oracle, shafa):
    rng = np.random.default_rng(1)
    blocks = []
    for s, L in SHAPES:
        for border in (32, 2048, TILE):
            for before in (0, 1, 2, 3):
                blocks.append(np.concatenate([_noise(rng, border - before, s), np.full(L, s, dtype=np.uint8),
                                              _noise(rng, int(rng.integers(1, 90)), s)]))
                blocks.append(np.concatenate([_noise(rng, border - before, s), np.full(L, s, dtype=np.uint8)]))   # ends the block
    # isolated zeros between literals, and zeros next to runs
    x = _noise(rng, 3 * TILE + 5, 0)
    x[rng.integers(0, x.size, 2000)] = 0
    blocks.append(x)
    blocks.append(np.tile(np.array([0, 1], dtype=np.uint8), TILE))
    blocks.append(np.concatenate([_noise(rng, 777, 9), np.full(5 * TILE + 50, 9, dtype=np.uint8), _noise(rng, 333, 9)]))
    blocks.append(np.concatenate([_noise(rng, 777, 0), np.zeros(5 * TILE + 50, dtype=np.uint8), _noise(rng, 333, 0)]))
    for n in (0, 1, 31, 32, 33, 255, 2048, TILE - 1, TILE, TILE + 1, 3 * TILE, 255 * 70):
        blocks.append(np.full(n, 200, dtype=np.uint8))                 # a block that is one run
        blocks.append(np.zeros(n, dtype=np.uint8))                     # ... of zeros
        blocks.append(np.full(n, 255, dtype=np.uint8))
        blocks.append(_noise(rng, n, 0))
        blocks.append(rng.integers(0, 3, n, dtype=np.uint8))
    assert {0, 1, 31, 32, 33, 8191, 8192, 8193} <= {b.size for b in blocks}
    _check(oracle, shafa, blocks, what="shapes")


def test_a_last_lane_does_not_run_on_behind_the_block(oracle, shafa):
    """_Blocks fills the room behind a block with 0xEE: blocks that end in 0xEE inside a lane must stop there"""
    rng = np.random.default_rng(2)
    blocks = []
    for tail in range(1, 32):
        for base in (0, 64, TILE, TILE + 2048):
            x = rng.integers(0, 4, base + tail, dtype=np.uint8)
            x[-min(tail, 1 + tail % 6):] = 0xEE
            blocks.append(x)
    _check(oracle, shafa, blocks, caps=[b.size + 64 for b in blocks], what="tails")


# ---------------------------------------------------------------- 2. whole calls
def test_nineteen_ragged_blocks(oracle, shafa):
    rng = np.random.default_rng(3)
    blocks = []
    for i in range(19):
        n = int(rng.integers(0, 5 * TILE))
        blocks.append(_run_heavy(i, n, run=int(rng.choice([1, 3, 5, 40, 300, 3000]))) if i % 4 else rng.integers(0, 256, n, dtype=np.uint8))
    _check(oracle, shafa, blocks, caps=[b.size + int(rng.integers(0, 3 * TILE)) for b in blocks], what="ragged")


def test_one_large_block_among_thousands_of_small_ones(oracle, shafa):
    rng = np.random.default_rng(4)
    big = _run_heavy(11, 8 << 20, run=300)
    big[5 * TILE:9 * TILE + 77] = 0
    big[100 * TILE - 3:100 * TILE + 600] = 255
    small = [_run_heavy(1000 + i, 1024, run=40) if i % 3 == 0 else rng.integers(0, 256, 1024, dtype=np.uint8) for i in range(3000)]
    _check(oracle, shafa, small[:1400] + [big] + small[1400:], what="mix")


# ---------------------------------------------------------------- 3. capacities
def test_a_block_past_its_capacity_fails_alone(oracle, shafa):
    import torch
    blocks = [np.frombuffer(bytes([65, 65, 65, 65, 66, 0] * 700), dtype=np.uint8), np.full(9000, 3, dtype=np.uint8),
              np.frombuffer(bytes([0, 5, 5, 0, 0, 200] * 2000), dtype=np.uint8), np.zeros(0, dtype=np.uint8)]
    want_n, want_f = _want(oracle, blocks)
    blk = _Blocks(blocks)
    blk.d_n[1] = blk.cap[1] + 1
    before = blk.d_in.clone()
    got_n, got_f, errs = _hist(shafa, blk)
    assert errs == [0, shafa.OUTSIDE_MODULE, 0, 0], errs
    assert got_n == [want_n[0], 0, want_n[2], 0]
    assert (got_f[0] == want_f[0]).all() and (got_f[2] == want_f[2]).all()
    assert not got_f[1].any() and not got_f[3].any()
    assert torch.equal(blk.d_in, before)


# ---------------------------------------------------------------- 4. enqueue only
def test_the_call_only_enqueues(oracle, shafa):
    import torch
    rng = np.random.default_rng(5)
    blocks = [rng.integers(0, 4, 70000, dtype=np.uint8) for _ in range(6)]
    want_n, want_f = _want(oracle, blocks)
    blk = _Blocks(blocks)
    nb = len(blocks)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        d_size = torch.zeros(nb, dtype=torch.int64, device=_dev())
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=_dev())
        bt.rle_encoded_hist_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size, d_freq)     # warm-up: the batch grows here
        bt.finish(st, nb)
        assert d_size.cpu().tolist() == want_n
        d_size.zero_()
        d_freq.fill_(77)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)
        bt.rle_encoded_hist_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size, d_freq)
        busy = not st.query()
        bt.finish(st, nb)
        assert busy, "the stream had drained when the call returned: something synchronised"
        assert d_size.cpu().tolist() == want_n
        assert (d_freq.cpu().numpy().view(np.uint64).reshape(nb, 256) == want_f).all()
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. golden sessions
@pytest.mark.parametrize("case", F_CASES)
def test_golden_inputs_at_their_block_sizes(oracle, shafa, case):
    blocks, _, S = _session_blocks(shafa, case)
    try:
        _check(oracle, shafa, blocks, what=case)
    finally:
        if S is not None:
            S.close()


# ---------------------------------------------------------------- 6. a 64 MiB block
def test_a_64_mib_block_equals_the_encoders_histogram(shafa):
    import torch
    x = _run_heavy(21, M64, run=7)
    x[3 * TILE + 5:40 * TILE + 9] = 0                                  # a zero run over many tiles
    x[M64 - 70000:] = 255                                              # the block ends in a long run of 255
    x[M64 // 2:M64 // 2 + (1 << 20)] = np.random.default_rng(6).integers(0, 256, 1 << 20, dtype=np.uint8)
    blk = _Blocks([x])
    bt = shafa.Batch(1, 2 * M64 + 64)
    st = torch.cuda.Stream(device=_dev())
    try:
        got_n, got_f, rc = _hist(shafa, blk, bt, st)
        cap = 2 * M64 + 3
        d_out = torch.empty(_al16(cap) + 16, dtype=torch.uint8, device=_dev())
        d_th = torch.empty(shafa.tile_hist_bytes(cap) + 16, dtype=torch.uint8, device=_dev())
        d_n = torch.zeros(1, dtype=torch.int64, device=_dev())
        d_f = torch.zeros(256, dtype=torch.int64, device=_dev())
        bt.rle_encode_tiles(st, blk.d_in, blk.off, blk.n, d_out, [0], [cap], d_n, d_f, d_th, [0])
        bt.finish(st, 1)
        assert rc == [0] and got_n == d_n.cpu().tolist()
        assert (got_f[0] == d_f.cpu().numpy().view(np.uint64)).all()
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. fuzz
def fuzz_blocks(seed=20261017, count=300):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 40001))
        lens = [[1], [1, 1, 2, 3], [1, 2, 3, 4, 5, 6], [1, 3, 4, 254, 255, 256, 509, 510, 511], [30, 31, 32, 33, 64, 100],
                [1, 2, 2000, 2048, 9000], [max(n, 1)]][i % 7]
        alphabet = [np.arange(256), np.array([0, 1, 255]), np.array([0, 7]), np.arange(1, 256)][i % 4]
        L = rng.choice(lens, n // min(lens) + 1)
        L = L[:int(np.searchsorted(np.cumsum(L), n)) + 1]              # the runs that reach n bytes
        x = np.repeat(rng.choice(alphabet, L.size).astype(np.uint8), L)[:n]
        out.append(np.ascontiguousarray(x))
    return out


def test_fuzz_equals_the_oracle_and_the_encoder(oracle, shafa):
    import torch
    blocks = fuzz_blocks()
    want_n, want_f = _want(oracle, blocks)
    blk = _Blocks(blocks)
    nb = len(blocks)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        got_n, got_f, rc = _hist(shafa, blk, bt, st)
        bad = [(i, blocks[i].size, got_n[i], rc[i], want_n[i]) for i in range(nb)
               if (got_n[i], rc[i]) != (want_n[i], 0) or not (got_f[i] == want_f[i]).all()]
        assert not bad, f"(block, bytes, size, code, the oracle's size): {bad[:10]}"
        room = [2 * n + 3 for n in blk.n]
        ooff, pos = [], 0
        for r in room:
            ooff.append(pos)
            pos += _al16(r) + 16
        d_out = torch.empty(pos + 16, dtype=torch.uint8, device=_dev())
        d_enc_n = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        d_enc_f = torch.zeros(nb * 256, dtype=torch.int64, device=_dev())
        bt.rle_encode(st, blk.d_in, blk.off, blk.n, d_out, ooff, room, d_enc_n, d_enc_f)
        _, enc_rc = bt.finish(st, nb, raise_on_error=False)
        assert not any(enc_rc)
        assert d_enc_n.cpu().tolist() == got_n
        assert (d_enc_f.cpu().numpy().view(np.uint64).reshape(nb, 256) == got_f).all()
    finally:
        bt.close()

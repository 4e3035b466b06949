"""The Shannon-Fano size entry (shafa_hipd_sf_encoded_size_dev, csrc/sf_encoded_size.hip): per block
ceil(sum freq[s] * len[s] / 8) under binary_coding's rules.

1. histograms of the golden inputs and of the RLE pass's fuzz blocks with sf_build_codes' tables: the size equals
   sf_encode_dev's d_out_n for the same block and the oracle's;
2. hand-made tables with codes of 1, 16, 33 and 255 bits; the all-empty table; a block of one symbol; a counted symbol without a
   code fails alone; a bit sum past 64 bits is refused."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_pack import F_CASES
from test_gpu_rle_encoded_hist import fuzz_blocks
from test_gpu_rle_encoded_size import _session_blocks
from test_gpu_rle_measure import SENT, _al16, _Blocks
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu


def _sizes(shafa, freq, tables=None):
    """freq: nb x 256 counts; tables: CodeTables, or None = sf_build_codes on the device -> (sizes, codes, d_tables)"""
    import torch
    freq = np.ascontiguousarray(np.asarray(freq, dtype=np.uint64).reshape(-1, 256))
    nb = freq.shape[0]
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        d_freq = torch.from_numpy(freq.view(np.int64).reshape(-1)).to(_dev())
        if tables is None:
            d_tab = torch.empty(nb * C.sizeof(shafa.CodeTable), dtype=torch.uint8, device=_dev())
            bt.sf_build_codes(st, nb, d_freq, d_tab)
        else:
            d_tab = torch.from_numpy(np.frombuffer(b"".join(bytes(t) for t in tables), dtype=np.uint8).copy()).to(_dev())
        words = torch.full((nb + 8,), SENT, dtype=torch.int64, device=_dev())
        bt.sf_encoded_size_dev(st, nb, d_freq, d_tab, words[4:4 + nb])
        _, errs = bt.finish(st, nb, raise_on_error=False)
        w = words.cpu().tolist()
        assert w[:4] == [SENT] * 4 and w[4 + nb:] == [SENT] * 4
        return w[4:4 + nb], errs, d_tab
    finally:
        bt.close()


def _encoder_sizes(shafa, blocks, d_tab):
    """sf_encode_dev's d_out_n for these blocks with these device tables"""
    import torch
    blk = _Blocks(blocks)
    nb = len(blocks)
    ocap = [n + n // 2 + 64 for n in blk.n]
    ooff, pos = [], 0
    for c in ocap:
        ooff.append(pos)
        pos += _al16(c) + 16
    bt = shafa.Batch(nb, 2 * max(blk.n) + 64)
    st = torch.cuda.Stream(device=_dev())
    try:
        d_out = torch.empty(pos + 16, dtype=torch.uint8, device=_dev())
        d_n = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        bt.sf_encode_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_tab, d_out, ooff, ocap, d_n)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        return d_n.cpu().tolist(), errs
    finally:
        bt.close()


def _oracle_sizes(oracle, blocks):
    """orc_sf_encode's size with the oracle's own table: by encoding, and for blocks over 256 KiB (the oracle writes bit by
    bit) by its size rule, bits = the sum of the code lengths of the block's bytes"""
    out = []
    for b in blocks:
        freq = oracle.hist256(b)
        tab = oracle.sf_build(freq)
        if b.size <= 1 << 18:
            rc, enc = oracle.sf_encode(b, tab)
            assert rc == 0
            out.append(len(enc))
        else:
            lens = tab.lens().astype(np.uint64)
            assert not ((lens == 0) & (freq > 0)).any() or not lens.any()
            out.append((int((freq.astype(np.uint64) * lens).sum()) + 7) // 8)
    return out


def _compare(oracle, shafa, blocks, what):
    freq = np.stack([np.bincount(b, minlength=256) for b in blocks])
    got, rc, d_tab = _sizes(shafa, freq)
    assert not any(rc), (what, rc[:10])
    enc, enc_rc = _encoder_sizes(shafa, blocks, d_tab)
    assert not any(enc_rc) and got == enc, (what, [(i, g, e) for i, (g, e) in enumerate(zip(got, enc)) if g != e][:8])
    assert got == _oracle_sizes(oracle, blocks), what


# ---------------------------------------------------------------- 1. real histograms
def test_fuzz_blocks_equal_the_encoder_and_the_oracle(oracle, shafa):
    _compare(oracle, shafa, fuzz_blocks(), "fuzz")


@pytest.mark.parametrize("case", F_CASES)
def test_golden_inputs_equal_the_encoder_and_the_oracle(oracle, shafa, case):
    blocks, _, S = _session_blocks(shafa, case)
    try:
        _compare(oracle, shafa, blocks, case)
    finally:
        if S is not None:
            S.close()


# ---------------------------------------------------------------- 2. hand-made tables
def _table(shafa, lens):
    """a prefix-free shape is not needed for a size: symbol s gets a code of lens[s] bits"""
    return shafa.CodeTable.from_strings([("10" * 128)[:int(n)] for n in lens])


def test_hand_made_tables(shafa):
    rng = np.random.default_rng(7)
    lens = np.zeros((8, 256), dtype=np.int64)
    freq = np.zeros((8, 256), dtype=np.uint64)
    lens[0, :] = 1
    freq[0] = rng.integers(0, 1000, 256)
    lens[1, :] = 16
    freq[1] = rng.integers(0, 1 << 40, 256)
    lens[2, :] = rng.choice([1, 16, 33, 255], 256)
    freq[2] = rng.integers(0, 1 << 20, 256)
    lens[3, 5], lens[3, 200] = 255, 33                                 # two codes, the other symbols have no count
    freq[3, 5], freq[3, 200] = 3, 1
    # block 4: the all-empty table, counts everywhere; block 5: one symbol, no code (what sf_build_codes leaves for it)
    freq[4] = 9
    freq[5, 77] = 65536
    lens[6, :] = 255                                                   # 255 x 2^57 x 256 bits: past 64 bits
    freq[6] = 1 << 57
    lens[7, :] = 8                                                     # the largest sum that fits: 2^64 - 8 bits
    freq[7, 0] = (1 << 61) - 1
    got, rc, _ = _sizes(shafa, freq, [_table(shafa, l) for l in lens])
    want = [(sum(int(f) * int(n) for f, n in zip(freq[b], lens[b])) + 7) // 8 for b in range(8)]
    assert want[6] >= 1 << 61 and want[7] == (1 << 61) - 1
    want[4] = want[5] = want[6] = 0
    assert rc == [0, 0, 0, 0, 0, 0, shafa.OUTSIDE_MODULE, 0], rc
    assert [g & (2 ** 64 - 1) for g in got] == want, (got, want)


def test_a_counted_symbol_without_a_code_fails_alone(shafa):
    rng = np.random.default_rng(8)
    lens = np.full((5, 256), 9, dtype=np.int64)
    freq = rng.integers(1, 5000, (5, 256)).astype(np.uint64)
    lens[1, 40] = 0                                                    # counted, no code
    lens[3, 41] = 0                                                    # no code, but no count either
    freq[3, 41] = 0
    got, rc, _ = _sizes(shafa, freq, [_table(shafa, l) for l in lens])
    want = [(int((freq[b] * lens[b].astype(np.uint64)).sum()) + 7) // 8 for b in range(5)]
    want[1] = 0
    assert rc == [0, shafa.FILE_UNRECOGNIZABLE, 0, 0, 0], rc
    assert got == want


def test_a_block_of_one_symbol_is_size_zero(oracle, shafa):
    blocks = [np.full(5000, 3, dtype=np.uint8), np.arange(5000, dtype=np.uint8), np.zeros(1, dtype=np.uint8)]
    freq = np.stack([np.bincount(b, minlength=256) for b in blocks])
    got, rc, _ = _sizes(shafa, freq)
    assert not any(rc) and got[0] == 0 and got[2] == 0 and got[1] > 0
    assert got == _oracle_sizes(oracle, blocks)

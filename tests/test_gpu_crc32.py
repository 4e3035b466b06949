"""CRC-32 on the device (shafa_hipd_crc32_dev, shafa_hipd_crc32_combine_dev, csrc/crc32.hip) through the C-ABI, against
zlib.crc32 on host copies, and shafa.crc32.

Every block's bytes lie at their own alignment (0..15) inside a view, at storage offset 3, of one tensor whose other bytes —
in front of every region, the slack behind d_in_n up to the capacity, and the gaps — are 0xA5.  Every test is one call with
many blocks (a block's answer is its own); after every call d_crc[-1], d_crc[nblocks] and the buffer are what they were.

1. every length (0, 1, 15 .. 33, around one tile, 3 tiles + 5, 256 tiles + 1) at alignments 0, 1, 7, 15 (3 tiles + 5 at all
   sixteen), with random bytes, zeros (the raw remainder is 0: only the length speaks), 0xFF, and the "123456789" vector;
2. flipping every byte outside the regions between two calls changes no CRC;
3. d_in_n > h_in_cap: OUTSIDE_MODULE and CRC 0 for that block, its neighbours as without it;
4. the combine: files of 1, 2 and 300 blocks with empty blocks at the start, middle and end, h_count = 0, files that share no
   block, fabricated lengths of 2^33 + 5 against shafa.crc32_combine, a second call over the first call's outputs;
5. shafa.crc32: whole tensors, segments at odd offsets, empty segments, a segment cut into pieces."""
import zlib

import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

TILE = 8192
BIG = 3 * TILE + 5
WIDE = 256 * TILE + 1               # every thread of the blocks kernel composes two records; the last tile holds one byte
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, TILE - 1, TILE, TILE + 1, BIG, WIDE]
VIEW = 3                            # storage offset of the view handed over as d_in
FILL = 0xA5
CANARY = 0x5A5A5A5A


def _aligns(n):
    return range(16) if n == BIG else (0, 1, 7, 15)


_RANDOM = np.random.default_rng(2024).integers(0, 256, WIDE + 128, dtype=np.uint8)


def _content(kind, n, salt):
    if kind == "random":
        return _RANDOM[salt % 61:salt % 61 + n]
    return np.full(n, 0 if kind == "zeros" else 0xFF, dtype=np.uint8)


class _Blk:
    """one block: `data` at address `align` mod 16, d_in_n = n (default: all of it), capacity cap (default: n)"""

    def __init__(self, data, align=0, n=None, cap=None):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.align = align
        self.n = len(self.data) if n is None else n
        self.cap = self.n if cap is None else cap

    def want(self):
        return zlib.crc32(self.data[:self.n].tobytes()) if self.n <= self.cap else 0


def _layout(blocks):
    off, pos = [], 64
    for k in blocks:
        pos += (k.align - (VIEW + pos)) % 16
        off.append(pos)
        pos += max(len(k.data), k.cap) + 40
    return off, VIEW + pos + 64


def _run(shafa, blocks, flip_outside=False):
    """one crc32_dev call over these blocks -> (the CRCs, the per-block codes); asserts the canaries.  flip_outside: every
    byte that belongs to no block's first d_in_n bytes is complemented first"""
    import torch
    nb = len(blocks)
    off, total = _layout(blocks)
    host = np.full(total, FILL, dtype=np.uint8)
    inside = np.zeros(total, dtype=bool)
    for o, k in zip(off, blocks):
        host[VIEW + o:VIEW + o + len(k.data)] = k.data
        if k.n <= k.cap:
            inside[VIEW + o:VIEW + o + k.n] = True
    if flip_outside:
        host[~inside] ^= 0xFF
    d_buf = torch.from_numpy(host).to(_dev())
    d_in = d_buf[VIEW:]
    assert d_buf.data_ptr() % 16 == 0
    for o, k in zip(off, blocks):
        assert (d_in.data_ptr() + o) % 16 == k.align
    d_n = torch.tensor([k.n for k in blocks], dtype=torch.int64, device=_dev())
    d_crc = torch.full((nb + 2,), CANARY, dtype=torch.int32, device=_dev())
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        bt.crc32_dev(st, d_in, off, [k.cap for k in blocks], d_n, d_crc[1:])
        _, errs = bt.finish(st, nb, raise_on_error=False)
    finally:
        bt.close()
    crc = d_crc.cpu().numpy().view(np.uint32)
    assert int(crc[0]) == CANARY and int(crc[nb + 1]) == CANARY, "d_crc was written outside [0, nblocks)"
    assert np.array_equal(d_buf.cpu().numpy(), host), "the input was written"
    assert d_n.cpu().tolist() == [k.n for k in blocks]
    return [int(c) for c in crc[1:nb + 1]], errs


def _check(shafa, blocks, labels, **kw):
    got, errs = _run(shafa, blocks, **kw)
    assert not any(errs), [(l, e) for l, e in zip(labels, errs) if e]
    bad = [(l, hex(g), hex(k.want())) for l, g, k in zip(labels, got, blocks) if g != k.want()]
    assert not bad, f"(block, d_crc, zlib): {bad[:12]}"
    return got


def _every_block(kinds):
    blocks, labels = [], []
    for kind in kinds:
        for n in LENGTHS:
            for al in _aligns(n):
                if n == WIDE and kind != "random" and al not in (0, 7):
                    continue
                # exact regions and regions with slack behind d_in_n
                blocks.append(_Blk(_content(kind, n + (n + al) % 3 * 9, n + al)[:n + (n + al) % 3 * 9], al, n=n,
                                   cap=n + (n + al) % 3 * 9))
                labels.append((kind, n, al))
    return blocks, labels


# ---------------------------------------------------------------- 1. lengths, alignments, contents
def test_check_vector_and_empty(shafa):
    v = np.frombuffer(b"123456789", dtype=np.uint8)
    blocks = [_Blk(v, al) for al in range(16)] + [_Blk(v[:0], 5), _Blk(v, 3, n=0, cap=9), _Blk(v, 9, n=4), _Blk(v, 2, n=3)]
    got = _check(shafa, blocks, list(range(len(blocks))))
    assert got[:16] == [0xCBF43926] * 16 and got[16] == 0 and got[17] == 0


def test_random_bytes_every_length_and_alignment(shafa):
    _check(shafa, *_every_block(["random"]))


def test_zeros_and_ones_every_length_and_alignment(shafa):
    _check(shafa, *_every_block(["zeros", "ones"]))


# ---------------------------------------------------------------- 2. neighbours
def test_bytes_outside_the_regions_do_not_count(shafa):
    blocks, labels = _every_block(["random"])
    blocks = [k for k in blocks if k.n != WIDE or k.align == 7]
    labels = [l for l in labels if l[1] != WIDE or l[2] == 7]
    a = _check(shafa, blocks, labels)
    b = _check(shafa, blocks, labels, flip_outside=True)
    assert a == b


# ---------------------------------------------------------------- 3. bounds
def test_size_past_capacity(shafa):
    x = _content("random", BIG, 1)
    blocks = [_Blk(x, 1), _Blk(x, 5, n=BIG, cap=BIG - 1), _Blk(x[:100], 7), _Blk(x[:17], 0, n=1 << 40, cap=17), _Blk(x, 15),
              _Blk(x[:0], 3, n=1, cap=0), _Blk(x[:TILE], 2)]
    got, errs = _run(shafa, blocks)
    OM = shafa.OUTSIDE_MODULE
    assert errs == [0, OM, 0, OM, 0, OM, 0]
    assert got == [k.want() for k in blocks] and got[1] == got[3] == got[5] == 0


# ---------------------------------------------------------------- 4. the combine
def _combine(shafa, crcs, lens, first, count):
    import torch
    nf = len(first)
    d_crc = torch.from_numpy(np.asarray(crcs, dtype=np.uint32).view(np.int32).copy()).to(_dev())
    d_n = torch.from_numpy(np.asarray(lens, dtype=np.uint64).view(np.int64).copy()).to(_dev())
    d_fc = torch.full((nf + 2,), CANARY, dtype=torch.int32, device=_dev())
    d_fn = torch.full((nf + 2,), CANARY, dtype=torch.int64, device=_dev())
    bt = shafa.Batch(max(nf, 4), 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        bt.crc32_combine_dev(st, first, count, d_crc, d_n, d_fc[1:], d_fn[1:])
        _, errs = bt.finish(st, nf, raise_on_error=False)
    finally:
        bt.close()
    assert not any(errs)
    fc, fn = d_fc.cpu().numpy().view(np.uint32), d_fn.cpu().numpy().view(np.uint64)
    assert int(fc[0]) == CANARY == int(fc[nf + 1]) and int(fn[0]) == CANARY == int(fn[nf + 1])
    return [int(c) for c in fc[1:nf + 1]], [int(n) for n in fn[1:nf + 1]]


def test_combine_against_zlib(shafa):
    rng = np.random.default_rng(7)
    lens = [0, 5, 0, 70000, 1, 0, 33, 0] + [int(rng.choice([0, 1, 17, 300, 9000])) for _ in range(300)] + [0, 12, 0]
    parts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    crcs = [zlib.crc32(p) for p in parts]
    # 1 block, 2 blocks, none, 300 blocks with empty ones at the start, middle and end, all of them, an empty block alone,
    # and two files that share no block
    files = [(3, 1), (3, 2), (4, 0), (7, 300), (0, len(parts)), (0, 1), (0, 4), (4, 4), (len(parts) - 3, 3), (0, 0)]
    assert lens[7] == 0 and lens[4] == 1 and lens[5] == 0
    got_c, got_n = _combine(shafa, crcs, lens, [f for f, _ in files], [c for _, c in files])
    for (f, c), gc, gn in zip(files, got_c, got_n):
        whole = b"".join(parts[f:f + c])
        assert gn == len(whole) and gc == zlib.crc32(whole), (f, c, hex(gc), gn)
    # associative: the files (0, 4) and (4, 4) joined by a second call are the file (0, 8)
    c2, n2 = _combine(shafa, got_c[6:8], got_n[6:8], [0], [2])
    assert c2 == [zlib.crc32(b"".join(parts[:8]))] and n2 == [sum(lens[:8])]


def test_combine_lengths_above_2_32(shafa):
    rng = np.random.default_rng(9)
    L = (1 << 33) + 5
    crcs = [int(c) for c in rng.integers(0, 1 << 32, 6, dtype=np.uint64)]
    lens = [L, 0, L, 7, (1 << 40) - 1, L]
    got_c, got_n = _combine(shafa, crcs, lens, [0, 2, 0], [6, 3, 2])
    for (f, c), gc, gn in zip([(0, 6), (2, 3), (0, 2)], got_c, got_n):
        want = 0
        for crc, n in zip(crcs[f:f + c], lens[f:f + c]):
            want = shafa.crc32_combine(want, crc, n)
        assert gc == want and gn == sum(lens[f:f + c]), (f, c)


# ---------------------------------------------------------------- 5. shafa.crc32
def test_crc32_driver(shafa):
    import torch
    host = _RANDOM[:(1 << 20) + 77]
    d = torch.from_numpy(np.concatenate([host[:5], host])).to(_dev())[5:]
    assert d.data_ptr() % 16 == 5
    want = zlib.crc32(host.tobytes())
    got = shafa.crc32(d)
    assert type(got) is int and got == want
    assert shafa.crc32(d[:0]) == 0 and shafa.crc32(torch.zeros(0, dtype=torch.uint8, device=_dev())) == 0
    assert shafa.crc32(d[:0], sizes=[0, 0]) == [0, 0]
    # segments at odd offsets, empty ones among them, the tensor's tail not covered
    sizes = [1, 0, 4097, 0, 65536 + 3, 9, 0]
    got = shafa.crc32(d, sizes=sizes)
    pos, wants = 0, []
    for n in sizes:
        wants.append(zlib.crc32(host[pos:pos + n].tobytes()))
        pos += n
    assert got == wants and all(type(g) is int for g in got)
    # a segment cut into pieces: 1 MiB + 77 in pieces of 40000 bytes (27 pieces, the last one short), then of 8192 and 1 << 20
    for piece in (40000, 8192, 1 << 20):
        assert shafa.crc32(d, _piece=piece) == want, piece
        assert shafa.crc32(d, sizes=[70001, 0, 1 << 19, 5], _piece=piece) == \
            [zlib.crc32(host[:70001].tobytes()), 0, zlib.crc32(host[70001:70001 + (1 << 19)].tobytes()),
             zlib.crc32(host[70001 + (1 << 19):70006 + (1 << 19)].tobytes())], piece
    for bad in ([-1], [d.numel() + 1]):
        with pytest.raises(ValueError):
            shafa.crc32(d, sizes=bad)

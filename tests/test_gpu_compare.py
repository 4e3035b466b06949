"""The compare pass (shafa_hipd_compare_dev, csrc/compare.hip) through the C-ABI, against numpy on host copies.

Side a: 16-aligned regions of one device buffer, sizes in device memory, the slack of every region and the gaps between
them filled with 0xFE.  Side ref: every block's bytes at its own alignment (0..15) inside a view, at storage offset 3, of a
larger tensor filled with 0xFF.  The blocks' own bytes are below 0xFE, so a byte read out of range on either side differs
from whatever it is compared with.  Every test is one call with many blocks (a block's answer is its own); after every call
d_first[nblocks] and both buffers are what they were.

1. equal blocks: d_first == n, every length at every alignment;
2. one difference: at byte 0, at n - 1, at the tile seam (8191, 8192), at the last byte of the last whole word;
3. two differences: the first wins — in different tiles, in different waves of a tile, in one lane's two words, in one word;
4. a difference only behind d_a_n in the region, or only behind h_ref_n in ref, is not seen (and is, one byte sooner);
5. unequal sizes with an equal prefix give the smaller size, with a difference in the prefix that difference;
6. eight blocks of mixed lengths (0 and 5 tiles among them), some equal, some not;
7. d_a_n > h_a_cap: OUTSIDE_MODULE and d_first = 0 for that block, its neighbours as without it."""
import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

SENT = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64
TILE = 8192
BIG = 3 * TILE + 5
LENGTHS = [0, 1, 15, 16, 17, 31, 33, TILE - 1, TILE, TILE + 1]
REF_VIEW = 3                        # storage offset of the view handed over as d_ref


def _al16(n):
    return (n + 15) // 16 * 16


def _aligns(n):
    return range(16) if n == BIG else (0, 1, 7, 15)


def _data(seed, n):
    return np.random.default_rng(seed).integers(0, 0xFE, n, dtype=np.uint8)


class _Blk:
    """one block: a = the region's bytes in front of a_n (and, if longer, the slack behind it), ref = the original's bytes
    (ref_tail: what follows them in ref's buffer), align = ref's address mod 16, cap = the region's capacity"""

    def __init__(self, a, ref, align=0, a_n=None, cap=None, ref_tail=b""):
        self.a = np.asarray(a, dtype=np.uint8)
        self.ref = np.asarray(ref, dtype=np.uint8)
        self.align = align
        self.a_n = len(self.a) if a_n is None else a_n
        self.cap = max(len(self.a), self.a_n) if cap is None else cap
        self.ref_tail = np.frombuffer(bytes(ref_tail), dtype=np.uint8)

    def want(self):
        m = min(self.a_n, len(self.ref))
        d = np.flatnonzero(self.a[:m] != self.ref[:m])
        return int(d[0]) if d.size else m


def _flip(x, *at):
    y = x.copy()
    for i in at:
        y[i] ^= 0x5A
        if y[i] >= 0xFE:            # stay below the fill bytes, and different from x[i]
            y[i] = (int(x[i]) + 1) % 0xFE
    return y


def _run(shafa, blocks):
    """one compare_dev call over these blocks -> (d_first[0 .. nb) as a list, the per-block codes); asserts the canaries"""
    import torch
    nb = len(blocks)
    a_off, pos = [], 0
    for k in blocks:
        a_off.append(pos)
        pos += _al16(max(k.cap, len(k.a))) + 16
    host_a = np.full(pos + 16, 0xFE, dtype=np.uint8)
    for o, k in zip(a_off, blocks):
        host_a[o:o + len(k.a)] = k.a
    ref_off, pos = [], 64
    for k in blocks:
        pos += (k.align - (REF_VIEW + pos)) % 16
        ref_off.append(pos)
        pos += len(k.ref) + len(k.ref_tail) + 40
    host_r = np.full(REF_VIEW + pos + 64, 0xFF, dtype=np.uint8)
    for o, k in zip(ref_off, blocks):
        host_r[REF_VIEW + o:REF_VIEW + o + len(k.ref)] = k.ref
        host_r[REF_VIEW + o + len(k.ref):REF_VIEW + o + len(k.ref) + len(k.ref_tail)] = k.ref_tail
    d_a = torch.from_numpy(host_a).to(_dev())
    d_r = torch.from_numpy(host_r).to(_dev())
    d_ref = d_r[REF_VIEW:]
    assert d_a.data_ptr() % 16 == 0 and d_r.data_ptr() % 16 == 0
    for o, k in zip(ref_off, blocks):
        assert (d_ref.data_ptr() + o) % 16 == k.align
    d_a_n = torch.tensor([k.a_n for k in blocks], dtype=torch.int64, device=_dev())
    d_first = torch.full((nb + 1,), SENT, dtype=torch.int64, device=_dev())
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        bt.compare_dev(st, d_a, a_off, [k.cap for k in blocks], d_a_n, d_ref, ref_off, [len(k.ref) for k in blocks], d_first)
        _, errs = bt.finish(st, nb, raise_on_error=False)
    finally:
        bt.close()
    first = d_first.cpu().numpy()
    assert int(first[nb]) == SENT, "d_first[nblocks] was written"
    assert np.array_equal(d_a.cpu().numpy(), host_a) and np.array_equal(d_r.cpu().numpy(), host_r), "an operand was written"
    assert d_a_n.cpu().tolist() == [k.a_n for k in blocks]
    return first[:nb].view(np.uint64).tolist(), errs


def _check(shafa, blocks, labels):
    got, errs = _run(shafa, blocks)
    assert not any(errs), [(l, e) for l, e in zip(labels, errs) if e]
    bad = [(l, g, k.want()) for l, g, k in zip(labels, got, blocks) if g != k.want()]
    assert not bad, f"(block, d_first, numpy): {bad[:12]}"


def _every_length():
    for n in LENGTHS + [BIG]:
        for al in _aligns(n):
            yield n, al


# ---------------------------------------------------------------- 1. equal
def test_equal_blocks(shafa):
    blocks, labels = [], []
    for n, al in _every_length():
        x = _data(n + al, n)
        blocks.append(_Blk(x, x, al, cap=n + (n + al) % 3 * 9))      # exact regions and regions with slack
        labels.append((n, al))
    assert all(k.want() == len(k.ref) for k in blocks)
    _check(shafa, blocks, labels)


# ---------------------------------------------------------------- 2. one difference
def test_one_difference(shafa):
    blocks, labels = [], []
    for n, al in _every_length():
        x = _data(100 + n + al, n)
        for at in sorted({0, n - 1, TILE - 1, TILE, n // 16 * 16 - 1, n // 16 * 16, BIG - 6, 2 * TILE + 4095}):
            if 0 <= at < n:
                blocks.append(_Blk(x, _flip(x, at), al) if (n + at) % 2 else _Blk(_flip(x, at), x, al))
                labels.append((n, al, at))
                assert blocks[-1].want() == at
    _check(shafa, blocks, labels)


# ---------------------------------------------------------------- 3. two differences: the first wins
PAIRS = [(5, TILE + 7), (TILE - 1, TILE), (TILE + 3, 2 * TILE + 1),            # different tiles
         (1027, 2057), (1025, 4096 + 5), (4096 + 5, 1024 * 3 + 1),             # different waves of one tile
         (40, 4096 + 40), (4096 + 41, 44),                                     # one lane's two words
         (16, 31), (33, 34), (1, 14)]                                          # one word


def test_two_differences(shafa):
    blocks, labels = [], []
    for n in (33, TILE - 1, TILE + 1, BIG):
        for al in _aligns(n):
            x = _data(200 + n + al, n)
            for p, q in PAIRS:
                if max(p, q) < n:
                    blocks.append(_Blk(x, _flip(x, p, q), al))
                    labels.append((n, al, p, q))
                    assert blocks[-1].want() == min(p, q)
    assert len({l[2:] for l in labels}) == len(PAIRS)
    _check(shafa, blocks, labels)


# ---------------------------------------------------------------- 4. bytes that do not count
def test_slack_and_bytes_behind_ref_are_not_seen(shafa):
    blocks, labels = [], []
    for n, al in _every_length():
        x = _data(300 + n + al, n + 48)
        for d in (0, 1, 15, 16, 40):                                   # a difference d bytes behind the end
            y = _flip(x, n + d)
            # both sides n bytes long; the region goes on as ref's buffer does, but for that byte
            blocks.append(_Blk(y, x[:n], al, a_n=n, ref_tail=x[n:]))
            labels.append(("slack", n, al, d))
            blocks.append(_Blk(x, y[:n], al, a_n=n, ref_tail=y[n:]))
            labels.append(("behind ref", n, al, d))
            assert blocks[-1].want() == n and blocks[-2].want() == n
        # the control: one byte more on both sides and the difference right behind the end is inside
        y = _flip(x, n)
        blocks.append(_Blk(y, x[:n + 1], al, a_n=n + 1, ref_tail=x[n + 1:]))
        labels.append(("control", n, al))
        assert blocks[-1].want() == n
    _check(shafa, blocks, labels)


# ---------------------------------------------------------------- 5. unequal sizes
def test_unequal_sizes(shafa):
    blocks, labels = [], []
    for n, al in _every_length():
        x = _data(400 + n + al, n + 40)
        for more in (1, 16, 33):
            blocks.append(_Blk(x[:n], x[:n + more], al))               # a_n < ref_n
            labels.append(("a short", n, al, more))
            blocks.append(_Blk(x[:n + more], x[:n], al))               # a_n > ref_n
            labels.append(("ref short", n, al, more))
            assert blocks[-1].want() == n and blocks[-2].want() == n
            if n:
                blocks.append(_Blk(x[:n + more], _flip(x[:n], n - 1), al))
                labels.append(("ref short, differs", n, al, more))
                assert blocks[-1].want() == n - 1
    _check(shafa, blocks, labels)


# ---------------------------------------------------------------- 6. one call, mixed blocks
def test_mixed_call(shafa):
    big = _data(500, 5 * TILE)
    x = [_data(501 + i, n) for i, n in enumerate((0, 1, 100, TILE, TILE + 77, 3000, 17))]
    blocks = [_Blk(x[0], x[0], 4), _Blk(big, _flip(big, 4 * TILE + 123), 9), _Blk(x[1], x[1], 15),
              _Blk(x[2], _flip(x[2], 99), 2), _Blk(x[3], x[3], 1), _Blk(x[4], _flip(x[4], TILE, TILE + 76), 0),
              _Blk(x[5], x[5][:2000], 13), _Blk(x[6], _flip(x[6], 0), 6)]
    assert [k.want() for k in blocks] == [0, 4 * TILE + 123, 1, 99, TILE, TILE, 2000, 0]
    _check(shafa, blocks, list(range(8)))
    # the same blocks in the opposite order: a block's answer does not depend on its place
    _check(shafa, blocks[::-1], list(range(8))[::-1])


# ---------------------------------------------------------------- 7. a size past its capacity
def test_size_past_the_capacity(shafa):
    x = [_data(600 + i, n) for i, n in enumerate((100, 2 * TILE + 5, 48, 33))]
    mk = lambda over: [_Blk(x[0], _flip(x[0], 50), 3),
                       _Blk(x[1], _flip(x[1], 7), 5, a_n=len(x[1]) + (1 if over else 0), cap=len(x[1])),
                       _Blk(x[2], x[2], 11),
                       _Blk(x[3][:16], x[3], 0, a_n=17 if over else 16, cap=16)]
    got0, errs0 = _run(shafa, mk(False))
    assert errs0 == [0, 0, 0, 0] and got0 == [50, 7, 48, 16]
    got, errs = _run(shafa, mk(True))
    assert errs == [0, shafa.OUTSIDE_MODULE, 0, shafa.OUTSIDE_MODULE], errs
    assert got == [50, 0, 48, 0], got

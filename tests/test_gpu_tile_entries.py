"""The entries whose launchers take their workspace from tile_setup (csrc/internal.hpp), one behind another on ONE batch and ONE
stream with no synchronisation in between and one finish at the end: rle_decoded_size_dev, rle_encoded_size_dev,
rle_encoded_hist_dev, compare_dev, crc32_dev, find_dev, and split + merge of planes (element 2), of planes XOR (element 4, one
block without a base), of differences (element 8) and of records (width 3).  Every launch lays its offsets, capacities, extras
and tile bases over the workspace the launch in front has used, so a part that one of them misplaces shows in the next one's
result.

Five blocks — an odd count, so that the 4-byte tile bases do not end at a multiple of 16 behind the 8-byte arrays: a capacity of
0, 1 unit, 8192 units (one whole tile), 8193 (two tiles, the second with one unit) and 16 389 (three tiles) at an odd byte
offset wherever the entry takes one.  Then the same sequence on the same batch with three of the blocks, so that every part
moves.  Expected values: numpy, zlib.crc32, bytes.find, and for the RLE sizes the oracle (seek_index_dev needs coded input and
stays with test_gpu_seek.py)."""
import zlib

import numpy as np
import pytest

from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

UNITS = [0, 1, 8192, 8193, 16389]
PATTERN = b"\x41\x42\x43"
NO_BASE_BLOCK = 2               # of the XOR launches: the block without a base (where the call has that many)


def _al16(n):
    return (n + 15) // 16 * 16


def _stream_bytes(rng, n):
    """exactly n bytes of whole RLE tokens — literals, {0, symbol, count} triples — with PATTERN here and there, and across
    the first tile border where the block reaches it"""
    b = bytearray()

    def fill(upto):
        while len(b) < upto:
            r = rng.random()
            if upto - len(b) >= 3 and r < 0.10:
                b.extend((0, int(rng.integers(0, 256)), int(rng.integers(1, 256))))
            elif upto - len(b) >= 3 and r < 0.12:
                b.extend(PATTERN)
            else:
                b.append(int(rng.integers(1, 256)))

    if n >= 8193:
        fill(8190)
        b.extend(PATTERN)                                              # bytes 8190 .. 8192
    fill(n)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _place(blocks, odd_last, shift=0):
    """the blocks in one host image filled with 0xEE -> (image, offsets): 16-aligned offsets (+ shift), the last block's odd
    with odd_last"""
    off, pos = [], 32
    for i, b in enumerate(blocks):
        off.append(pos + shift + (7 if odd_last and i == len(blocks) - 1 else 0))
        pos += _al16(b.size) + 48
    img = np.full(pos + 64, 0xEE, dtype=np.uint8)
    for o, b in zip(off, blocks):
        img[o:o + b.size] = b
    return img, off


def _planes_of(x, n, w):
    """the w byte columns of n units of w bytes"""
    return [x.reshape(n, w)[:, j] for j in range(w)]


def _zigzag_diff(x, n):
    """the bytes of the zigzag-folded differences of n uint64"""
    v = x.view("<u8")
    d = (v - np.concatenate([np.zeros(1, dtype=np.uint64), v[:-1]])) if n else v
    z = (d << np.uint64(1)) ^ (d.view(np.int64) >> np.int64(63)).view(np.uint64)
    return z.view(np.uint8)


class _Transpose:
    """split then merge of one variant over `units`: the inputs, the outputs of its own, the expected images"""

    def __init__(self, rng, units, width, kind):
        import torch
        self.units, self.w, self.kind = units, width, kind
        blocks = [rng.integers(0, 256, n * width, dtype=np.uint8) for n in units]
        if kind == "planes_diff":                                      # small steps with a jump now and then, either sign
            blocks = [(np.cumsum(rng.integers(-3, 4, n)).astype(np.int64) * (1 << 20) + rng.integers(0, 2, n) * -(1 << 50))
                      .astype("<i8").view(np.uint8) for n in units]
        self.img, self.off = _place(blocks, odd_last=True)
        self.d_in = torch.from_numpy(self.img).to(_dev())
        coded = blocks
        self.base_off = None
        if kind == "planes_xor":
            bases = [rng.integers(0, 256, b.size, dtype=np.uint8) for b in blocks]
            bimg, boff = _place(bases, odd_last=False, shift=3)        # the base side at an alignment of its own
            self.d_base = torch.from_numpy(bimg).to(_dev())
            have = [i != NO_BASE_BLOCK for i in range(len(blocks))]
            self.base_off = [o if h else (1 << 64) - 1 for o, h in zip(boff, have)]
            coded = [b ^ s if h else b for b, s, h in zip(blocks, bases, have)]
        if kind == "planes_diff":
            coded = [_zigzag_diff(b, n) for b, n in zip(blocks, units)]
        self.poff, pos = [], 0
        for n in units:
            self.poff += [pos + j * _al16(n) for j in range(width)]
            pos += width * _al16(n) + 16
        self.want_planes = np.full(pos + 16, 0xEE, dtype=np.uint8)
        at = 0
        for b, n in zip(coded, units):
            for p in _planes_of(b, n, width):
                self.want_planes[self.poff[at]:self.poff[at] + n] = p
                at += 1
        self.d_planes = torch.full((pos + 16,), 0xEE, dtype=torch.uint8, device=_dev())
        self.d_out = torch.full((self.img.size,), 0xEE, dtype=torch.uint8, device=_dev())
        self.d_n = torch.tensor(units, dtype=torch.int64, device=_dev())

    def enqueue(self, bt, st):
        side = () if self.base_off is None else (self.d_base, self.base_off)
        split, merge = getattr(bt, f"split_{self.kind}_dev"), getattr(bt, f"merge_{self.kind}_dev")
        split(st, self.w, self.d_in, self.off, *side, self.units, self.d_n, self.d_planes, self.poff)
        merge(st, self.w, self.d_planes, self.poff, *side, self.units, self.d_n, self.d_out, self.off)

    def check(self, what):
        got = self.d_planes.cpu().numpy()
        bad = np.flatnonzero(got != self.want_planes)
        assert not bad.size, f"{what}: split_{self.kind}_dev: {bad.size} plane bytes differ, the first at {int(bad[0])}"
        got = self.d_out.cpu().numpy()
        bad = np.flatnonzero(got != self.img)                          # the regions, and no byte around them
        assert not bad.size, f"{what}: merge_{self.kind}_dev: {bad.size} bytes differ, the first at {int(bad[0])}"


class _Round:
    """every entry over the blocks of `units`: prepared first, enqueued without a synchronisation, checked after the finish"""

    def __init__(self, shafa, oracle, rng, units):
        import torch
        self.shafa, self.units, self.nb = shafa, units, len(units)
        dev = _dev()
        self.blocks = [_stream_bytes(rng, n) for n in units]
        img, self.off = _place(self.blocks, odd_last=False)            # the RLE passes and compare_dev take 16-aligned regions
        self.d_al = torch.from_numpy(img).to(dev)
        img, self.odd = _place(self.blocks, odd_last=True)             # crc32_dev and find_dev any
        self.d_odd = torch.from_numpy(img).to(dev)
        self.d_n = torch.tensor(units, dtype=torch.int64, device=dev)
        # the oracle's RLE sizes: every block is whole tokens and decodes
        dec = [oracle.rle_decode(b, cap=int(shafa.RLE_DECODE_MAX)) for b in self.blocks]
        assert all(rc == 0 for rc, _ in dec)
        self.want_dec = [int(out.size) for _, out in dec]
        enc = [oracle.rle_encode(b) for b in self.blocks]
        self.want_enc = [int(e.size) for e in enc]
        self.want_hist = np.stack([np.bincount(e, minlength=256).astype(np.int64) for e in enc])
        # compare_dev: the reference at an odd offset; a difference in a tile's last byte, one in a second tile's only byte, a
        # shorter reference, equal blocks
        refs = [b.copy() for b in self.blocks]
        for r, n in zip(refs, units):
            if n == 8192:
                r[8191] ^= 0x10
            if n == 8193:
                r[8192] ^= 0x01
        refs = [r[:-5] if n == 16389 else r for r, n in zip(refs, units)]
        img, self.ref_off = _place(refs, odd_last=True, shift=5)
        self.d_ref = torch.from_numpy(img).to(dev)
        self.ref_n = [int(r.size) for r in refs]
        self.want_first = []
        for b, r in zip(self.blocks, refs):
            m = min(b.size, r.size)
            d = np.flatnonzero(b[:m] != r[:m])
            self.want_first.append(int(d[0]) if d.size else m)
        self.want_crc = [zlib.crc32(b.tobytes()) for b in self.blocks]
        # find_dev: block b's positions count from pos[b]
        self.pos = [1000000 * (i + 1) for i in range(self.nb)]
        self.want_hits, self.want_count = [], []
        for b, p in zip(self.blocks, self.pos):
            s, at, c = b.tobytes(), -1, 0
            while (at := s.find(PATTERN, at + 1)) >= 0:
                self.want_hits.append(p + at)
                c += 1
            self.want_count.append(c)
        assert any(n >= 8193 for n in units) <= any((h % 1000000) == 8190 for h in self.want_hits)
        self.max_hits = len(self.want_hits) + 8
        # outputs, each entry's own, pre-filled
        i64 = lambda n, v=-1: torch.full((n,), v, dtype=torch.int64, device=dev)
        self.d_dec, self.d_enc, self.d_hn, self.d_hist = i64(self.nb), i64(self.nb), i64(self.nb), i64(self.nb * 256)
        self.d_first, self.d_count, self.d_total, self.d_hits = i64(self.nb), i64(self.nb), i64(1, 0), i64(self.max_hits)
        self.d_crc = torch.full((self.nb,), -1, dtype=torch.int32, device=dev)
        self.transposes = [_Transpose(rng, units, 2, "planes"), _Transpose(rng, units, 4, "planes_xor"),
                           _Transpose(rng, units, 8, "planes_diff"), _Transpose(rng, units, 3, "records")]

    def enqueue(self, bt, st):
        u = self.units
        bt.rle_decoded_size_dev(st, self.d_al, self.off, u, self.d_n, self.d_dec)
        bt.rle_encoded_size_dev(st, self.d_al, self.off, u, self.d_n, self.d_enc)
        self.transposes[3].enqueue(bt, st)
        bt.rle_encoded_hist_dev(st, self.d_al, self.off, u, self.d_n, self.d_hn, self.d_hist)
        self.transposes[1].enqueue(bt, st)
        bt.compare_dev(st, self.d_al, self.off, u, self.d_n, self.d_ref, self.ref_off, self.ref_n, self.d_first)
        self.transposes[2].enqueue(bt, st)
        bt.crc32_dev(st, self.d_odd, self.odd, u, self.d_n, self.d_crc)
        self.transposes[0].enqueue(bt, st)
        bt.find_dev(st, self.d_odd, self.odd, u, self.d_n, None, self.pos, PATTERN, self.max_hits, self.d_hits, self.d_count,
                    self.d_total)

    def check(self, what):
        host = lambda t: t.cpu().numpy().tolist()
        assert host(self.d_dec) == self.want_dec, f"{what}: rle_decoded_size_dev"
        assert host(self.d_enc) == self.want_enc, f"{what}: rle_encoded_size_dev"
        assert host(self.d_hn) == self.want_enc, f"{what}: rle_encoded_hist_dev's sizes"
        assert (self.d_hist.cpu().numpy().reshape(self.nb, 256) == self.want_hist).all(), f"{what}: rle_encoded_hist_dev's counts"
        assert host(self.d_first) == self.want_first, f"{what}: compare_dev"
        assert [c & 0xFFFFFFFF for c in host(self.d_crc)] == self.want_crc, f"{what}: crc32_dev"
        assert host(self.d_count) == self.want_count and host(self.d_total) == [len(self.want_hits)], f"{what}: find_dev's counts"
        assert host(self.d_hits)[:len(self.want_hits)] == self.want_hits, f"{what}: find_dev's positions"
        for t in self.transposes:
            t.check(what)


def test_every_tile_entry_behind_another_on_one_batch(shafa, oracle):
    import torch
    rng = np.random.default_rng(20261019)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(len(UNITS), 1 << 20)
    try:
        for what, units in (("five blocks", UNITS), ("three blocks", [UNITS[3], UNITS[1], UNITS[4]])):
            r = _Round(shafa, oracle, rng, units)
            torch.cuda.synchronize()                                   # the inputs are there; from here on only launches
            r.enqueue(bt, st)
            _, errs = bt.finish(st, len(units), raise_on_error=False)
            assert errs == [0] * len(units), (what, errs)
            r.check(what)
    finally:
        bt.close()

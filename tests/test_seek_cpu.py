"""CPU-side checks of the seek index entries (shafa_hipd_seek_index_dev, shafa_hipd_read_spans_dev, csrc/seek.hip) and of
shafa.build_index / read_ranges / read_range: declared, exported, bound in Python, the ABI version unchanged, every argument
error refused before HIP is touched, and read_ranges' ValueErrors raised before a device is touched (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shafa_hipd_seek_index_dev", "shafa_hipd_read_spans_dev")


def _i32(*v):
    return (C.c_int * len(v))(*v)


def test_declared_exported_and_bound(shafa):
    decl = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in decl and hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("seek_index_dev", "read_spans_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("build_index", "read_ranges", "read_range"):
        assert callable(getattr(shafa, name, None)), name
    assert shafa.SeekBlock._fields == ("decoded_size", "n_symbols", "payload_offset", "payload_size", "first_checkpoint", "indexed")
    with open(os.path.join(ROOT, "include", "shafa_hip.h")) as f:
        text = f.read()
    assert (shafa.SEEK_SF, shafa.SEEK_RLE, shafa.SEEK_UNINDEXED) == (1, 2, 1)
    for line in ("#define SHAFA_SEEK_SF 1", "#define SHAFA_SEEK_RLE 2", "#define SHAFA_SEEK_UNINDEXED 1u"):
        assert line in text, line


def test_seek_index_dev_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM, LM = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY

    def call(**kw):
        a = dict(b=A.p, nb=3, d_in=A.p, off=_u64(0, 16, 4096), cap=_u64(5, 100, 70000), d_in_n=A.p, tab=A.p, span=1024,
                 flags=shafa.SEEK_SF | shafa.SEEK_RLE, first=_u64(0, 1, 2), ck=A.p, status=A.p, out_n=A.p)
        a.update(kw)
        return L.shafa_hipd_seek_index_dev(a["b"], None, a["nb"], a["d_in"], a["off"], a["cap"], a["d_in_n"], a["tab"],
                                           a["span"], a["flags"], a["first"], a["ck"], a["status"], a["out_n"])

    assert call() not in (shafa.SUCCESS, OM, LM)                       # every check passed: HIP refuses the stand-in batch
    for k in ("b", "d_in", "d_in_n", "ck", "status", "out_n", "off", "cap", "first", "tab"):
        assert call(**{k: None}) == OM, k
    assert call(tab=None, flags=shafa.SEEK_RLE) not in (shafa.SUCCESS, OM, LM)     # no tables wanted without SEEK_SF
    for span in (0, 1, 128, 255, 257, 1000, 3 * 1024, 8191, 16384, 1 << 31):
        assert call(span=span) == OM, span
        assert call(span=span, nb=0) == OM, span                       # the shape comes before the block count
    for span in (256, 512, 2048, 4096, 8192):
        assert call(span=span) not in (shafa.SUCCESS, OM, LM), span
    assert call(flags=4) == OM and call(flags=-1) == OM
    assert call(nb=0) == shafa.SUCCESS and call(nb=-4) == shafa.SUCCESS
    assert call(nb=0, off=None, cap=None, first=None) == shafa.SUCCESS
    assert call(b=None, nb=0) == OM
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM  # above the batch's max_blocks
    assert call(d_in=A.odd) == OM
    assert call(off=_u64(0, 8, 4096)) == OM
    assert call(span=256, cap=_u64(5, (1 << 31) * 256, 7)) == LM       # 2^31 spans or more
    assert call(span=256, cap=_u64(5, ((1 << 31) - 3) * 256, 256)) not in (shafa.SUCCESS, OM, LM)


def test_read_spans_dev_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM, LM = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY

    def call(**kw):
        a = dict(b=A.p, nb=2, d_file=A.odd, file_n=5000, pay_off=_u64(7, 2000), pay_n=_u64(1500, 3000), nsym=_u64(2048, 5000),
                 first=_u64(0, 2), tab=A.p, span=1024, flags=shafa.SEEK_SF, ck=A.p, ni=2, blk=_i32(0, 1), ifirst=_u64(0, 1),
                 ilast=_u64(1, 4), lo=_u64(5, 1024), hi=_u64(1500, 5000), dst=_u64(0, 1495), out=A.p, out_n=1495 + 3976)
        a.update(kw)
        return L.shafa_hipd_read_spans_dev(a["b"], None, a["nb"], a["d_file"], a["file_n"], a["pay_off"], a["pay_n"], a["nsym"],
                                           a["first"], a["tab"], a["span"], a["flags"], a["ck"], a["ni"], a["blk"], a["ifirst"],
                                           a["ilast"], a["lo"], a["hi"], a["dst"], a["out"], a["out_n"])

    assert call() not in (shafa.SUCCESS, OM, LM)                       # every check passed: HIP refuses the stand-in batch
    for k in ("b", "d_file", "ck", "out", "tab", "pay_off", "pay_n", "nsym", "first", "blk", "ifirst", "ilast", "lo", "hi", "dst"):
        assert call(**{k: None}) == OM, k
    assert call(d_file=None, file_n=0, pay_off=_u64(0, 0), pay_n=_u64(0, 0)) not in (shafa.SUCCESS, OM, LM)
    for span in (0, 255, 1000, 16384):
        assert call(span=span) == OM, span
    assert call(flags=8) == OM
    assert call(ni=0) == shafa.SUCCESS and call(ni=-1) == shafa.SUCCESS
    assert call(b=None, ni=0) == OM
    assert call(ni=0x7F7F7F7F + 1) == LM                               # items above the batch's max_blocks
    assert call(nb=0x7F7F7F7F + 1) == LM                               # blocks above it
    assert call(nb=0) == OM
    assert call(pay_n=_u64(1500, 3001)) == OM                          # a payload past the end of its file
    assert call(pay_off=_u64(7, (1 << 64) - 1)) == OM
    assert call(blk=_i32(0, 2)) == OM and call(blk=_i32(-1, 1)) == OM
    assert call(ilast=_u64(2, 4)) == OM                                # block 0 has two checkpoints
    assert call(ilast=_u64(1, 5)) == OM                                # block 1 has five
    assert call(ifirst=_u64(0, 5)) == OM                               # first > last
    assert call(lo=_u64(1501, 1024)) == OM                             # lo > hi
    assert call(out_n=1495 + 3975) == OM                               # the last item's bytes do not fit
    assert call(dst=_u64(0, (1 << 64) - 8)) == OM


def _index(shafa, mode="N"):
    blocks = [shafa.SeekBlock(4096, 4096, 10, 3000, 0, True), shafa.SeekBlock(100, 100, 3020, 80, 4, True)]
    return shafa.SeekIndex(None, blocks, 1024, mode, (3200, 9000), None if mode == "N" else np.zeros(5, dtype=np.uint64))


def test_read_ranges_value_errors_before_a_device(shafa):
    import torch
    idx = _index(shafa)
    assert idx.decoded_size == 4196 and idx.starts == [0, 4096, 4196] and idx.span == 1024
    shaf, cod = torch.zeros(3200, dtype=torch.uint8), torch.zeros(9000, dtype=torch.uint8)
    for ranges in ([(-1, 5)], [(0, 5), (3, -2)], [(0, 1), (-7, -7)]):
        with pytest.raises(ValueError, match="negative"):
            shafa.read_ranges(idx, ranges, shaf=shaf, cod=cod)
    with pytest.raises(ValueError, match="negative"):
        shafa.read_range(idx, -1, 5, shaf=shaf, cod=cod)
    with pytest.raises(ValueError):
        shafa.read_ranges(None, [(0, 1)], shaf=shaf, cod=cod)
    with pytest.raises(ValueError):                                    # host tensors are no file set in device memory
        shafa.read_ranges(idx, [(0, 1)], shaf=shaf, cod=cod)
    with pytest.raises(ValueError):                                    # shaf and cod go together
        shafa.read_ranges(idx, [(0, 1)], shaf=shaf)
    # the lengths and the form are looked at on the host: stand-ins that claim to be device tensors
    class Fake:
        dtype, is_cuda = torch.uint8, True

        def __init__(self, n):
            self.n = n

        def reshape(self, *_):
            return self

        def is_contiguous(self):
            return True

        def numel(self):
            return self.n

        @property
        def device(self):
            raise AssertionError("a device was touched")

    for kw in (dict(shaf=Fake(3201), cod=Fake(9000)), dict(shaf=Fake(3200), cod=Fake(8999)), dict(rle=Fake(3200), freq=Fake(9000))):
        with pytest.raises(ValueError, match="not the files"):
            shafa.read_ranges(idx, [(0, 1)], **kw)
    with pytest.raises(ValueError, match="not the files"):
        shafa.read_ranges(_index(shafa, "rle"), [(0, 1)], shaf=Fake(3200), cod=Fake(9000))


def test_build_index_span_is_checked_first(shafa):
    for span in (0, 100, 255, 1000, 16384, 1024.0, None):
        with pytest.raises(ValueError, match="span"):
            shafa.build_index(shaf=None, cod=None, span=span)


def test_items_from_the_block_table(shafa):
    """mode N: the checkpoints of a range are lo // span .. (hi - 1) // span of each block it touches; an RLE form looks the
    decoded offsets up"""
    idx = _index(shafa)
    items, other = shafa._seek_items(idx, [(0, 1, 0), (1000, 1100, 1), (4000, 4196, 101), (4096, 4097, 297)])
    assert not other
    assert items == [(0, 0, 0, 0, 1, 0), (0, 0, 1, 1000, 1100, 1), (0, 3, 3, 4000, 4096, 101), (1, 0, 0, 0, 100, 197),
                     (1, 0, 0, 0, 1, 297)]
    blocks = [shafa.SeekBlock(5000, 2100, 0, 900, 0, True), shafa.SeekBlock(0, 0, 900, 0, 3, True),
              shafa.SeekBlock(300, 10, 900, 10, 4, False)]
    off = np.array([0, 2000, 2000, 0, 0], dtype=np.uint64)
    idx = shafa.SeekIndex(None, blocks, 1024, "R", (1, 1), off)
    items, other = shafa._seek_items(idx, [(0, 5300, 0), (1999, 2001, 5300), (2000, 2001, 5302)])
    assert items == [(0, 0, 2, 0, 5000, 0), (0, 0, 2, 1999, 2001, 5300), (0, 2, 2, 2000, 2001, 5302)]
    assert other == [(2, 0, 300, 5000)]

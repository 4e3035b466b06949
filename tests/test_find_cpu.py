"""CPU-side checks of the pattern search (shafa_hipd_find_dev, csrc/find.hip) and of shafa.find / find_files: declared,
exported, bound in Python, the ABI version unchanged, every argument error refused before HIP is touched and in the stated
order, and the drivers' ValueErrors before a device is touched (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "shafa_hipd_find_dev"


def test_declared_exported_and_bound(shafa):
    assert NAME in declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    assert hasattr(C.CDLL(shafa.LIB_PATH), NAME)
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "find_dev", None))
    for name in ("find", "find_files"):
        assert callable(getattr(shafa, name, None)), name
    assert shafa.Found._fields == ("count", "positions", "size")
    assert (shafa.FIND_NEXT, shafa.FIND_CONTEXT, shafa.FIND_MAX_PATTERN, shafa.FIND_PIECE) == (1, 2, 256, 1 << 26)
    with open(os.path.join(ROOT, "include", "shafa_hip.h")) as f:
        text = f.read()
    for line in ("#define SHAFA_FIND_MAX_PATTERN 256", "#define SHAFA_FIND_NEXT 1", "#define SHAFA_FIND_CONTEXT 2"):
        assert line in text, line


def test_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS

    def call(**kw):
        a = dict(b=A.p, nb=3, d_in=A.odd, off=_u64(0, 5, (1 << 40) + 3), cap=_u64(5, 100, 70000), d_in_n=A.p, flags=b"\x01\x03\x00",
                 pos=_u64(0, 5, 1 << 50), pat=b"ab\x00c", pat_n=4, max_hits=10, d_hits=A.p, d_count=A.p, d_total=A.p)
        a.update(kw)
        return L.shafa_hipd_find_dev(a["b"], None, a["nb"], a["d_in"], a["off"], a["cap"], a["d_in_n"], a["flags"], a["pos"],
                                     a["pat"], a["pat_n"], a["max_hits"], a["d_hits"], a["d_count"], a["d_total"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed (an odd address, odd 64-bit offsets, both flags): HIP refuses the stand-in batch
    assert reached_hip(call())
    assert reached_hip(call(flags=None))                               # NULL flags = all 0
    assert reached_hip(call(max_hits=0, d_hits=None))                  # counts only
    assert reached_hip(call(pat=bytes(256), pat_n=256)) and reached_hip(call(pat_n=1))
    # 1. the device pointers, the pattern and d_hits, in front of nblocks
    for k in ("b", "d_in", "d_in_n", "d_count", "d_total", "pat"):
        assert call(**{k: None}) == OM, k
        assert call(**{k: None}, nb=0) == OM, k
        assert call(**{k: None}, nb=0x7FFFFFFF) == OM, k
    assert call(pat_n=0) == OM and call(pat=bytes(300), pat_n=257) == OM and call(pat_n=0xFFFFFFFF) == OM
    assert call(pat_n=0, nb=0) == OM
    assert call(d_hits=None) == OM and call(d_hits=None, max_hits=1 << 63) == OM and call(d_hits=None, nb=0) == OM
    assert call(b=None, d_in=None, pat_n=0) == OM                      # a NULL batch comes first (all are the same code)
    # 2. nothing to search: success, the host arrays are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, pos=None, flags=None) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, pos=None) == LM
    # 2^31 tiles of 8 KiB or more in the capacities, in one block or in their sum; one tile fewer gets to HIP
    T = 8192
    assert call(cap=_u64(5, (1 << 31) * T, 7)) == LM
    assert call(cap=_u64(1 << 43, 1 << 43, (1 << 31) * T - (1 << 44))) == LM
    assert call(cap=_u64((1 << 64) - 1, 0, 0)) == LM
    assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0)))
    assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1)) == LM
    assert call(cap=_u64(5, (1 << 31) * T, 7), flags=b"\x04\x00\x00") == LM        # in front of the flags
    # 4. the host arrays and the flags
    for k in ("off", "cap", "pos"):
        assert call(**{k: None}) == OM, k
    for bad in (b"\x04\x00\x00", b"\x00\x80\x00", b"\x01\x07\x00", b"\x00\x00\xfe"):
        assert call(flags=bad) == OM, bad
    assert call(flags=b"\x00\x00\x01") == OM and call(flags=b"\x01\x01\x03") == OM  # NEXT on the last region
    assert call(nb=1, flags=b"\x01") == OM and reached_hip(call(nb=1, flags=b"\x02"))
    assert reached_hip(call(nb=2, flags=b"\x01\x02\x01"))              # only the call's regions are looked at


def test_drivers_refuse_bad_arguments(shafa):
    import torch
    cpu = torch.zeros(8, dtype=torch.uint8)
    for bad in (cpu, None, b"abc", cpu.to(torch.int8)):
        with pytest.raises(ValueError):
            shafa.find(bad, b"a")
    # the tensor is looked at first, so nothing below reaches a device either; a pattern and max_hits come before the files
    for e in ({"shaf": cpu, "cod": cpu}, {"rle": cpu, "freq": cpu}, {"shaf": cpu}, {"cod": cpu, "rle": cpu, "freq": cpu}, {},
              {"shaf": cpu, "cod": cpu, "rle": cpu}, {"rle": cpu}):
        with pytest.raises(ValueError):
            shafa.find_files(b"abc", **e)
    for pat in (b"", bytes(257), "text", 5, None, [1, 2]):
        with pytest.raises(ValueError):
            shafa._find_args(pat, 1, "find")
        with pytest.raises(ValueError):
            shafa.find_files(pat, shaf=cpu, cod=cpu)
    for hits in (-1, None, 1.5, "7", True):
        with pytest.raises(ValueError):
            shafa._find_args(b"a", hits, "find")
        with pytest.raises(ValueError):
            shafa.find_files(b"a", shaf=cpu, cod=cpu, max_hits=hits)
    assert shafa._find_args(bytearray(b"ab"), 0, "find") == (b"ab", 0)
    assert shafa._find_args(memoryview(bytes(256)), 1 << 40, "find") == (bytes(256), 1 << 40)

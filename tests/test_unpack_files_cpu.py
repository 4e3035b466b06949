"""CPU-side checks of the segmented parses (shafa_hipd_unpack_cod_files / _unpack_rle_freq_files / _unpack_shaf_files,
csrc/unpack.hip): declared, exported, bound in Python next to decompress_many, the ABI version unchanged, and every argument
error refused before HIP is touched (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["shafa_hipd_unpack_cod_files", "shafa_hipd_unpack_rle_freq_files", "shafa_hipd_unpack_shaf_files"]


def test_declared_and_exported(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    L = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared and hasattr(L, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_python_bindings_exist(shafa):
    for m in ("unpack_cod_files", "unpack_rle_freq_files", "unpack_shaf_files", "unpack_payloads_at"):
        assert callable(getattr(shafa.Batch, m, None)), m
    assert callable(getattr(shafa, "decompress_many", None))
    assert shafa.MANY_GROUP_SLOTS >= shafa.MANY_GROUP_BLOCKS


def test_decompress_many_refuses_malformed_entries(shafa):
    with pytest.raises(ValueError):
        shafa.decompress_many([])
    for bad in ([None], [{}], [{"shaf": None}], [{"rle": 1, "freq": 2}], [{"shaf": b"@0", "cod": b"@N@0@0"}],
                [{"shaf": None, "cod": None, "bogus": 1}]):
        with pytest.raises(ValueError):
            shafa.decompress_many(bad)


def test_decompress_many_refuses_bad_tensors(shafa):
    import torch
    cpu = torch.zeros(8, dtype=torch.uint8)
    for e in ({"shaf": cpu, "cod": cpu}, {"rle": cpu, "freq": cpu}, {"shaf": cpu}, {"cod": cpu, "rle": cpu, "freq": cpu}):
        with pytest.raises(ValueError):
            shafa.decompress_many([e])


class _Args:
    """stand-ins for the batch and the device pointers, aligned to 16 bytes.  The batch's bytes are 0x7F, so a range check
    against its max_blocks passes for the small ranges used here; a call that gets past every check reaches HIP, which
    refuses the stand-in batch (it names no device) before anything is enqueued."""

    def __init__(self):
        self.raw = C.create_string_buffer(b"\x7f" * 512, 512)
        a = C.addressof(self.raw)
        self.p = C.c_void_p((a + 15) // 16 * 16)


def _i32(*v):
    return (C.c_int * len(v))(*v)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


def _common_errors(call, shafa, arrays):
    OM = shafa.OUTSIDE_MODULE
    assert call() not in (shafa.SUCCESS, OM)                           # every check passed: HIP refuses the stand-in batch
    assert call(b=None) == OM
    for k in arrays:
        assert call(**{k: None}) == OM, k
    assert call(nf=0) == OM and call(nf=-1) == OM
    assert call(mb=_i32(4, 0)) == OM and call(mb=_i32(-1, 3)) == OM    # h_max_blocks[f] < 1
    assert call(fi=_i32(-1, 4)) == OM                                  # a slot range below 0
    assert call(fi=_i32(0, 0x7F7F7F7F - 2)) == OM                      # a slot range past the batch's max_blocks
    assert call(fi=_i32(0, 3)) == OM                                   # overlapping slot ranges: [0, 4) and [3, 6)
    assert call(fi=_i32(4, 0), mb=_i32(3, 5)) == OM                    # [4, 7) and [0, 5), in either order
    assert call(fi=_i32(0, 4), mb=_i32(4, 3)) not in (shafa.SUCCESS, OM)   # adjacent ranges are fine
    assert call(base=None) == OM                                       # a NULL base with a length > 0
    assert call(base=None, n=_u64(0, 0)) not in (shafa.SUCCESS, OM)    # ... and with no bytes at all, fine


def test_cod_files_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, nf=2, fi=_i32(0, 4), mb=_i32(4, 3), base=p, o=_u64(0, 64), n=_u64(64, 32), info=p, sizes=p, tabs=p):
        return L.shafa_hipd_unpack_cod_files(b, None, nf, fi, mb, base, o, n, info, sizes, tabs)

    _common_errors(call, shafa, ("fi", "mb", "o", "n", "info", "sizes", "tabs"))


def test_rle_freq_files_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, nf=2, fi=_i32(0, 4), mb=_i32(4, 3), base=p, o=_u64(0, 64), n=_u64(64, 32), ro=_u64(0, 100),
             rn=_u64(100, 50), info=p, off=p, sz=p):
        return L.shafa_hipd_unpack_rle_freq_files(b, None, nf, fi, mb, base, o, n, ro, rn, info, off, sz)

    _common_errors(call, shafa, ("fi", "mb", "o", "n", "ro", "rn", "info", "off", "sz"))


def test_shaf_files_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, nf=2, fi=_i32(0, 4), mb=_i32(4, 3), base=p, o=_u64(0, 64), n=_u64(64, 32), cnt=p, off=p, sz=p):
        return L.shafa_hipd_unpack_shaf_files(b, None, nf, fi, mb, base, o, n, cnt, off, sz)

    _common_errors(call, shafa, ("fi", "mb", "o", "n", "cnt", "off", "sz"))

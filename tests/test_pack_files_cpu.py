"""CPU-side checks of the segmented packs (shafa_hipd_pack_payloads_files / _pack_cod_files / _pack_freq_files,
csrc/pack.hip): declared, exported, bound in Python next to compress_many, and every argument error is refused before HIP is
touched (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["shafa_hipd_pack_payloads_files", "shafa_hipd_pack_cod_files", "shafa_hipd_pack_freq_files"]


def test_declared_and_exported(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    L = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared and hasattr(L, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_python_bindings_exist(shafa):
    for m in ("pack_payloads_files", "pack_cod_files", "pack_freq_files"):
        assert callable(getattr(shafa.Batch, m, None)), m
    assert callable(getattr(shafa, "compress_many", None))


def test_compress_many_refuses_no_files(shafa):
    with pytest.raises(ValueError):
        shafa.compress_many([], block_size=65536)


class _Args:
    """stand-ins for the batch and the device pointers, aligned to 16 bytes.  The batch's bytes are 0x7F, so a range check
    against its max_blocks passes for the small ranges used here; a call that gets past every check reaches HIP, which
    refuses the stand-in batch (it names no device) with SHAFA_DEVICE_ERROR before anything is enqueued."""

    def __init__(self):
        self.raw = C.create_string_buffer(b"\x7f" * 512, 512)
        a = C.addressof(self.raw)
        self.p = C.c_void_p((a + 15) // 16 * 16)


def _i32(*v):
    return (C.c_int * len(v))(*v)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


def test_payload_argument_errors_are_refused_without_hip(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p
    first, count = _i32(0, 1), _i32(1, 2)                              # files: block 0; blocks 1 .. 2
    off, cap = _u64(0, 16, 32), _u64(16, 16, 16)
    doff, dcap = _u64(0, 4096), _u64(4096, 4096)

    def call(b=p, nf=2, fi=first, co=count, framing=shafa.FRAME_SHAF, src=p, o=off, c=cap, src_n=p, dst=p, do=doff, dc=dcap,
             dst_n=p):
        return L.shafa_hipd_pack_payloads_files(b, None, nf, fi, co, framing, src, o, c, src_n, dst, do, dc, dst_n)

    OM = shafa.OUTSIDE_MODULE
    assert call() not in (shafa.SUCCESS, OM)                           # every check passed: HIP refuses the stand-in batch
    assert call(b=None) == OM
    for k in ("fi", "co", "src", "o", "c", "src_n", "dst", "do", "dc", "dst_n"):
        assert call(**{k: None}) == OM, k
    assert call(nf=0) == OM and call(nf=-1) == OM
    assert call(co=_i32(1, 0)) == OM and call(co=_i32(-1, 2)) == OM    # h_count[f] < 1
    assert call(fi=_i32(-1, 1)) == OM                                  # a block range below 0
    assert call(framing=2) == OM and call(framing=-1) == OM
    assert call(o=_u64(0, 8, 32)) == OM                                # a listed block's d_src + h_src_off not 16-aligned
    assert call(o=_u64(0, 16, 33)) == OM
    assert call(src=C.c_void_p(p.value + 4)) == OM


@pytest.mark.parametrize("which", ["pack_cod_files", "pack_freq_files"])
def test_text_argument_errors_are_refused_without_hip(shafa, which):
    L, A = shafa.lib(), _Args()
    p = A.p
    fn = getattr(L, "shafa_hipd_" + which)
    doff, dcap = _u64(0, 1 << 20), _u64(1 << 20, 1 << 20)

    def call(b=p, nf=2, fi=_i32(0, 1), co=_i32(1, 1), modes=b"RN", sizes=p, data=p, dst=p, do=doff, dc=dcap, dst_n=p):
        return fn(b, None, nf, fi, co, modes, sizes, data, dst, do, dc, dst_n)

    OM = shafa.OUTSIDE_MODULE
    assert call() not in (shafa.SUCCESS, OM)
    assert call(b=None) == OM
    for k in ("fi", "co", "modes", "sizes", "data", "dst", "do", "dc", "dst_n"):
        assert call(**{k: None}) == OM, k
    assert call(nf=0) == OM and call(nf=-2) == OM
    assert call(co=_i32(1, 0)) == OM
    assert call(fi=_i32(0, -1)) == OM
    for modes in (b"Rr", b"nN", b"RX", b"R\0", b"@N"):
        assert call(modes=modes) == OM, modes

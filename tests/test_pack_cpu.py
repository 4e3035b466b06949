"""CPU-side checks of the file packs (shafa_hipd_pack_payloads / _pack_cod / _pack_freq, csrc/pack.hip): declared, exported,
bound in Python, the host-only bounds equal their formulas, and every argument error is refused before HIP is touched (no
GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["shafa_hip_pack_payloads_max", "shafa_hip_pack_cod_max", "shafa_hip_pack_freq_max", "shafa_hipd_pack_payloads",
         "shafa_hipd_pack_cod", "shafa_hipd_pack_freq"]


def digits(v):
    return len(str(v))


def test_declared_and_exported(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    L = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared and hasattr(L, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_python_bindings_exist(shafa):
    for m in ("pack_payloads", "pack_cod", "pack_freq"):
        assert callable(getattr(shafa.Batch, m, None)), m
    for f in ("pack_payloads_max", "pack_cod_max", "pack_freq_max", "compress_files"):
        assert callable(getattr(shafa, f, None)), f
    assert (shafa.FRAME_RAW, shafa.FRAME_SHAF) == (0, 1)


@pytest.mark.parametrize("caps", [[0], [9], [10], [99], [100], [1 << 40], [0, 9, 10, 99, 100, 1 << 40],
                                  [65536] * 10, [1] * 100])
def test_payload_bound_is_the_formula(shafa, caps):
    n = len(caps)
    assert shafa.pack_payloads_max(caps, shafa.FRAME_RAW) == sum(caps)
    assert shafa.pack_payloads_max(caps, shafa.FRAME_SHAF) == 1 + digits(n) + sum(2 + digits(c) + c for c in caps)


@pytest.mark.parametrize("n", [1, 9, 10, 99, 100, 128, 1000])
def test_text_bounds_are_the_formulas(shafa, n):
    assert shafa.pack_cod_max(n) == 3 + digits(n) + n * (22 + 256 * 255 + 255) + 2
    assert shafa.pack_freq_max(n) == 3 + digits(n) + n * (22 + 256 * 20 + 255) + 2


def test_bounds_of_nothing_are_zero(shafa):
    L = shafa.lib()
    caps = (C.c_uint64 * 1)(5)
    assert L.shafa_hip_pack_payloads_max(0, caps, 0) == 0
    assert L.shafa_hip_pack_payloads_max(1, caps, 2) == 0
    assert L.shafa_hip_pack_cod_max(0) == 0 and L.shafa_hip_pack_freq_max(-1) == 0


def test_bounds_cover_the_largest_text(shafa):
    """a .cod block of 256 codes of 255 bits and a .freq block of 256 distinct 20-digit counts, with 20-digit sizes"""
    big = 2 ** 64 - 1
    cod = b"@R@1" + b"@" + str(big).encode() + b"@" + b";".join([b"1" * 255] * 256) + b"@0"
    freq = b"@N@1" + b"@" + str(big).encode() + b"@" + b";".join(str(big - s).encode() for s in range(256)) + b"@0"
    assert len(cod) == shafa.pack_cod_max(1)
    assert len(freq) == shafa.pack_freq_max(1)


class _Args:
    """stand-ins for device pointers (a refused call reads none of them), aligned to 16 bytes"""

    def __init__(self):
        self.raw = C.create_string_buffer(256)
        a = C.addressof(self.raw)
        self.p = C.c_void_p((a + 15) // 16 * 16)


def test_payload_argument_errors_are_refused_without_hip(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p
    off, cap = (C.c_uint64 * 2)(0, 16), (C.c_uint64 * 2)(16, 16)

    def call(b=p, n=2, framing=shafa.FRAME_SHAF, src=p, o=off, c=cap, src_n=p, dst=p, dst_n=p):
        return L.shafa_hipd_pack_payloads(b, None, n, framing, src, o, c, src_n, dst, 1 << 20, dst_n)

    OM = shafa.OUTSIDE_MODULE
    assert call(b=None) == OM
    assert call(src=None) == OM
    assert call(o=None) == OM
    assert call(c=None) == OM
    assert call(src_n=None) == OM
    assert call(dst=None) == OM
    assert call(dst_n=None) == OM
    assert call(n=0) == OM and call(n=-3) == OM
    assert call(framing=2) == OM and call(framing=-1) == OM
    assert call(o=(C.c_uint64 * 2)(0, 8)) == OM                       # h_src_off[1] % 16 != 0
    assert call(o=(C.c_uint64 * 2)(1, 16)) == OM
    assert call(src=C.c_void_p(p.value + 4)) == OM                     # d_src itself not 16-aligned


@pytest.mark.parametrize("which", ["pack_cod", "pack_freq"])
def test_text_argument_errors_are_refused_without_hip(shafa, which):
    L, A = shafa.lib(), _Args()
    p = A.p
    fn = getattr(L, "shafa_hipd_" + which)

    def call(b=p, n=1, mode=b"R", sizes=p, data=p, dst=p, dst_n=p):
        return fn(b, None, n, C.c_char(mode), sizes, data, dst, 1 << 20, dst_n)

    OM = shafa.OUTSIDE_MODULE
    assert call(b=None) == OM
    assert call(sizes=None) == OM
    assert call(data=None) == OM
    assert call(dst=None) == OM
    assert call(dst_n=None) == OM
    assert call(n=0) == OM and call(n=-1) == OM
    for mode in (b"r", b"n", b"X", b"\0", b"@"):
        assert call(mode=mode) == OM, mode

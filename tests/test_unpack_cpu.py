"""CPU-side checks of the file parsers (shafa_hipd_unpack_cod / _unpack_rle_freq / _unpack_shaf / _unpack_payloads,
csrc/unpack.hip): declared, exported, bound in Python, the ABI version unchanged, and every argument error refused before
HIP is touched (no GPU needed)."""
import ctypes as C
import os

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["shafa_hipd_unpack_cod", "shafa_hipd_unpack_rle_freq", "shafa_hipd_unpack_shaf", "shafa_hipd_unpack_payloads"]


def test_declared_and_exported(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    L = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared and hasattr(L, name), name


def test_abi_version_is_still_8(shafa):
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_python_bindings_exist(shafa):
    for m in ("unpack_cod", "unpack_rle_freq", "unpack_shaf", "unpack_payloads"):
        assert callable(getattr(shafa.Batch, m, None)), m
    assert callable(getattr(shafa, "decompress_files", None))
    assert shafa.UNPACK_INFO_WORDS == 8
    assert shafa.unpack_max_blocks(257, "cod") == 1 and shafa.unpack_max_blocks(258, "cod") == 2
    assert shafa.unpack_max_blocks(3, "freq") == 1 and shafa.unpack_max_blocks(4, "freq") == 2


class _Args:
    """stand-ins for device pointers (a refused call reads none of them), aligned to 16 bytes; as a batch it reads as one
    of max_blocks 0 (zeroed memory), so any block count exceeds it"""

    def __init__(self):
        self.raw = C.create_string_buffer(512)
        a = C.addressof(self.raw)
        self.p = C.c_void_p((a + 15) // 16 * 16)


OM, LM = 1, 2      # SHAFA_OUTSIDE_MODULE, SHAFA_LACK_OF_MEMORY


def test_unpack_cod_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, mb=1, f=p, n=16, info=p, sizes=p, tabs=p):
        return L.shafa_hipd_unpack_cod(b, None, mb, f, n, info, sizes, tabs)

    assert call(b=None) == OM
    assert call(mb=0) == OM and call(mb=-2) == OM
    assert call(f=None) == OM                               # NULL file with n > 0
    assert call(info=None) == OM and call(sizes=None) == OM and call(tabs=None) == OM
    assert call(mb=1) == LM and call(mb=7) == LM            # more blocks than the batch holds


def test_unpack_rle_freq_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, mb=1, f=p, n=16, rle_n=100, info=p, off=p, sz=p):
        return L.shafa_hipd_unpack_rle_freq(b, None, mb, f, n, rle_n, info, off, sz)

    assert call(b=None) == OM
    assert call(mb=0) == OM
    assert call(f=None) == OM
    assert call(info=None) == OM and call(off=None) == OM and call(sz=None) == OM
    assert call(mb=3) == LM


def test_unpack_shaf_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, mb=1, f=p, n=16, cnt=p, off=p, sz=p):
        return L.shafa_hipd_unpack_shaf(b, None, mb, f, n, cnt, off, sz)

    assert call(b=None) == OM
    assert call(mb=0) == OM and call(mb=-1) == OM
    assert call(f=None) == OM
    assert call(cnt=None) == OM and call(off=None) == OM and call(sz=None) == OM
    assert call(mb=2) == LM


def test_unpack_payloads_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p
    off, cap = (C.c_uint64 * 2)(0, 16), (C.c_uint64 * 2)(16, 16)

    def call(b=p, nb=2, f=p, n=64, d_off=p, d_n=p, dst=p, o=off, c=cap):
        return L.shafa_hipd_unpack_payloads(b, None, nb, f, n, d_off, d_n, dst, o, c)

    assert call(b=None) == OM
    assert call(nb=0) == OM and call(nb=-4) == OM
    assert call(f=None) == OM
    assert call(d_off=None) == OM and call(d_n=None) == OM and call(dst=None) == OM
    assert call(o=None) == OM and call(c=None) == OM
    assert call(o=(C.c_uint64 * 2)(0, 8)) == OM             # h_dst_off[1] % 16 != 0
    assert call(dst=C.c_void_p(p.value + 4)) == OM          # d_dst itself not 16-aligned
    assert call() == LM                                     # nblocks > the batch's max_blocks

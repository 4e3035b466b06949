"""CPU-side checks of shafa_hipd_sf_decode_dev and shafa_hipd_rle_decode_dev (Module D from device-resident tables and
sizes): declared, exported, bound in Python, and refusing NULL arguments before they touch HIP (no GPU needed)."""
import ctypes as C
import os

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shafa_hipd_sf_decode_dev", "shafa_hipd_rle_decode_dev")


def test_declared_and_exported(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    for name in NAMES:
        assert name in declared
        assert hasattr(C.CDLL(shafa.LIB_PATH), name)
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_batch_methods_exist(shafa):
    assert callable(getattr(shafa.Batch, "sf_decode_dev", None))
    assert callable(getattr(shafa.Batch, "rle_decode_dev", None))


def test_null_arguments_are_refused_without_hip(shafa):
    L = shafa.lib()
    off = (C.c_uint64 * 1)(0)
    cap = (C.c_uint64 * 1)(16)
    scratch = C.create_string_buffer(64)          # stands in for device pointers: a refused call reads none of them
    p = C.cast(scratch, C.c_void_p)

    def sf(batch, d_in_n, d_tables, d_nsym):
        return L.shafa_hipd_sf_decode_dev(batch, None, 1, p, off, cap, d_in_n, d_tables, d_nsym, p, off, cap)

    assert sf(None, p, p, p) == shafa.OUTSIDE_MODULE
    assert sf(p, None, p, p) == shafa.OUTSIDE_MODULE
    assert sf(p, p, None, p) == shafa.OUTSIDE_MODULE
    assert sf(p, p, p, None) == shafa.OUTSIDE_MODULE
    assert sf(None, None, None, None) == shafa.OUTSIDE_MODULE

    def rle(batch, d_in_n):
        return L.shafa_hipd_rle_decode_dev(batch, None, 1, p, off, cap, d_in_n, p, off, cap, p)

    assert rle(None, p) == shafa.OUTSIDE_MODULE
    assert rle(p, None) == shafa.OUTSIDE_MODULE

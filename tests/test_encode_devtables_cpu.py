"""CPU-side checks of shafa_hipd_sf_encode_dev (Module C from device-resident tables and block sizes): declared, exported,
bound in Python, and refusing NULL arguments before it touches HIP (no GPU needed)."""
import ctypes as C
import os

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported(shafa):
    assert "shafa_hipd_sf_encode_dev" in declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    assert hasattr(C.CDLL(shafa.LIB_PATH), "shafa_hipd_sf_encode_dev")
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_batch_method_exists(shafa):
    assert callable(getattr(shafa.Batch, "sf_encode_dev", None))


def test_null_arguments_are_refused_without_hip(shafa):
    L = shafa.lib()
    off = (C.c_uint64 * 1)(0)
    cap = (C.c_uint64 * 1)(16)
    scratch = C.create_string_buffer(64)          # stands in for device pointers: a refused call reads none of them
    p = C.cast(scratch, C.c_void_p)

    def call(batch, d_in_n, d_tables):
        return L.shafa_hipd_sf_encode_dev(batch, None, 1, p, off, cap, d_in_n, d_tables, None, None, p, off, cap, p)

    assert call(None, p, p) == shafa.OUTSIDE_MODULE
    assert call(p, None, p) == shafa.OUTSIDE_MODULE
    assert call(p, p, None) == shafa.OUTSIDE_MODULE
    assert call(None, None, None) == shafa.OUTSIDE_MODULE

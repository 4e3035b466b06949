"""CPU-side checks of Modules T and C on files in device memory (shafa_hipd_unpack_freq, csrc/unpack.hip; shafa.build_cod /
shafa.encode_files): declared, exported, bound in Python, the ABI version unchanged, and every argument error refused before
HIP or the device is touched (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_abi_cpu import declared_symbols
from test_unpack_cpu import LM, OM, _Args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    L = C.CDLL(shafa.LIB_PATH)
    assert "shafa_hipd_unpack_freq" in declared and hasattr(L, "shafa_hipd_unpack_freq")


def test_abi_version_is_still_8(shafa):
    assert shafa.lib().shafa_hip_abi_version() == 8


def test_python_bindings_exist(shafa):
    assert callable(getattr(shafa.Batch, "unpack_freq", None))
    assert callable(getattr(shafa, "build_cod", None)) and callable(getattr(shafa, "encode_files", None))
    # a block whose counts parse takes "@d@", a digit and 255 ';'
    assert shafa.unpack_max_blocks(258, "counts") == 1 and shafa.unpack_max_blocks(259, "counts") == 2


def test_unpack_freq_argument_errors(shafa):
    L, A = shafa.lib(), _Args()
    p = A.p

    def call(b=p, mb=1, f=p, n=16, info=p, sizes=p, counts=p):
        return L.shafa_hipd_unpack_freq(b, None, mb, f, n, info, sizes, counts)

    assert call(b=None) == OM
    assert call(mb=0) == OM and call(mb=-3) == OM
    assert call(f=None) == OM                               # NULL text with freq_n > 0
    assert call(info=None) == OM and call(sizes=None) == OM and call(counts=None) == OM
    assert call(mb=1) == LM and call(mb=9) == LM            # more blocks than the batch holds
    assert call(f=None, n=0) == LM                          # a NULL text of 0 bytes is no argument error


def test_build_cod_and_encode_files_check_their_arguments(shafa):
    import torch
    ok = torch.zeros(8, dtype=torch.uint8)                  # right type, wrong place: a CPU tensor
    bad = [b"@N@0", np.zeros(4, dtype=np.uint8), None, torch.zeros(8, dtype=torch.int32), ok, ok[::2]]
    for x in bad:
        with pytest.raises(ValueError):
            shafa.build_cod(x)
        with pytest.raises(ValueError):
            shafa.encode_files(x, ok)
        with pytest.raises(ValueError):
            shafa.encode_files(ok, x)

"""CPU-side checks of the compare pass (shafa_hipd_compare_dev, csrc/compare.hip) and of shafa.verify_files: declared,
exported, bound in Python, the ABI version unchanged, every argument error refused before HIP is touched, and verify_files'
ValueErrors on file arguments it cannot take (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "shafa_hipd_compare_dev"


def test_declared_exported_and_bound(shafa):
    assert NAME in declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    assert hasattr(C.CDLL(shafa.LIB_PATH), NAME)
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "compare_dev", None))
    assert callable(getattr(shafa, "verify_files", None))
    assert shafa.Verify._fields == ("equal", "first_diff", "decoded_size")


class _Args:
    """stand-ins for the batch and the device pointers (tests/test_rle_measure_cpu.py): the batch's bytes are 0x7F, so its
    max_blocks is 0x7F7F7F7F; a call that gets past every check reaches HIP, which refuses the stand-in batch (it names no
    device) before anything is enqueued."""

    def __init__(self):
        self.raw = C.create_string_buffer(b"\x7f" * 512, 512)
        a = C.addressof(self.raw)
        self.p = C.c_void_p((a + 15) // 16 * 16)
        self.odd = C.c_void_p(self.p.value + 5)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


def test_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM, LM = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY

    def call(**kw):
        a = dict(b=A.p, nb=3, d_a=A.p, a_off=_u64(0, 16, 4096), a_cap=_u64(5, 100, 70000), d_a_n=A.p, d_ref=A.odd,
                 ref_off=_u64(0, 5, (1 << 40) + 3), ref_n=_u64(5, 99, 70001), d_first=A.p)
        a.update(kw)
        return L.shafa_hipd_compare_dev(a["b"], None, a["nb"], a["d_a"], a["a_off"], a["a_cap"], a["d_a_n"], a["d_ref"],
                                        a["ref_off"], a["ref_n"], a["d_first"])

    # every check passed (ref at an odd address and odd offsets is fine): HIP refuses the stand-in batch
    assert call() not in (shafa.SUCCESS, OM, LM)
    for k in ("b", "d_a", "d_a_n", "d_ref", "d_first", "a_off", "a_cap", "ref_off", "ref_n"):
        assert call(**{k: None}) == OM, k
    assert call(d_a=A.odd) == OM                                       # side a is a decoder's output: 16-aligned
    assert call(d_a=C.c_void_p(A.p.value + 8)) == OM
    for bad in (_u64(1, 16, 4096), _u64(0, 24, 4096), _u64(0, 16, 4103)):
        assert call(a_off=bad) == OM
    assert call(nb=0) == shafa.SUCCESS and call(nb=-4) == shafa.SUCCESS
    assert call(nb=0, a_off=None, a_cap=None, ref_off=None, ref_n=None) == shafa.SUCCESS    # nothing to compare or look at
    assert call(nb=0x7F7F7F7F + 1) == LM                               # past max_blocks: refused before an array is read
    assert call(nb=0x7FFFFFFF) == LM
    assert call(b=None, nb=0) == OM                                    # a NULL batch comes before nblocks
    # 2^31 tiles of 8 KiB or more in the capacities, in one block or in their sum; one tile fewer gets to HIP
    T = 8192
    assert call(a_cap=_u64(5, (1 << 31) * T, 7)) == LM
    assert call(a_cap=_u64(1 << 43, 1 << 43, (1 << 31) * T - (1 << 44))) == LM
    assert call(a_cap=_u64((1 << 64) - 1, 0, 0)) == LM
    assert call(a_cap=_u64(((1 << 31) - 3) * T, T + 1, 0)) not in (shafa.SUCCESS, OM, LM)
    assert call(a_cap=_u64(((1 << 31) - 3) * T, T + 1, 1)) == LM


def test_verify_files_refuses_bad_file_arguments(shafa):
    import torch
    cpu = torch.zeros(8, dtype=torch.uint8)
    for e in ({"shaf": cpu, "cod": cpu}, {"rle": cpu, "freq": cpu}, {"shaf": cpu}, {"cod": cpu, "rle": cpu, "freq": cpu}, {},
              {"shaf": cpu, "cod": cpu, "rle": cpu}, {"rle": cpu}):
        with pytest.raises(ValueError):
            shafa.verify_files(cpu, **e)

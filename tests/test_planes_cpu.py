"""CPU-side checks of the byte-plane transposes (shafa_hipd_split_planes_dev / shafa_hipd_merge_planes_dev, csrc/planes.hip) and
of the tensor drivers on top: declared, exported, bound in Python, the ABI version unchanged, every argument error refused
before HIP is touched and in the stated order, the cases just under each LACK_OF_MEMORY bound reaching HIP, and the drivers'
ValueErrors before a device is touched (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shafa_hipd_split_planes_dev", "shafa_hipd_merge_planes_dev")


def test_declared_exported_and_bound(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_dev", "merge_planes_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("split_planes", "merge_planes", "compress_tensors", "decompress_tensors", "plane_files"):
        assert callable(getattr(shafa, name, None)), name
    assert isinstance(shafa.CompressedTensor, type)
    assert shafa.CompressedTensor.__slots__ == ("dtype", "shape", "planes", "nbytes")
    assert shafa.PLANES_TILE == 8192 and shafa.PLANES_ELEM == (1, 2, 4, 8)
    with open(os.path.join(ROOT, "include", "shafa_hip.h")) as f:
        assert "#define SHAFA_PLANES_TILE 8192" in f.read()


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=2, d_el=A.odd, off=_u64(0, 5, (1 << 40) + 3), cap=_u64(5, 100, 70000), d_n=A.p, d_planes=A.p,
                 poff=_u64(0, 16, 32, 1 << 40, 4096, 4096 + 112))
        a.update(kw)
        if merge:
            return L.shafa_hipd_merge_planes_dev(a["b"], None, a["nb"], a["elem"], a["d_planes"], a["poff"], a["cap"], a["d_n"],
                                                 a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_dev(a["b"], None, a["nb"], a["elem"], a["d_el"], a["off"], a["cap"], a["d_n"],
                                             a["d_planes"], a["poff"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed (the element side at an odd address and odd 64-bit offsets): HIP refuses the stand-in batch
    assert reached_hip(call())
    for elem in (1, 2, 4, 8):
        assert reached_hip(call(elem=elem, poff=_u64(*[16 * i for i in range(3 * elem)]))), elem
    # 1. the device pointers and the element size, in front of nblocks
    for k in ("b", "d_el", "d_planes", "d_n"):
        assert call(**{k: None}) == OM, k
        assert call(**{k: None}, nb=0) == OM, k
        assert call(**{k: None}, nb=0x7FFFFFFF) == OM, k
    for elem in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    assert call(b=None, d_el=None, elem=3) == OM
    # 2. no block: success, the host arrays are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, poff=None) == OK
    assert call(nb=0, d_planes=C.c_void_p(A.p.value + 8)) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, poff=None) == LM
    # 4. the capacities: NULL, then elem * h_cap[b] or the sum past 64 bits, then 2^31 tiles or more; all in front of the other
    #    host arrays and of the alignment rule
    assert call(cap=None) == OM
    bad_poff = _u64(0, 16, 33, 48, 64, 80)
    for elem in (1, 2, 4, 8):
        kw = dict(elem=elem, poff=_u64(*[16 * i for i in range(3 * elem)]))
        if elem > 1:                                                       # elem * h_cap[b] = 2^64
            assert call(cap=_u64(5, (1 << 64) // elem, 7), **kw) == LM, elem
            assert call(cap=_u64(0, 0, (1 << 64) // elem + 1), **kw) == LM, elem
        assert call(cap=_u64((1 << 64) - 1, 0, 0), **kw) == LM, elem
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, elem
        assert call(cap=_u64(1 << 43, 1 << 43, (1 << 31) * T - (1 << 44)), **kw) == LM, elem
        assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1), **kw) == LM, elem
        # one tile fewer gets to HIP: 2^31 - 1 tiles, elem * 2^44 bytes at the most
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), elem
        assert reached_hip(call(cap=_u64(((1 << 31) - 1) * T, 0, 0), **kw)), elem
    assert call(cap=_u64(5, (1 << 31) * T, 7), poff=bad_poff) == LM        # in front of the alignment rule
    assert call(cap=_u64(5, (1 << 31) * T, 7), off=None, poff=None) == LM  # and of the other arrays
    # the sum of elem * h_cap[b] past 64 bits where no single block is: only with more tiles than 2^31, LM either way
    assert call(elem=8, cap=_u64(1 << 60, 1 << 60, 1 << 60), poff=_u64(*[16 * i for i in range(24)])) == LM
    # 5. the other host arrays and the plane side's alignment
    for k in ("off", "poff"):
        assert call(**{k: None}) == OM, k
    for d in (1, 4, 8, 15):
        assert call(d_planes=C.c_void_p(A.p.value + d)) == OM, d
    for i in range(6):
        for d in (1, 8, 15):
            v = [0, 16, 32, 1 << 40, 4096, 4096 + 112]
            v[i] += d
            assert call(poff=_u64(*v)) == OM, (i, d)
    # only the call's blocks are looked at: nblocks * elem plane offsets
    assert reached_hip(call(nb=2, poff=_u64(0, 16, 32, 48, 7, 9)))
    assert reached_hip(call(nb=1, elem=4, poff=_u64(0, 16, 32, 48, 7, 9)))
    assert call(nb=1, elem=8, poff=_u64(0, 16, 32, 48, 7, 9, 0, 0)) == OM


def test_drivers_refuse_bad_arguments(shafa):
    import torch
    cpu = torch.zeros(64, dtype=torch.float32)
    meta = torch.zeros(64, dtype=torch.complex128, device="meta")          # elements of 16 bytes; never reaches a device
    for bad in (None, b"abc", 5, "x", cpu, [cpu], [None], (cpu, cpu), {"a": cpu}, cpu.numpy()):
        with pytest.raises(ValueError):
            shafa.compress_tensors(bad)
    for bad in (None, b"abc", cpu, [cpu], cpu.numpy()):
        with pytest.raises(ValueError):
            shafa.split_planes(bad)
    # a non-contiguous tensor and an element size outside 1, 2, 4, 8 are refused before the device is looked at
    assert not cpu.view(8, 8).t().is_contiguous()
    for bad in (cpu.view(8, 8).t(), cpu[::2], meta):
        with pytest.raises(ValueError):
            shafa._plane_tensors("test", bad)
    with pytest.raises(ValueError):
        shafa._plane_tensors("test", [torch.zeros(4, device="meta"), torch.zeros(4)])       # two devices
    # block_size: what shafa_block_count's uint64_t cannot take; the tensors are looked at first
    for bs in (-1, 1 << 64, 1.5, "64", None, True):
        with pytest.raises(ValueError):
            shafa.compress_tensors([], block_size=bs)
    for bs in (0, 1, 512, 8 << 20, (1 << 64) - 1):
        assert shafa.compress_tensors([], block_size=bs) == []
    assert shafa.compress_tensors([]) == [] and shafa.decompress_tensors([]) == []
    # merge_planes: the planes, the dtype and the shape
    u8 = torch.zeros(4, 64, dtype=torch.uint8)
    for planes, dtype, shape in ((u8, torch.float32, (64,)), (None, torch.float32, (64,)), (u8, "float32", (64,)),
                                 (u8, torch.complex128, (16,)), (u8, torch.float32, 64), (u8, torch.float32, (-64,)),
                                 (u8.to(torch.int8), torch.float32, (64,))):
        with pytest.raises(ValueError):
            shafa.merge_planes(planes, dtype, shape)
    # decompress_tensors: items and their planes
    CT = shafa.CompressedTensor
    raw = torch.zeros(8, dtype=torch.uint8)
    for bad in (None, 5, [None], [cpu], {"a": 1}, CT(torch.float32, (8,), [raw] * 3, 24), CT(torch.complex128, (8,), [raw] * 16, 128),
                CT("float32", (8,), [raw] * 4, 32), CT(torch.int16, (8,), [raw, None], 16), CT(torch.int16, (8,), [raw, {}], 16),
                CT(torch.int16, (8,), [raw, {".shaf": raw}], 16), CT(torch.int16, (8,), [raw, {".shaf": raw, ".cod": b"@"}], 16),
                CT(torch.int16, (8,), [raw, raw], 16), CT(torch.int16, (8,), [raw.view(2, 4), raw], 16),
                CT(torch.int16, (8,), [raw.to(torch.int8), raw], 16)):
        with pytest.raises(ValueError):
            shafa.decompress_tensors(bad)
    ct = CT(torch.bfloat16, [2, 3], [raw, raw], 12)
    assert (ct.dtype, ct.shape, ct.nbytes) == (torch.bfloat16, (2, 3), 12) and len(ct.planes) == 2
    assert shafa.plane_files({".shaf": 1, ".cod": 2, ".freq": 3}) == dict(shaf=1, cod=2, decode_rle=False)
    assert shafa.plane_files({".rle": 0, ".rle.freq": 0, ".rle.shaf": 1, ".rle.cod": 2}) == dict(shaf=1, cod=2)

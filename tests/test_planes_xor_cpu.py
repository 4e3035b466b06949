"""CPU-side checks of the byte-plane transposes against a base (shafa_hipd_split_planes_xor_dev /
shafa_hipd_merge_planes_xor_dev, csrc/planes.hip) and of the delta drivers on top: declared, exported, bound in Python, the ABI
version and CompressedTensor unchanged, every argument error refused before HIP is touched and in the plain entries' order with
the base side's two checks in their groups, and the drivers' ValueErrors before a device is touched (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shafa_hipd_split_planes_xor_dev", "shafa_hipd_merge_planes_xor_dev")
NO_BASE = (1 << 64) - 1


def test_declared_exported_and_bound(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_xor_dev", "merge_planes_xor_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("compress_deltas", "decompress_deltas"):
        assert callable(getattr(shafa, name, None)), name
    assert isinstance(shafa.CompressedDelta, type) and issubclass(shafa.CompressedDelta, shafa.CompressedTensor)
    assert shafa.CompressedDelta.__slots__ == ("base_crc",)
    assert shafa.CompressedTensor.__slots__ == ("dtype", "shape", "planes", "nbytes")
    assert shafa.PLANES_NO_BASE == NO_BASE
    with open(os.path.join(ROOT, "include", "shafa_hip.h")) as f:
        assert "#define SHAFA_PLANES_NO_BASE UINT64_MAX" in f.read()


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=2, d_el=A.odd, off=_u64(0, 5, (1 << 40) + 3), d_base=C.c_void_p(A.p.value + 3),
                 boff=_u64(7, (1 << 41) + 1, 0), cap=_u64(5, 100, 70000), d_n=A.p, d_planes=A.p,
                 poff=_u64(0, 16, 32, 1 << 40, 4096, 4096 + 112))
        a.update(kw)
        if merge:
            return L.shafa_hipd_merge_planes_xor_dev(a["b"], None, a["nb"], a["elem"], a["d_planes"], a["poff"], a["d_base"],
                                                     a["boff"], a["cap"], a["d_n"], a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_xor_dev(a["b"], None, a["nb"], a["elem"], a["d_el"], a["off"], a["d_base"], a["boff"],
                                                 a["cap"], a["d_n"], a["d_planes"], a["poff"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed (both sides at odd addresses and odd 64-bit offsets): HIP refuses the stand-in batch
    assert reached_hip(call())
    for elem in (1, 2, 4, 8):
        assert reached_hip(call(elem=elem, poff=_u64(*[16 * i for i in range(3 * elem)]))), elem
    # the base side needs no alignment, in the address or in the offsets, whatever the element side's; a block without a base
    for d in (0, 1, 4, 8, 15):
        assert reached_hip(call(d_base=C.c_void_p(A.p.value + d))), d
        assert reached_hip(call(d_base=C.c_void_p(A.p.value + d), d_el=A.p, off=_u64(0, 16, 4096))), d
    assert reached_hip(call(boff=_u64(1, 3, 15)))
    assert reached_hip(call(boff=_u64(NO_BASE, 3, NO_BASE)))
    assert reached_hip(call(boff=_u64(NO_BASE, NO_BASE, NO_BASE)))
    # 1. the device pointers, d_base among them, and the element size, in front of nblocks
    for k in ("b", "d_el", "d_planes", "d_n", "d_base"):
        assert call(**{k: None}) == OM, k
        assert call(**{k: None}, nb=0) == OM, k
        assert call(**{k: None}, nb=-1) == OM, k
        assert call(**{k: None}, nb=0x7FFFFFFF) == OM, k
    for elem in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    assert call(b=None, d_base=None, elem=3) == OM
    # 2. no block: success, the host arrays are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, boff=None, cap=None, poff=None) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, boff=None, cap=None, poff=None) == LM
    # 4. the capacities, in front of the other host arrays (h_base_off among them) and of the alignment rule
    assert call(cap=None) == OM
    assert call(cap=None, boff=None) == OM
    for elem in (1, 2, 4, 8):
        kw = dict(elem=elem, poff=_u64(*[16 * i for i in range(3 * elem)]))
        if elem > 1:
            assert call(cap=_u64(5, (1 << 64) // elem, 7), **kw) == LM, elem
        assert call(cap=_u64((1 << 64) - 1, 0, 0), **kw) == LM, elem
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, elem
        assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1), **kw) == LM, elem
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), elem
    assert call(cap=_u64(5, (1 << 31) * T, 7), boff=None) == LM            # LACK_OF_MEMORY in front of a NULL h_base_off
    assert call(cap=_u64(5, (1 << 31) * T, 7), off=None, boff=None, poff=None) == LM
    # 5. the other host arrays, h_base_off among them, and the plane side's alignment
    for k in ("off", "poff", "boff"):
        assert call(**{k: None}) == OM, k
    for d in (1, 4, 8, 15):
        assert call(d_planes=C.c_void_p(A.p.value + d)) == OM, d
    for i in range(6):
        v = [0, 16, 32, 1 << 40, 4096, 4096 + 112]
        v[i] += 8
        assert call(poff=_u64(*v)) == OM, i
    # only the call's blocks are looked at
    assert reached_hip(call(nb=2, poff=_u64(0, 16, 32, 48, 7, 9), boff=_u64(0, 1)))


def test_drivers_refuse_bad_arguments(shafa):
    import torch
    CT, CD = shafa.CompressedTensor, shafa.CompressedDelta
    cpu = torch.zeros(64, dtype=torch.float32)
    m32 = torch.zeros(64, dtype=torch.float32, device="meta")              # never reaches a device
    m16 = torch.zeros(64, dtype=torch.bfloat16, device="meta")
    # compress_deltas: the tensors are compress_tensors', and looked at first
    for bad in (None, b"abc", 5, cpu, [cpu], [None]):
        with pytest.raises(ValueError):
            shafa.compress_deltas(bad, [None])
    assert shafa.compress_deltas([], []) == []
    assert shafa.compress_deltas([], [], check_base=False) == []
    for bad in (None, [None], 5, "x", [cpu]):
        with pytest.raises(ValueError):
            shafa.compress_deltas([], bad)
    for bs in (-1, 1 << 64, 1.5, None, True):
        with pytest.raises(ValueError):
            shafa.compress_deltas([], [], block_size=bs)
    with pytest.raises(ValueError):
        shafa.compress_deltas([], [], check_base=1)
    # the bases: one per tensor, None or a contiguous CUDA tensor of the tensor's dtype and numel on its device
    metas = [(torch.float32, 64, m32.device), (torch.bfloat16, 64, m32.device)]
    assert shafa._base_tensors("test", [None, None], metas) == [None, None]
    for bad in (None, [], [None], [None, None, None], [cpu, None], [None, cpu.to(torch.bfloat16)], [m16, None], [None, m32],
                [m32[:63], None], [m32.view(8, 8).t(), None], [5, None], ["x", None]):
        with pytest.raises(ValueError):
            shafa._base_tensors("test", bad, metas)
    # decompress_deltas: the items, then the bases against them
    raw = torch.zeros(8, dtype=torch.uint8)
    plain = CT(torch.int16, (8,), [raw, raw], 16)
    delta = CD(torch.int16, (8,), [raw, raw], 16, 0x1234)
    assert delta.base_crc == 0x1234 and CD(torch.int16, (8,), [raw, raw], 16).base_crc is None
    assert (delta.dtype, delta.shape, delta.nbytes) == (torch.int16, (8,), 16) and len(delta.planes) == 2
    assert "CompressedDelta" in repr(delta) and "0x00001234" in repr(delta)
    assert shafa.decompress_deltas([], []) == []
    for items, bases in ((None, []), ([None], [None]), (5, [None]), ([cpu], [None]), ([plain], []), ([plain], [None, None]),
                         ([plain, delta], [None]), ([plain], 5), ([CT(torch.int16, (8,), [raw], 8)], [None])):
        with pytest.raises(ValueError):
            shafa.decompress_deltas(items, bases)
    i16 = torch.zeros(8, dtype=torch.int16, device="meta")
    for items, bases, why in (([delta], [None], "item 0 is a CompressedDelta and needs its base"),
                              (delta, None, "needs its base"),
                              ([plain, delta], [None, None], "item 1 is a CompressedDelta and needs its base"),
                              ([plain], [i16], "item 0 is a plain CompressedTensor and takes no base"),
                              (plain, i16, "takes no base"),
                              ([delta, plain], [i16, i16], "item 1 is a plain"),
                              ([delta], [i16.to(torch.float16)], "base 0 is torch.float16 x 8"),
                              ([delta], [torch.zeros(9, dtype=torch.int16, device="meta")], "base 0 is torch.int16 x 9"),
                              ([delta], [torch.zeros(8, dtype=torch.int16)], "base 0 is None or a contiguous CUDA tensor"),
                              ([delta], [5], "base 0 is None or a contiguous CUDA tensor")):
        with pytest.raises(ValueError, match=why):
            shafa.decompress_deltas(items, bases)
    with pytest.raises(ValueError):
        shafa.decompress_deltas([], [], check_base=None)
    # decompress_tensors does not hand out the XOR
    with pytest.raises(ValueError, match="decompress_deltas"):
        shafa.decompress_tensors(delta)
    with pytest.raises(ValueError, match="decompress_deltas"):
        shafa.decompress_tensors([plain, delta])

"""CPU-side checks of the byte-plane transposes of differences (shafa_hipd_split_planes_diff_dev /
shafa_hipd_merge_planes_diff_dev, csrc/planes.hip) and of the sequence drivers on top: declared, exported, bound in Python, the
ABI version and the three __slots__, every argument error of the plain entries refused before HIP is touched and in the plain
entries' order, the cases that pass every check, and the drivers' ValueErrors before a device is touched (no GPU needed)."""
import ctypes as C
import os

import pytest

from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shafa_hipd_split_planes_diff_dev", "shafa_hipd_merge_planes_diff_dev")


def test_declared_exported_and_bound(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_planes_diff_dev", "merge_planes_diff_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("compress_sequences", "decompress_sequences"):
        assert callable(getattr(shafa, name, None)), name
    assert isinstance(shafa.CompressedSequence, type) and issubclass(shafa.CompressedSequence, shafa.CompressedTensor)
    assert not issubclass(shafa.CompressedSequence, shafa.CompressedDelta)
    assert shafa.CompressedSequence.__slots__ == ()
    assert shafa.CompressedDelta.__slots__ == ("base_crc",)
    assert shafa.CompressedTensor.__slots__ == ("dtype", "shape", "planes", "nbytes")
    with open(os.path.join(ROOT, "include", "shafa_hip.h")) as f:
        assert "Byte planes of differences" in f.read()


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    """the plain entries' checks in the plain entries' order (tests/test_planes_cpu.py), on the stand-in batch"""
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.PLANES_TILE

    def call(**kw):
        a = dict(b=A.p, nb=3, elem=2, d_el=A.odd, off=_u64(0, 5, (1 << 40) + 3), cap=_u64(5, 100, 70000), d_n=A.p, d_planes=A.p,
                 poff=_u64(0, 16, 32, 1 << 40, 4096, 4096 + 112))
        a.update(kw)
        if merge:
            return L.shafa_hipd_merge_planes_diff_dev(a["b"], None, a["nb"], a["elem"], a["d_planes"], a["poff"], a["cap"],
                                                      a["d_n"], a["d_el"], a["off"])
        return L.shafa_hipd_split_planes_diff_dev(a["b"], None, a["nb"], a["elem"], a["d_el"], a["off"], a["cap"], a["d_n"],
                                                  a["d_planes"], a["poff"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed (the element side at an odd address and odd 64-bit offsets): HIP refuses the stand-in batch
    assert reached_hip(call())
    for elem in (1, 2, 4, 8):
        assert reached_hip(call(elem=elem, poff=_u64(*[16 * i for i in range(3 * elem)]))), elem
    # the element side needs no alignment, in the address or in the offsets
    for d in (0, 1, 4, 8, 15):
        assert reached_hip(call(d_el=C.c_void_p(A.p.value + d))), d
        assert reached_hip(call(d_el=C.c_void_p(A.p.value + d), off=_u64(1, 3, 15))), d
    # 1. the device pointers and the element size, in front of nblocks
    for k in ("b", "d_el", "d_planes", "d_n"):
        assert call(**{k: None}) == OM, k
        assert call(**{k: None}, nb=0) == OM, k
        assert call(**{k: None}, nb=-1) == OM, k
        assert call(**{k: None}, nb=0x7FFFFFFF) == OM, k
    for elem in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert call(elem=elem) == OM and call(elem=elem, nb=0) == OM and call(elem=elem, nb=0x7FFFFFFF) == OM, elem
    assert call(b=None, elem=3) == OM
    # 2. no block: success, the host arrays are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, poff=None) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, poff=None) == LM
    # 4. the capacities, in front of the other host arrays and of the alignment rule
    assert call(cap=None) == OM
    assert call(cap=None, off=None, poff=None) == OM
    for elem in (1, 2, 4, 8):
        kw = dict(elem=elem, poff=_u64(*[16 * i for i in range(3 * elem)]))
        if elem > 1:
            assert call(cap=_u64(5, (1 << 64) // elem, 7), **kw) == LM, elem
        assert call(cap=_u64((1 << 64) - 1, 0, 0), **kw) == LM, elem
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, elem
        assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1), **kw) == LM, elem
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), elem
    assert call(cap=_u64(5, (1 << 31) * T, 7), off=None, poff=None) == LM     # LACK_OF_MEMORY in front of a NULL host array
    assert call(cap=_u64(5, (1 << 31) * T, 7), d_planes=C.c_void_p(A.p.value + 8)) == LM
    # 5. the other host arrays and the plane side's alignment
    for k in ("off", "poff"):
        assert call(**{k: None}) == OM, k
    for d in (1, 4, 8, 15):
        assert call(d_planes=C.c_void_p(A.p.value + d)) == OM, d
    for i in range(6):
        v = [0, 16, 32, 1 << 40, 4096, 4096 + 112]
        v[i] += 8
        assert call(poff=_u64(*v)) == OM, i
    # only the call's blocks are looked at
    assert reached_hip(call(nb=2, poff=_u64(0, 16, 32, 48, 7, 9)))


def test_drivers_refuse_bad_arguments(shafa):
    import torch
    CT, CD, CS = shafa.CompressedTensor, shafa.CompressedDelta, shafa.CompressedSequence
    cpu = torch.zeros(64, dtype=torch.float32)
    # compress_sequences: compress_tensors' argument errors, message for message but for the name in front
    for bad in (None, b"abc", 5, cpu, [cpu], [None], [torch.zeros(4, dtype=torch.complex64, device="meta")]):
        with pytest.raises(ValueError) as mine:
            shafa.compress_sequences(bad)
        with pytest.raises(ValueError) as theirs:
            shafa.compress_tensors(bad)
        assert str(mine.value) == str(theirs.value).replace("compress_tensors", "compress_sequences"), bad
        assert str(mine.value).startswith("compress_sequences: ")
    assert shafa.compress_sequences([]) == []
    for bs in (-1, 1 << 64, 1.5, None, True):
        with pytest.raises(ValueError, match="compress_sequences: block_size"):
            shafa.compress_sequences([], block_size=bs)
    # the item
    raw = torch.zeros(8, dtype=torch.uint8)
    plain = CT(torch.int16, (8,), [raw, raw], 16)
    delta = CD(torch.int16, (8,), [raw, raw], 16, 0x1234)
    seq = CS(torch.int16, (2, 4), [raw, raw], 16)
    assert (seq.dtype, seq.shape, seq.nbytes) == (torch.int16, (2, 4), 16) and len(seq.planes) == 2
    assert repr(seq).startswith("CompressedSequence(torch.int16, (2, 4), planes=['raw', 'raw']")
    assert not hasattr(seq, "__dict__")
    # decompress_sequences: its own items only
    assert shafa.decompress_sequences([]) == []
    for bad in (None, 5, cpu, [cpu], [None], plain, [plain], delta, [seq, plain], [delta, seq]):
        with pytest.raises(ValueError, match="decompress_sequences: a CompressedSequence or a list of them"):
            shafa.decompress_sequences(bad)
    # malformed items: decompress_tensors' checks under this driver's name, before any device work
    with pytest.raises(ValueError, match="decompress_sequences: torch.int16 has 2 planes"):
        shafa.decompress_sequences(CS(torch.int16, (8,), [raw], 8))
    with pytest.raises(ValueError, match="decompress_sequences: planes are CUDA tensors"):
        shafa.decompress_sequences([seq])
    with pytest.raises(ValueError, match="decompress_sequences: negative dimension"):
        shafa.decompress_sequences(CS(torch.int16, (-8,), [raw, raw], 16))
    # the other two decoders do not hand out differences
    i16 = torch.zeros(8, dtype=torch.int16, device="meta")
    for items in (seq, [seq], [plain, seq]):
        with pytest.raises(ValueError, match="decompress_tensors: a CompressedSequence .*decompress_sequences"):
            shafa.decompress_tensors(items)
    for items, bases in ((seq, None), ([seq], [None]), ([seq], [i16]), ([delta, seq], [i16, None])):
        with pytest.raises(ValueError, match="decompress_deltas: a CompressedSequence .*decompress_sequences"):
            shafa.decompress_deltas(items, bases)

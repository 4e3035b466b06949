"""CPU-side checks of the record transposes (shafa_hipd_split_records_dev / shafa_hipd_merge_records_dev, csrc/records.hip) and of
the drivers on top (shafa-cd_amd/records.py): declared, exported, bound in Python, the ABI version unchanged, every argument
error refused before HIP is touched and in the stated order, the case one tile under the 2^31 bound reaching HIP, records_pass
equal to the header's macro, and the drivers' ValueErrors before a device is touched (no GPU needed)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import pkgload
from test_abi_cpu import declared_symbols
from test_compare_cpu import _Args, _u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shafa_hip.h")
NAMES = ("shafa_hipd_split_records_dev", "shafa_hipd_merge_records_dev")


@pytest.fixture(scope="module")
def records(shafa):
    return pkgload.load_submodule("records")


def test_declared_exported_and_bound(shafa, records):
    declared = declared_symbols(HEADER)
    dll = C.CDLL(shafa.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(dll, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    for name in ("split_records_dev", "merge_records_dev"):
        assert callable(getattr(shafa.Batch, name, None)), name
    for name in ("records_pass", "split_records", "merge_records", "compress_records", "decompress_records"):
        assert callable(getattr(records, name, None)), name
        assert getattr(shafa, name) is getattr(records, name), name        # re-exported, and the submodule's own
        assert getattr(records, name).__module__ == records.__name__
    assert isinstance(records.CompressedRecords, type) and shafa.CompressedRecords is records.CompressedRecords
    assert records.CompressedRecords.__slots__ == ("dtype", "shape", "width", "planes", "nbytes")
    assert not issubclass(records.CompressedRecords, shafa.CompressedTensor)
    assert shafa.RECORDS_MAX_WIDTH == 64 and shafa.RECORDS_TILE == 8192 == shafa.PLANES_TILE
    with open(HEADER) as f:
        text = f.read()
    assert "#define SHAFA_RECORDS_MAX_WIDTH 64" in text and "#define SHAFA_RECORDS_TILE 8192" in text
    # the plain entries' refusal of other element sizes is as it was
    assert shafa.PLANES_ELEM == (1, 2, 4, 8)


@pytest.mark.parametrize("merge", [False, True], ids=["split", "merge"])
def test_argument_errors_before_hip(shafa, merge):
    L = shafa.lib()
    A = _Args()
    OM, LM, OK = shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.SUCCESS
    T = shafa.RECORDS_TILE

    def poffs(nb, w):
        return _u64(*[16 * i for i in range(nb * w)])

    def call(**kw):
        a = dict(b=A.p, nb=3, width=2, d_rec=A.odd, off=_u64(0, 5, (1 << 40) + 3), cap=_u64(5, 100, 70000), d_n=A.p, d_planes=A.p,
                 poff=_u64(0, 16, 32, 1 << 40, 4096, 4096 + 112))
        a.update(kw)
        if merge:
            return L.shafa_hipd_merge_records_dev(a["b"], None, a["nb"], a["width"], a["d_planes"], a["poff"], a["cap"], a["d_n"],
                                                  a["d_rec"], a["off"])
        return L.shafa_hipd_split_records_dev(a["b"], None, a["nb"], a["width"], a["d_rec"], a["off"], a["cap"], a["d_n"],
                                              a["d_planes"], a["poff"])

    reached_hip = lambda rc: rc not in (OK, OM, LM)
    # every check passed (the record side at an odd address and odd 64-bit offsets): HIP refuses the stand-in batch
    assert reached_hip(call())
    for w in (1, 2, 3, 4, 5, 7, 8, 12, 16, 17, 33, 63, 64):
        assert reached_hip(call(width=w, poff=poffs(3, w))), w
    # 1. the device pointers and the width, in front of nblocks
    for k in ("b", "d_rec", "d_planes", "d_n"):
        assert call(**{k: None}) == OM, k
        assert call(**{k: None}, nb=0) == OM, k
        assert call(**{k: None}, nb=0x7FFFFFFF) == OM, k
    for w in (0, 65, 66, 128, 256, 0x80000000, 0xFFFFFFFF):
        assert call(width=w) == OM and call(width=w, nb=0) == OM and call(width=w, nb=0x7FFFFFFF) == OM, w
    assert call(b=None, d_rec=None, width=0) == OM
    # 2. no block: success, the host arrays are not looked at
    assert call(nb=0) == OK and call(nb=-4) == OK
    assert call(nb=0, off=None, cap=None, poff=None) == OK
    assert call(nb=0, width=64, off=None, cap=None, poff=None) == OK
    assert call(nb=0, d_planes=C.c_void_p(A.p.value + 8)) == OK
    # 3. past max_blocks (the stand-in's is 0x7F7F7F7F): refused before an array is read
    assert call(nb=0x7F7F7F7F + 1) == LM and call(nb=0x7FFFFFFF) == LM
    assert call(nb=0x7FFFFFFF, off=None, cap=None, poff=None) == LM
    # 4. the capacities: NULL, then width * h_cap[b] or the sum past 64 bits, then 2^31 tiles or more; all in front of the other
    #    host arrays and of the alignment rule
    assert call(cap=None) == OM
    bad_poff = _u64(0, 16, 33, 48, 64, 80)
    for w in (1, 2, 3, 12, 64):
        kw = dict(width=w, poff=poffs(3, w))
        if w > 1:                                                          # width * h_cap[b] past 2^64
            assert call(cap=_u64(5, (1 << 64) // w + 1, 7), **kw) == LM, w
            assert call(cap=_u64(0, 0, ((1 << 64) - 1) // w + 1), **kw) == LM, w
        assert call(cap=_u64((1 << 64) - 1, 0, 0), **kw) == LM, w
        assert call(cap=_u64(5, (1 << 31) * T, 7), **kw) == LM, w
        assert call(cap=_u64(1 << 43, 1 << 43, (1 << 31) * T - (1 << 44)), **kw) == LM, w
        assert call(cap=_u64(((1 << 31) - 3) * T, T + 1, 1), **kw) == LM, w
        # one tile fewer gets to HIP: 2^31 - 1 tiles of RECORDS_TILE records
        assert reached_hip(call(cap=_u64(((1 << 31) - 3) * T, T + 1, 0), **kw)), w
        assert reached_hip(call(cap=_u64(((1 << 31) - 1) * T, 0, 0), **kw)), w
    assert call(cap=_u64(5, (1 << 31) * T, 7), poff=bad_poff) == LM        # in front of the alignment rule
    assert call(cap=_u64(5, (1 << 31) * T, 7), off=None, poff=None) == LM  # and of the other arrays
    assert call(width=64, cap=_u64(1 << 57, 1 << 57, 1 << 58), poff=poffs(3, 64)) == LM    # the sum past 64 bits
    # 5. the other host arrays and the column side's alignment
    for k in ("off", "poff"):
        assert call(**{k: None}) == OM, k
    for d in (1, 4, 8, 15):
        assert call(d_planes=C.c_void_p(A.p.value + d)) == OM, d
    for i in range(6):
        for d in (1, 8, 15):
            v = [0, 16, 32, 1 << 40, 4096, 4096 + 112]
            v[i] += d
            assert call(poff=_u64(*v)) == OM, (i, d)
    for w in (3, 64):                                                      # every one of the nblocks * width offsets is looked at
        v = [16 * i for i in range(3 * w)]
        v[-1] += 8
        assert call(width=w, poff=_u64(*v)) == OM, w
    # only the call's blocks are looked at: nblocks * width column offsets
    assert reached_hip(call(nb=2, poff=_u64(0, 16, 32, 48, 7, 9)))
    assert reached_hip(call(nb=1, width=4, poff=_u64(0, 16, 32, 48, 7, 9)))
    assert reached_hip(call(nb=1, width=3, poff=_u64(0, 16, 32, 7, 7, 9)))
    assert call(nb=1, width=5, poff=_u64(0, 16, 32, 48, 7, 9)) == OM
    # the plain plane entries still refuse what the record entries take
    for w in (3, 12, 16, 64):
        assert L.shafa_hipd_split_planes_dev(A.p, None, 3, w, A.odd, _u64(0, 5, 9), _u64(5, 100, 70000), A.p, A.p, poffs(3, w)) == OM


def test_records_pass_is_the_headers(shafa, records, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the host library too"
    src = tmp_path / "pass.c"
    src.write_text('#include <stdio.h>\n#include "shafa_hip.h"\n'
                   'int main(void) { for (unsigned w = 1; w <= SHAFA_RECORDS_MAX_WIDTH; ++w) '
                   'printf("%u %u %u\\n", w, (unsigned)SHAFA_RECORDS_PASS(w), (unsigned)SHAFA_RECORDS_TILE); return 0; }\n')
    exe = tmp_path / "pass"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = [tuple(int(x) for x in l.split()) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                     text=True).stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(1, 65))
    for w, p, t in rows:
        assert t == shafa.RECORDS_TILE
        assert records.records_pass(w) == p, w
        assert p % 16 == 0 and 8192 % p == 0 and p * w <= 32768 and (p == 8192 or 2 * p * w > 32768), (w, p)
    for bad in (0, 65, -1, 1.0, "3", None, True):
        with pytest.raises(ValueError):
            records.records_pass(bad)


def test_drivers_refuse_bad_arguments_before_a_device(shafa, records, monkeypatch):
    import torch
    # any device work would need a stream or a batch: both refuse to be made here
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(64, 3, dtype=torch.uint8)
    meta = lambda *shape, dtype=torch.uint8: torch.zeros(*shape, dtype=dtype, device="meta")  # never reaches a device
    # not a tensor, a CPU tensor, a non-contiguous one
    for bad in (None, b"abc", 5, "x", [None], {"a": cpu}, cpu.numpy(), [cpu, None]):
        with pytest.raises(ValueError, match="compress_records: a tensor or a list of tensors"):
            records.compress_records(bad)
    for bad in (cpu, [cpu], (cpu, cpu), cpu.t(), cpu[::2], meta(64, 3), meta(8, 8).t()):
        with pytest.raises(ValueError, match="compress_records: contiguous CUDA tensors"):
            records.compress_records(bad)
    for bad in (None, b"abc", [cpu], cpu.numpy()):
        with pytest.raises(ValueError, match="split_records: a contiguous CUDA tensor"):
            records.split_records(bad)
    with pytest.raises(ValueError, match="split_records: contiguous CUDA tensors"):
        records.split_records(cpu)
    with pytest.raises(ValueError, match="one device"):
        records._record_tensors("test", [_FakeCuda(cpu, 0), _FakeCuda(cpu, 1)], None)
    # widths: outside 1 .. 64, of the wrong type, not dividing, of the wrong length — the default included
    for w in (0, 65, -3, 1 << 40, 2.0, "3", True, [3.0], [None, 3]):
        with pytest.raises(ValueError, match="width"):
            records.compress_records(meta(64, 3), widths=w)
    for t, w in ((meta(64, 3), 5), (meta(64, 3), 7), (meta(7, dtype=torch.complex128), 32), (meta(5, dtype=torch.float32), 8),
                 (meta(10, 3, dtype=torch.float32), 7)):
        with pytest.raises(ValueError, match="does not divide"):
            records.compress_records(t, widths=w)
    for t in (meta(4, 65), meta(4, 17, dtype=torch.float32), meta(2, 5, dtype=torch.complex128)):     # None: the last dimension
        with pytest.raises(ValueError, match="a width is an int of 1 .. 64"):
            records.compress_records(t)
    for w in ([], [3, 3], (3, 3, 3), {"a": 3}):
        with pytest.raises(ValueError, match="widths is None, an int or a list"):
            records.compress_records([meta(64, 3)], widths=w)
    # what None means: the bytes of the last dimension; the element for 0 and 1 dimensions and for an empty last dimension
    f = _FakeCuda
    got = records._record_tensors("test", [f(torch.zeros(9, 3, dtype=torch.uint8)), f(torch.zeros(9, 3)), f(torch.zeros(9)),
                                           f(torch.zeros((), dtype=torch.complex128)), f(torch.zeros(3, 0, dtype=torch.int16)),
                                           f(torch.zeros(2, 3, 5, dtype=torch.bfloat16)), f(torch.zeros(6, dtype=torch.bool))],
                                  None)[1]
    assert got == [3, 12, 4, 16, 2, 10, 1]
    assert records._record_tensors("test", [f(torch.zeros(96, dtype=torch.uint8))] * 3, [32, None, 1])[1] == [32, 1, 1]
    # block_size: what shafa_block_count's uint64_t cannot take; the tensors are looked at first
    for bs in (-1, 1 << 64, 1.5, "64", None, True):
        with pytest.raises(ValueError, match="block_size"):
            records.compress_records([], block_size=bs)
    for bs in (0, 1, 512, 8 << 20, (1 << 64) - 1):
        assert records.compress_records([], block_size=bs) == []
    assert records.compress_records([]) == [] and records.decompress_records([]) == []
    assert records.compress_records([], widths=3) == [] and records.compress_records([], widths=[]) == []
    # merge_records: the planes, the dtype and the shape
    u8 = torch.zeros(3, 64, dtype=torch.uint8)
    for planes, dtype, shape in ((None, torch.uint8, (64, 3)), (u8, "uint8", (64, 3)), (u8, torch.uint8, 192), (u8, torch.uint8, (-64, 3)),
                                 (u8.to(torch.int8), torch.uint8, (64, 3)), (u8[0], torch.uint8, (64,)), (u8, torch.uint8, (65, 3)),
                                 (u8, torch.float32, (16, 3)), (u8, torch.int16, (97,)), (torch.zeros(65, 4, dtype=torch.uint8), torch.uint8, (260,)),
                                 (torch.zeros(0, 4, dtype=torch.uint8), torch.uint8, (0,)), (u8, torch.uint8, (64, 3))):
        with pytest.raises(ValueError):
            records.merge_records(planes, dtype, shape)


class _FakeCuda:
    """a CPU tensor that says it is a contiguous CUDA tensor on device `index`: what _record_tensors looks at, and nothing a
    device is needed for"""

    def __new__(cls, t, index=0):
        import torch

        class T(torch.Tensor):
            is_cuda = True
            device = torch.device("cuda", index)

        return t.as_subclass(T)


def test_items_are_kept_apart(shafa, records, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    raw = torch.zeros(8, dtype=torch.uint8)
    CR, CT = records.CompressedRecords, shafa.CompressedTensor
    cr = CR(torch.uint8, [8, 3], 3, [raw] * 3, 24)
    assert (cr.dtype, cr.shape, cr.width, cr.nbytes) == (torch.uint8, (8, 3), 3, 24) and len(cr.planes) == 3
    assert "width=3" in repr(cr)
    # the three existing decompressors refuse a CompressedRecords with their present ValueError
    with pytest.raises(ValueError, match="decompress_tensors: a CompressedTensor or a list of them"):
        shafa.decompress_tensors(cr)
    with pytest.raises(ValueError, match="decompress_tensors: a CompressedTensor or a list of them"):
        shafa.decompress_tensors([cr])
    with pytest.raises(ValueError, match="decompress_deltas: a CompressedDelta / CompressedTensor or a list of them"):
        shafa.decompress_deltas([cr], [None])
    with pytest.raises(ValueError, match="decompress_sequences: a CompressedSequence or a list of them"):
        shafa.decompress_sequences([cr])
    # decompress_records refuses theirs, and malformed items of its own
    for bad in (CT(torch.int16, (8,), [raw, raw], 16), shafa.CompressedDelta(torch.int16, (8,), [raw, raw], 16),
                shafa.CompressedSequence(torch.int16, (8,), [raw, raw], 16), None, 5, [None], [raw], {"a": 1}):
        with pytest.raises(ValueError, match="decompress_records: a CompressedRecords or a list of them"):
            records.decompress_records(bad)
        if isinstance(bad, CT):
            with pytest.raises(ValueError, match="decompress_records: a CompressedRecords or a list of them"):
                records.decompress_records([cr, bad])
    for bad in (CR(torch.uint8, (8, 3), 3, [raw] * 2, 16), CR(torch.uint8, (8, 3), 0, [], 0), CR(torch.uint8, (8, 3), 65, [raw] * 65, 0),
                CR(torch.uint8, (8, 3), 5, [raw] * 5, 0), CR(torch.uint8, (8, 3), "3", [raw] * 3, 0), CR("uint8", (8, 3), 3, [raw] * 3, 0),
                CR(torch.uint8, (8, -3), 3, [raw] * 3, 0), CR(torch.uint8, (8, 3), 3, [raw, raw, None], 0),
                CR(torch.uint8, (8, 3), 3, [raw, raw, {}], 0), CR(torch.uint8, (8, 3), 3, [raw, raw, {".shaf": raw}], 0),
                CR(torch.uint8, (8, 3), 3, [raw, raw, {".shaf": raw, ".cod": b"@"}], 0), CR(torch.uint8, (8, 3), 3, [raw, raw, raw], 0),
                CR(torch.uint8, (8, 3), 3, [raw.view(2, 4), raw, raw], 0), CR(torch.uint8, (8, 3), 3, [raw.to(torch.int8), raw, raw], 0),
                CR(torch.complex128, (3,), 16, [raw] * 16, 0)):
        with pytest.raises(ValueError):
            records.decompress_records(bad)
    # compress_tensors keeps refusing elements of 16 bytes
    with pytest.raises(ValueError):
        shafa._plane_tensors("test", torch.zeros(4, dtype=torch.complex128, device="meta"))

"""CPU-side checks of the RLE size pass (shafa_hipd_rle_decoded_size_dev, csrc/rle_measure.hip):

1. declared, exported, bound in Python, the ABI version unchanged, and every argument error refused before HIP is touched
   (no GPU needed);
2. the oracle side of the entry's contract, on which tests/test_gpu_rle_measure.py rests: with cap = RLE_DECODE_MAX
   oracle.rle_decode returns success or FILE_UNRECOGNIZABLE and never LACK_OF_MEMORY — on every RLE stream of the golden
   sessions (stored, or rebuilt from the manifest: the oracle's RLE of each block of the session's input) and on the fuzz
   generator of the GPU tests."""
import ctypes as C
import json
import os

import numpy as np

from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "shafa_hipd_rle_decoded_size_dev"
BLOCK = {"K": 655360, "m": 8 << 20, "M": 64 << 20}


# ---------------------------------------------------------------- 1. the boundary
def test_declared_exported_and_bound(shafa):
    assert NAME in declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    assert hasattr(C.CDLL(shafa.LIB_PATH), NAME)
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "rle_decoded_size_dev", None))
    assert callable(getattr(shafa, "decoded_sizes", None)) and callable(getattr(shafa, "decompress_range", None))


class _Args:
    """stand-ins for the batch and the device pointers (tests/test_unpack_files_cpu.py): the batch's bytes are 0x7F, so its
    max_blocks is 0x7F7F7F7F; a call that gets past every check reaches HIP, which refuses the stand-in batch (it names no
    device) before anything is enqueued."""

    def __init__(self):
        self.raw = C.create_string_buffer(b"\x7f" * 512, 512)
        a = C.addressof(self.raw)
        self.p = C.c_void_p((a + 15) // 16 * 16)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


def test_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM = shafa.OUTSIDE_MODULE

    def call(**kw):
        a = dict(b=A.p, nb=3, d_in=A.p, off=_u64(0, 16, 4096), cap=_u64(5, 100, 70000), d_n=A.p, d_out_n=A.p)
        a.update(kw)
        return L.shafa_hipd_rle_decoded_size_dev(a["b"], None, a["nb"], C.cast(a["d_in"], C.POINTER(C.c_uint8)), a["off"],
                                                 a["cap"], a["d_n"], a["d_out_n"])

    assert call() not in (shafa.SUCCESS, OM, shafa.LACK_OF_MEMORY)     # every check passed: HIP refuses the stand-in batch
    for k in ("b", "d_n", "d_out_n", "off", "cap"):
        assert call(**{k: None}) == OM, k
    for bad in (_u64(1, 16, 4096), _u64(0, 24, 4096), _u64(0, 16, 4103)):
        assert call(off=bad) == OM
    assert call(nb=0) == shafa.SUCCESS and call(nb=-4) == shafa.SUCCESS
    assert call(nb=0, off=None, cap=None) == shafa.SUCCESS             # nothing to measure, nothing looked at
    assert call(nb=0x7F7F7F7F + 1) == shafa.LACK_OF_MEMORY             # past max_blocks: refused before an array is read
    assert call(nb=0x7FFFFFFF) == shafa.LACK_OF_MEMORY
    assert call(b=None, nb=0) == OM                                    # a NULL batch comes first


def test_queries_refuse_bad_arguments(shafa):
    import pytest
    import torch
    cpu = torch.zeros(8, dtype=torch.uint8)
    for fn in (shafa.decoded_sizes, lambda **k: shafa.decompress_range(0, 1, **k)):
        for e in ({"shaf": cpu, "cod": cpu}, {"rle": cpu, "freq": cpu}, {"shaf": cpu}, {"cod": cpu, "rle": cpu, "freq": cpu}, {}):
            with pytest.raises(ValueError):
                fn(**e)
    for off, n in ((-1, 5), (0, -1)):
        with pytest.raises(ValueError):
            shafa.decompress_range(off, n, rle=cpu, freq=cpu)


# ---------------------------------------------------------------- 2. the oracle's codes at cap = RLE_DECODE_MAX
def _opt(argv, flag):
    return argv[argv.index(flag) + 1] if flag in argv else None


def _session_input(case, man, fn):
    """the session's input: stored, or rebuilt from the manifest's generator (tests/test_gpu_pack.py: _case_input)"""
    import golden.make_golden as mg
    path = os.path.join(GOLD, case, fn)
    if os.path.exists(path):
        return np.fromfile(path, dtype=np.uint8)
    if "generators" in man:
        return mg.make_input(man["generators"][fn])
    zt = mg.zipf_table(1.2)
    return mg.runs_stream(7, 655360, zt) if case == "cfg0_K_runs" else mg.gen_bytes(8, 655360)


def _golden_rle_streams(oracle):
    """(case, block, stream) for every golden session with a .rle or .rle.shaf: the stored .rle cut by the stored .rle.freq
    where both are stored, else the oracle's RLE of every block of the input"""
    from oracle_lib import parse_blocks_text
    for case in sorted(os.listdir(GOLD)):
        p = os.path.join(GOLD, case, "manifest.json")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            man = json.load(f)
        argv = man["cmds"][0]["argv"]
        fn = argv[0]
        if fn + ".rle" not in man["files"] and fn + ".rle.shaf" not in man["files"]:
            continue
        rle_p, freq_p = os.path.join(GOLD, case, fn + ".rle"), os.path.join(GOLD, case, fn + ".rle.freq")
        if os.path.exists(rle_p) and os.path.exists(freq_p):
            rle = np.fromfile(rle_p, dtype=np.uint8)
            with open(freq_p, "rb") as f:
                _, blocks = parse_blocks_text(f.read())
            pos = 0
            for b, (size, _) in enumerate(blocks):
                yield case, b, rle[pos:pos + size]
                pos += size
            assert pos == rle.size, case
            continue
        data = _session_input(case, man, fn)
        bs = BLOCK.get(_opt(argv, "-b"), 65536)
        for b, a in enumerate(range(0, data.size, bs)):
            yield case, b, oracle.rle_encode(data[a:a + bs])


def test_oracle_never_lacks_memory_at_the_maximum_golden(oracle, shafa):
    MAX = int(shafa.RLE_DECODE_MAX)
    assert MAX == 67108864 + 1024
    cases, blocks = set(), 0
    for case, b, s in _golden_rle_streams(oracle):
        rc, out = oracle.rle_decode(s, cap=MAX)
        assert rc in (0, shafa.FILE_UNRECOGNIZABLE) and rc != shafa.LACK_OF_MEMORY, (case, b, rc)
        assert rc == 0, (case, b)                                      # an encoder's stream decodes
        cases.add(case)
        blocks += 1
    assert len(cases) == 20 and blocks > 1000, (sorted(cases), blocks)


def test_oracle_never_lacks_memory_at_the_maximum_fuzz(oracle, shafa):
    from test_gpu_rle_measure import fuzz_streams
    MAX = int(shafa.RLE_DECODE_MAX)
    codes = set()
    for i, s in enumerate(fuzz_streams()):
        rc, out = oracle.rle_decode(s, cap=MAX)
        assert rc in (0, shafa.FILE_UNRECOGNIZABLE) and rc != shafa.LACK_OF_MEMORY, (i, rc)
        assert rc == 0 or out.size == 0
        codes.add(rc)
    assert codes == {0, shafa.FILE_UNRECOGNIZABLE}
    # the maximum itself (tests/test_gpu_codec.py:148): reaching it is success, one byte more is FILE_UNRECOGNIZABLE
    n_tr = MAX // 255
    exact = np.concatenate([np.tile(np.array([0, 1, 255], dtype=np.uint8), n_tr), np.full(MAX - 255 * n_tr, 7, dtype=np.uint8)])
    rc, out = oracle.rle_decode(exact, cap=MAX)
    assert rc == 0 and out.size == MAX
    rc, out = oracle.rle_decode(np.concatenate([exact, np.array([9], dtype=np.uint8)]), cap=MAX)
    assert rc == shafa.FILE_UNRECOGNIZABLE and out.size == 0

"""CPU-side checks of the RLE encoded-size pass (shafa_hipd_rle_encoded_size_dev, csrc/rle_encode_measure.hip):

1. declared, exported, bound in Python, the ABI version unchanged, shafa.rle_encoded_sizes callable;
2. every argument error refused before HIP is touched (no GPU needed);
3. rle_encoded_sizes refuses CPU tensors;
4. the anchor on which tests/test_gpu_rle_encoded_size.py rests: the oracle's rle_encode size of every input block equals the
   block size the reference wrote into every stored .rle.freq, and the per-run rule of include/shafa_hip.h equals the oracle
   on the fuzz generator of the GPU tests;
5. that generator covers the run lengths, edges and block lengths the size pass has a path for."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle_lib import parse_blocks_text
from test_abi_cpu import declared_symbols
from test_gpu_rle_encoded_size import fuzz_inputs, rle_size_by_runs, runs_of, split_blocks
from test_rle_measure_cpu import BLOCK, GOLD, ROOT, _Args, _opt, _session_input, _u64

NAME = "shafa_hipd_rle_encoded_size_dev"
TILE = 8192


# ---------------------------------------------------------------- 1. - 3. the boundary
def test_declared_exported_and_bound(shafa):
    assert NAME in declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    assert hasattr(C.CDLL(shafa.LIB_PATH), NAME)
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "rle_encoded_size_dev", None))
    assert callable(getattr(shafa, "rle_encoded_sizes", None))


def test_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM = shafa.OUTSIDE_MODULE

    def call(**kw):
        a = dict(b=A.p, nb=3, d_in=A.p, off=_u64(0, 16, 4096), cap=_u64(5, 100, 70000), d_n=A.p, d_out_n=A.p)
        a.update(kw)
        return L.shafa_hipd_rle_encoded_size_dev(a["b"], None, a["nb"], C.cast(a["d_in"], C.POINTER(C.c_uint8)), a["off"],
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


def test_the_query_refuses_cpu_tensors(shafa):
    import torch
    cpu = torch.zeros(4096, dtype=torch.uint8)
    for args in ((cpu, [4096]), ([cpu, cpu], None), (cpu.numpy(), [4096]), (cpu, [])):
        with pytest.raises(ValueError):
            shafa.rle_encoded_sizes(*args)


# ---------------------------------------------------------------- 4. the anchor
def test_oracle_sizes_are_the_references(oracle, shafa):
    cases, blocks = set(), 0
    for case in sorted(os.listdir(GOLD)):
        p = os.path.join(GOLD, case, "manifest.json")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            man = json.load(f)
        cmd = man["cmds"][0]
        fn = cmd["argv"][0]
        freq_p = os.path.join(GOLD, case, fn + ".rle.freq")
        if not os.path.exists(freq_p):
            continue
        with open(freq_p, "rb") as f:
            mode, ref = parse_blocks_text(f.read())
        assert mode == "R", case
        data = _session_input(case, man, fn)
        sizes = split_blocks(shafa, data.size, BLOCK.get(_opt(cmd["argv"], "-b"), 65536))
        assert len(sizes) == len(ref), case
        pos = 0
        for b, (n, (want, _)) in enumerate(zip(sizes, ref)):
            x = data[pos:pos + n]
            got = len(oracle.rle_encode(x))
            assert got == want, (case, b, got, want)
            if n <= 1 << 20:
                assert rle_size_by_runs(x) == want, (case, b)
            pos += n
            blocks += 1
        cases.add(case)
    assert len(cases) == 18 and blocks == 91, (sorted(cases), blocks)


def test_the_per_run_rule_is_the_oracle_on_the_fuzz(oracle):
    inputs = fuzz_inputs()
    assert len(inputs) > 100
    for i, x in enumerate(inputs):
        assert rle_size_by_runs(x) == len(oracle.rle_encode(x)), i


def test_the_memory_tests_generator_is_run_heavy(oracle):
    from test_gpu_rle_measure import _run_heavy
    x = _run_heavy(31, 1 << 22, run=96)
    assert len(oracle.rle_encode(x)) <= 0.2 * x.size


# ---------------------------------------------------------------- 5. what the fuzz covers
def test_the_fuzz_covers_every_path():
    lengths, zero_runs, block_lengths = set(), set(), set()
    lane_cross = tile_cross = tile_end = three_tiles = False
    for x in fuzz_inputs():
        block_lengths.add(x.size)
        start, L, s = runs_of(x)
        end = start + L
        lengths.update(np.unique(L).tolist())
        zero_runs.update(np.unique(L[s == 0]).tolist())
        lane_cross |= bool(np.any((end - 1) // 32 > start // 32))
        tile_cross |= bool(np.any((end - 1) // TILE > start // TILE))
        tile_end |= bool(np.any((end % TILE == 0) & (end < x.size) & (L > 1)))
        first_whole = -(-start // TILE)                                # the first tile that starts inside the run
        three_tiles |= bool(np.any(end // TILE - first_whole >= 3))
    assert {1, 2, 3, 4, 254, 255, 256, 509, 510, 511} <= lengths
    assert {1, 2, 3} <= zero_runs
    assert lane_cross and tile_cross and tile_end and three_tiles
    assert {0, 1, 31, 32, 33, 8191, 8192, 8193} <= block_lengths

"""bench.py --dump-outputs without a GPU: which positions of the timed step's outputs the dump keeps, and where they lie
in the device buffer (tests/test_gpu_multi.py runs the dump itself against the oracle)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_keeps_small_outputs_whole_and_a_seeded_bounded_sample_of_large_ones():
    b = _bench()
    assert b.dump_positions(1000, 1).tolist() == list(range(1000))
    n = 128 * (64 << 20)                                         # the default shard: 128 blocks of 64 MiB
    p = b.dump_positions(n, 7)
    assert p.size == b.DUMP_SAMPLE and (np.diff(p) >= 0).all() and 0 <= p.min() and p.max() < n
    assert (p == b.dump_positions(n, 7)).all() and not (p == b.dump_positions(n, 8)).all()
    # two sampled outputs, value (float32) and position (float64) each, plus the sizes of up to 1024 blocks
    assert 2 * b.DUMP_SAMPLE * (4 + 8) + 1024 * 8 <= 64 * 10 ** 6


def test_encoded_positions_map_into_each_blocks_slot_and_skip_empty_blocks():
    b = _bench()
    enc = np.array([5, 0, 3, 0, 7], dtype=np.uint64)
    off = np.arange(5, dtype=np.uint64) * np.uint64(100)
    got = b.encoded_addresses(np.arange(15), off, enc)
    assert got.tolist() == [0, 1, 2, 3, 4, 200, 201, 202, 400, 401, 402, 403, 404, 405, 406]


def test_steps_must_be_positive():
    b = _bench()
    assert b.parse_args(["--steps", "3", "--dump-outputs", "d"]).steps == 3
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        try:
            b.parse_args(argv)
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError(f"{argv} accepted")


def test_full_is_off_by_default():
    b = _bench()
    assert b.parse_args([]).full is False
    assert b.parse_args(["--full"]).full is True

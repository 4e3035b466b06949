"""shafa.compressed_sizes: the lengths of the files compress_many would write, without an RLE or Shannon-Fano stream.

1. every golden session group (tests/test_gpu_pack_files.py: GROUPS, with the group's -b and -c r|f): compressed_sizes equals
   {key: numel} of compress_many with the same arguments, file by file, and equal error codes where a file is refused;
2. the same on 24 mixed synthetic files, run-heavy and random, a refused file and a last block of one byte among them;
3. no encoder and no payload pack runs, and finish is called at most as often as by compress_many;
4. peak device memory beyond a 256 MiB input at 64 MiB blocks stays under n / 8."""
import numpy as np
import pytest

from test_gpu_pack import BLOCK, _case_input, _manifest
from test_gpu_pack_files import GROUPS
from test_gpu_rle_measure import _count_calls, _run_heavy
from test_gpu_unpack import _dev

pytestmark = pytest.mark.gpu

M64 = 64 << 20


def _same_sizes(shafa, got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, shafa.ShafaError):
            assert isinstance(g, shafa.ShafaError) and g.code == w.code, (what, i, g, w)
            continue
        assert isinstance(g, dict), (what, i, g)
        assert all(type(v) is int for v in g.values()), (what, i, g)
        assert g == {k: int(v.numel()) for k, v in w.items()}, (what, i, g, {k: int(v.numel()) for k, v in w.items()})


# ---------------------------------------------------------------- 1. golden sessions
@pytest.mark.parametrize("key,cases", GROUPS, ids=[f"b{k[0]}-c{k[1]}" for k, _ in GROUPS])
def test_golden_session_groups(shafa, key, cases):
    import torch
    b, c = key
    kw = dict(force_rle=c == "r", force_freq=c == "f")
    bs = BLOCK.get(b, 65536)
    datas, sessions = [], []
    try:
        for case in cases:
            man = _manifest(case)
            data, S = _case_input(shafa, case, man, man["cmds"][0]["argv"][0])
            if S is not None:
                sessions.append(S)
            datas.append(data)
        d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
        sizes = [d.size for d in datas]
        got = shafa.compressed_sizes(d_in, sizes, bs, **kw)
        want = shafa.compress_many(d_in, sizes, bs, **kw)
        _same_sizes(shafa, got, want, str(key))
    finally:
        for S in sessions:
            S.close()


# ---------------------------------------------------------------- 2. synthetic files
def _mixed_files():
    N = 65536
    rng = np.random.default_rng(6)
    sizes = [1000, 1024, 5000, N, 3 * N + 100, 2 * N + 1]
    datas = []
    for i in range(24):
        n = sizes[i % len(sizes)] if i < 12 else int(rng.choice(sizes))
        datas.append(_run_heavy(50 + i, n, run=int(rng.choice([5, 64, 400]))) if i % 3 != 1 else rng.integers(0, 256, n, dtype=np.uint8))
    return datas, N


@pytest.mark.parametrize("kw", [dict(), dict(force_rle=True), dict(force_freq=True), dict(force_rle=True, force_freq=True)],
                         ids=["default", "r", "f", "rf"])
def test_mixed_synthetic_files(shafa, kw):
    import torch
    datas, N = _mixed_files()
    d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
    sizes = [d.size for d in datas]
    got = shafa.compressed_sizes(d_in, sizes, N, **kw)
    want = shafa.compress_many(d_in, sizes, N, **kw)
    _same_sizes(shafa, got, want, str(kw))
    assert any(isinstance(w, shafa.ShafaError) and w.code == shafa.FILE_TOO_SMALL for w in want)
    if not kw:
        assert {".rle" in w for w in want if isinstance(w, dict)} == {True, False}
    # a list of tensors, as compress_many takes it
    got = shafa.compressed_sizes([torch.from_numpy(d).to(_dev()) for d in datas[:7]], None, N, **kw)
    _same_sizes(shafa, got, want[:7], "list")


# ---------------------------------------------------------------- 3. what runs
@pytest.mark.parametrize("force_rle", [False, True])
def test_nothing_is_encoded_and_no_more_synchronisations(shafa, monkeypatch, force_rle):
    import torch
    datas, N = _mixed_files()
    d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
    sizes = [d.size for d in datas]
    fin = _count_calls(shafa, monkeypatch, "finish")
    shafa.compress_many(d_in, sizes, N, force_rle=force_rle)
    many = len(fin)
    assert many == (1 if force_rle else 2)
    fin.clear()
    banned = [_count_calls(shafa, monkeypatch, name) for name in ("rle_encode_tiles", "rle_encode", "sf_encode_dev", "sf_encode",
                                                                  "pack_payloads_files", "pack_payloads")]
    hist = _count_calls(shafa, monkeypatch, "rle_encoded_hist_dev")
    size = _count_calls(shafa, monkeypatch, "sf_encoded_size_dev")
    res = shafa.compressed_sizes(d_in, sizes, N, force_rle=force_rle)
    assert len(res) == len(datas)
    assert not any(banned), [len(c) for c in banned]
    assert len(hist) == 1 and len(size) == 1
    assert len(fin) <= many, (len(fin), many)


# ---------------------------------------------------------------- 4. memory
def test_peak_memory_stays_far_below_the_input(shafa):
    import torch
    n = 256 << 20
    nb = n // M64
    # compress_files' own regions at this shape: the encoder's output c + c / 2 + 64 per block, and the .shaf of the same
    # capacities — over 1.6 n each way; this chain holds per block two histograms, a table and the bounds of three texts
    enc = nb * (M64 + M64 // 2 + 64)
    texts = 3 * shafa.pack_cod_max(nb) + 4 * nb * (256 * 8 + 8320)
    assert texts < n // 8 < 1.6 * n < 2 * enc
    zt = torch.from_numpy(shafa.zipf_table(1.2)).to(_dev())
    g = torch.Generator(device=_dev())
    g.manual_seed(12)
    d_in = zt[torch.randint(0, 65536, (n,), device=_dev(), generator=g)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = shafa.compressed_sizes(d_in, [n], M64)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak {peak} bytes = {peak / n:.5f} n")
    assert isinstance(res[0], dict) and ".shaf" in res[0] and 0 < res[0][".shaf"] < n
    assert peak < n // 8, f"{peak / n:.4f} n"

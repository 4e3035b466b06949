"""CPU-side checks of the size-only chain (shafa_hipd_rle_encoded_hist_dev, csrc/rle_encode_hist.hip;
shafa_hipd_sf_encoded_size_dev, csrc/sf_encoded_size.hip; shafa.compressed_sizes):

1. both entries declared, exported and bound, the ABI version unchanged;
2. their argument errors refused before HIP is touched (no GPU needed);
3. the composition the kernels implement — the plain histogram of the input plus a signed correction per encoded run, runs
   charged where a composition closes them, the block's first and last run at the end — equals the histogram of the oracle's
   RLE bytes, for pieces of 1, 7 and 32 bytes folded as a tree and in the kernels' lane -> wave -> tile -> block order;
4. the .shaf length arithmetic equals the length of every golden .shaf file, from the block sizes parsed out of it."""
import ctypes as C
import os

import numpy as np
import pytest

from test_abi_cpu import declared_symbols
from test_rle_measure_cpu import GOLD, ROOT, _Args, _u64

HIST, SIZE = "shafa_hipd_rle_encoded_hist_dev", "shafa_hipd_sf_encoded_size_dev"


# ---------------------------------------------------------------- 1. - 2. the boundary
def test_declared_exported_and_bound(shafa):
    declared = declared_symbols(os.path.join(ROOT, "include", "shafa_hip.h"))
    L = C.CDLL(shafa.LIB_PATH)
    for name in (HIST, SIZE):
        assert name in declared and hasattr(L, name), name
    assert shafa.lib().shafa_hip_abi_version() == 8
    assert callable(getattr(shafa.Batch, "rle_encoded_hist_dev", None))
    assert callable(getattr(shafa.Batch, "sf_encoded_size_dev", None))
    assert callable(getattr(shafa, "compressed_sizes", None))


def test_hist_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM = shafa.OUTSIDE_MODULE

    def call(**kw):
        a = dict(b=A.p, nb=3, d_in=A.p, off=_u64(0, 16, 4096), cap=_u64(5, 100, 70000), d_n=A.p, d_out_n=A.p, d_freq=A.p)
        a.update(kw)
        return L.shafa_hipd_rle_encoded_hist_dev(a["b"], None, a["nb"], a["d_in"], a["off"], a["cap"], a["d_n"], a["d_out_n"],
                                                 a["d_freq"])

    assert call() not in (shafa.SUCCESS, OM, shafa.LACK_OF_MEMORY)     # every check passed: HIP refuses the stand-in batch
    for k in ("b", "d_n", "d_out_n", "d_freq", "off", "cap"):
        assert call(**{k: None}) == OM, k
    for bad in (_u64(1, 16, 4096), _u64(0, 24, 4096), _u64(0, 16, 4103)):
        assert call(off=bad) == OM
    assert call(nb=0) == shafa.SUCCESS and call(nb=-4) == shafa.SUCCESS
    assert call(nb=0, off=None, cap=None) == shafa.SUCCESS
    assert call(nb=0x7F7F7F7F + 1) == shafa.LACK_OF_MEMORY
    assert call(b=None, nb=0) == OM and call(d_freq=None, nb=0) == OM


def test_sf_size_argument_errors_before_hip(shafa):
    L = shafa.lib()
    A = _Args()
    OM = shafa.OUTSIDE_MODULE

    def call(**kw):
        a = dict(b=A.p, nb=3, d_freq=A.p, d_tables=A.p, d_out_n=A.p)
        a.update(kw)
        return L.shafa_hipd_sf_encoded_size_dev(a["b"], None, a["nb"], a["d_freq"], a["d_tables"], a["d_out_n"])

    assert call() not in (shafa.SUCCESS, OM, shafa.LACK_OF_MEMORY)
    for k in ("b", "d_freq", "d_tables", "d_out_n"):
        assert call(**{k: None}) == OM, k
    assert call(nb=0) == shafa.SUCCESS and call(nb=-1) == shafa.SUCCESS
    assert call(nb=0x7F7F7F7F + 1) == shafa.LACK_OF_MEMORY
    assert call(b=None, nb=0) == OM


def test_the_query_refuses_cpu_tensors(shafa):
    import torch
    cpu = torch.zeros(4096, dtype=torch.uint8)
    for args in ((cpu, [4096]), ([cpu, cpu], None), (cpu, [])):
        with pytest.raises(ValueError):
            shafa.compressed_sizes(*args)


# ---------------------------------------------------------------- 3. the composition
def charge(H, s, L):
    """the correction of one maximal run (csrc/rle_encode_hist.hip: charge)"""
    if s != 0 and L < 4:
        return
    q, m = divmod(L, 255)
    H[s] -= L
    H[0] += q
    H[s] += q
    H[255] += q
    if m:
        if s == 0 or m >= 4:
            H[0] += 1
            H[s] += 1
            H[m] += 1
        else:
            H[s] += m


def piece(H, x):
    """a lane's summary (n, first byte, first-run length, last byte, last-run length); the runs strictly inside are charged"""
    n = len(x)
    if n == 0:
        return (0, 0, 0, 0, 0)
    heads = [0] + [i for i in range(1, n) if x[i] != x[i - 1]]
    ends = heads[1:] + [n]
    for h, e in list(zip(heads, ends))[1:-1]:
        charge(H, int(x[h]), e - h)
    return (n, int(x[0]), ends[0], int(x[-1]), n - heads[-1])


def then(H, a, b):
    """rs_then"""
    if a[0] == 0:
        return b
    if b[0] == 0:
        return a
    ua, ub = a[2] == a[0], b[2] == b[0]
    flen, llen = a[2], b[4]
    if a[3] == b[1]:
        if ua:
            flen = a[0] + b[2]
        if ub:
            llen = a[4] + b[0]
        if not ua and not ub:
            charge(H, a[3], a[4] + b[2])
    else:
        if not ua:
            charge(H, a[3], a[4])
        if not ub:
            charge(H, b[1], b[2])
    return (a[0] + b[0], a[1], flen, b[3], llen)


def tree(H, items):
    """the aligned tree of rs_wave_reduce: at distance d the multiples of 2 d take the d items behind them"""
    items = list(items)
    d = 1
    while d < len(items):
        for i in range(0, len(items), 2 * d):
            if i + d < len(items):
                items[i] = then(H, items[i], items[i + d])
        d *= 2
    return items[0] if items else (0, 0, 0, 0, 0)


def seq(H, items):
    r = (0, 0, 0, 0, 0)
    for it in items:
        r = then(H, r, it)
    return r


def finish(H, t):
    if t[0] == 0:
        return
    if t[2] == t[0]:
        charge(H, t[1], t[0])
    else:
        charge(H, t[1], t[2])
        charge(H, t[3], t[4])


def _chunks(items, k):
    return [items[i:i + k] for i in range(0, len(items), k)]


def model(x, bpl, order, lanes=64, waves=4, threads=8):
    """the histogram of x's RLE bytes by the kernels' composition; order "tree": one tree over all pieces; "kernel": lanes of
    bpl bytes -> waves of `lanes` lanes (tree) -> tiles of `waves` waves (in order) -> per thread a run of consecutive tiles
    (in order) -> waves of threads (tree) -> the waves in order"""
    H = [int(c) for c in np.bincount(x, minlength=256)]
    pieces = [piece(H, x[i:i + bpl]) for i in range(0, len(x), bpl)]
    if order == "tree":
        t = tree(H, pieces)
    else:
        tiles = [seq(H, [tree(H, w) for w in _chunks(t, lanes)]) for t in _chunks(pieces, lanes * waves)]
        per = -(-len(tiles) // threads) if tiles else 1
        thr = [seq(H, c) for c in _chunks(tiles, per)]
        t = seq(H, [tree(H, w) for w in _chunks(thr, 4)])
    finish(H, t)
    return H


def model_inputs(seed=20261017):
    rng = np.random.default_rng(seed)
    out = [np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint8), np.full(1, 9, dtype=np.uint8)]
    for k in range(300):
        alphabet = [[0], [0, 7], [0, 1, 255], [255], [4, 255], [7]][k % 6][:int(rng.integers(1, 4))]
        lens = [[1, 2, 3, 4, 5], [1, 3, 4, 7, 254, 255, 256], [258, 259, 510, 511, 700], [1, 1, 2, 31, 32, 33]][k % 4]
        parts, tot, n = [], 0, int(rng.integers(1, 1500))
        while tot < n:
            L = int(rng.choice(lens))
            parts.append(np.full(L, int(rng.choice(alphabet)), dtype=np.uint8))
            tot += L
        out.append(np.concatenate(parts)[:n])
    out.append(np.full(255 * 3, 255, dtype=np.uint8))
    out.append(np.full(255, 0, dtype=np.uint8))
    out.append(np.concatenate([np.full(7, 7, dtype=np.uint8), np.full(256, 255, dtype=np.uint8), np.zeros(255, dtype=np.uint8)]))
    return out


def test_the_composition_equals_the_oracles_histogram(oracle):
    inputs = model_inputs()
    assert len(inputs) > 300
    for i, x in enumerate(inputs):
        want = np.bincount(oracle.rle_encode(x), minlength=256).tolist()
        for bpl in (1, 7, 32):
            assert model(x, bpl, "tree") == want, (i, bpl, "tree")
            # small waves and tiles, so that inputs of a few hundred bytes pass every level
            assert model(x, bpl, "kernel", lanes=4, waves=2, threads=3) == want, (i, bpl, "kernel")


def test_the_composition_at_the_kernels_geometry(oracle):
    rng = np.random.default_rng(5)
    x = np.repeat(rng.integers(0, 3, 3000).astype(np.uint8), rng.choice([1, 2, 3, 4, 40, 300, 9000], 3000))[:5 * 8192 + 77]
    want = np.bincount(oracle.rle_encode(x), minlength=256).tolist()
    assert model(x, 32, "kernel") == want
    assert sum(want) == len(oracle.rle_encode(x))


# ---------------------------------------------------------------- 4. the .shaf length
def _shaf_block_sizes(data):
    """"@<blocks>", then "@<size>@" + payload per block -> the sizes"""
    pos = 1
    assert data[:1] == b"@"
    end = data.index(b"@", pos)
    nb = int(data[pos:end])
    pos, sizes = end, []
    for _ in range(nb):
        assert data[pos:pos + 1] == b"@"
        end = data.index(b"@", pos + 1)
        n = int(data[pos + 1:end])
        sizes.append(n)
        pos = end + 1 + n
    assert pos == len(data)
    return sizes


def test_shaf_length_arithmetic_on_the_golden_files(shafa):
    seen = 0
    for case in sorted(os.listdir(GOLD)):
        d = os.path.join(GOLD, case)
        if not os.path.isdir(d) or "bad_cod" in case:                   # sessions with a damaged .cod: Module C stopped inside the file
            continue
        for fn in sorted(os.listdir(d)):
            if not fn.endswith(".shaf"):
                continue
            with open(os.path.join(d, fn), "rb") as f:
                data = f.read()
            assert shafa.shaf_file_bytes(_shaf_block_sizes(data)) == len(data), (case, fn)
            seen += 1
    assert seen >= 10, seen
    assert shafa.shaf_file_bytes([0]) == len(b"@1@0@") and shafa.shaf_file_bytes([10] * 10) == len(b"@10") + 10 * (4 + 10)

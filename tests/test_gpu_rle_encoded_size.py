"""The RLE encoded-size pass (shafa_hipd_rle_encoded_size_dev, csrc/rle_encode_measure.hip), the compress drivers that settle
the RLE choice with it before anything is encoded, and the query built on it (shafa.rle_encoded_sizes).

6. every block of every golden session's input measures the oracle's RLE size (the reference's where a .rle.freq is stored),
   session by session and all sessions in one call;
7. seeded fuzz (fuzz_inputs; tests/test_rle_encoded_size_cpu.py checks what it covers): sizes equal the oracle's and
   shafa_hipd_rle_encode's d_out_n on the same blocks, all codes success;
8. a 64 MiB single run, 64 MiB of alternating 0, 1 (the worst case, 2 n) and 64 MiB of Zipf bytes;
9. a block past its capacity is OUTSIDE_MODULE alone; nothing around d_out_n is written, the input is not changed;
10. the call only enqueues;
11. one 64 MiB block next to 2 100 blocks of 1 KiB in one size call, and the same mix through compress_many at -b M;
12. the drivers call rle_encode_tiles once, over the blocks of the files that take RLE only, with out_cap = the measured
    sizes (guard bytes behind every exact region stay untouched), and not at all when every file is plain;
13. compress_many equals compress_files per file on the golden sessions, both decompress drivers round-trip, and the drivers
    synchronise twice (once with force_rle);
14. peak device memory of compress_files, from the code's own bounds: plain under 4 n, run-heavy under 2 n;
15. rle_encoded_sizes on the golden sessions."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle_lib import parse_blocks_text
from test_gpu_pack import BLOCK, F_CASES, GOLD, _case_input, _manifest, _opt
from test_gpu_pack_files import GROUPS
from test_gpu_rle_measure import SENT, TILE, _al16, _Blocks, _count_calls, _run_heavy
from test_gpu_unpack import _bytes, _dev

pytestmark = pytest.mark.gpu

M64 = 64 << 20


def rle_size_by_runs(x):
    """the size rule of include/shafa_hip.h, per maximal run: 3 (L / 255), plus for m = L % 255: 0 if m == 0; 3 if s == 0 or
    m >= 4; else m"""
    x = np.asarray(x, dtype=np.uint8)
    if x.size == 0:
        return 0
    heads = np.flatnonzero(np.concatenate([[True], x[1:] != x[:-1]]))
    L = np.diff(np.concatenate([heads, [x.size]]))
    s = x[heads]
    m = L % 255
    return int(np.sum(3 * (L // 255) + np.where(m == 0, 0, np.where((s == 0) | (m >= 4), 3, m))))


def runs_of(x):
    """(start, length, symbol) arrays of the maximal runs of x"""
    x = np.asarray(x, dtype=np.uint8)
    if x.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    heads = np.flatnonzero(np.concatenate([[True], x[1:] != x[:-1]]))
    return heads, np.diff(np.concatenate([heads, [x.size]])), x[heads].astype(np.int64)


def fuzz_inputs(seed=20261016):
    """input blocks that walk every path of the size pass: run lengths around the literal / triple rule (1 .. 4) and around
    255 and 510, zero runs, runs across and up to lane (32 bytes) and tile (8 KiB) edges, runs over several tiles, blocks
    around a lane and around a tile, noise (no lane is one run) and run-heavy text (many are)"""
    rng = np.random.default_rng(seed)
    out = []

    def runs(n, lens, p_zero):
        parts, tot, prev = [], 0, -1
        while tot < n:
            s = 0 if rng.random() < p_zero else int(rng.integers(1, 256))
            if s == prev:
                continue
            L = int(rng.choice(lens))
            parts.append(np.full(L, s, dtype=np.uint8))
            tot += L
            prev = s
        return np.concatenate(parts)[:n] if parts else np.zeros(0, dtype=np.uint8)

    edge = [1, 2, 3, 4, 254, 255, 256, 509, 510, 511]
    for n in (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, TILE - 1, TILE, TILE + 1, 2 * TILE + 17, 5 * TILE + 100):
        for lens, pz in (([1], 0.0), ([1], 0.3), ([1, 1, 1, 2, 3], 0.2), ([1, 2, 3, 4, 5, 6], 0.3), (edge, 0.2),
                         ([30, 31, 32, 33, 64, 100], 0.1), ([max(n, 1)], 0.5)):
            out.append(runs(n, lens, pz))
    noise = lambda n: rng.integers(1, 256, n, dtype=np.uint8)          # noqa: E731
    for s in (0, 65):                                                  # runs placed against the tile edges
        out.append(np.concatenate([noise(TILE - 300), np.full(300, s, dtype=np.uint8), noise(500)]))          # ends on the edge
        out.append(np.concatenate([noise(TILE - 10), np.full(20, s, dtype=np.uint8), noise(500)]))            # crosses it
        out.append(np.concatenate([noise(TILE - 1), np.full(2, s, dtype=np.uint8), noise(TILE - 1), np.full(TILE + 2, s, dtype=np.uint8)]))
        out.append(np.concatenate([noise(100), np.full(4 * TILE + 50, s, dtype=np.uint8), noise(100)]))       # whole tiles
        out.append(np.concatenate([noise(TILE), np.full(3 * TILE, s, dtype=np.uint8), noise(TILE)]))
        out.append(np.full(5 * TILE, s, dtype=np.uint8))
        out.append(np.full(255 * 40, s, dtype=np.uint8))
        out.append(np.concatenate([np.full(255 * 33 + 3, s, dtype=np.uint8), np.full(255 * 2, s + 1, dtype=np.uint8)]))
    out.append(rng.integers(0, 256, 5 * TILE + 100, dtype=np.uint8))
    out.append(rng.integers(0, 3, 4 * TILE + 7, dtype=np.uint8))
    out.append(np.tile(np.array([0, 1], dtype=np.uint8), 2 * TILE))
    out.append(runs(6 * TILE, [1, 2, 3, 4, 40, 96, 300], 0.1))
    return out


def _measure(shafa, blk, bt=None, st=None):
    """one size pass over blk -> (sizes, codes)"""
    import torch
    nb = len(blk.n)
    own = bt is None
    bt = bt or shafa.Batch(nb, 1 << 20)
    st = st or torch.cuda.Stream(device=_dev())
    try:
        d_size = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_encoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        return d_size.cpu().numpy().view(np.uint64).tolist(), errs
    finally:
        if own:
            bt.close()


def split_blocks(shafa, n, block_size):
    """the C host's block split of a file of n bytes"""
    bs, last = C.c_uint64(int(block_size)), C.c_uint64(0)
    nb = int(shafa.host().shafa_block_count(n, C.byref(bs), C.byref(last)))
    return [bs.value] * (nb - 1) + [last.value]


def _cut(data, sizes):
    out, pos = [], 0
    for n in sizes:
        out.append(data[pos:pos + n])
        pos += n
    assert pos == data.size
    return out


def _session_blocks(shafa, case):
    """-> (the blocks of the session's input, the block sizes of the stored .rle.freq or None, the Session to close or None)"""
    man = _manifest(case)
    argv = man["cmds"][0]["argv"]
    fn = argv[0]
    data, S = _case_input(shafa, case, man, fn)
    blocks = _cut(data, split_blocks(shafa, data.size, BLOCK.get(_opt(argv, "-b"), 65536)))
    ref = None
    p = os.path.join(GOLD, case, fn + ".rle.freq")
    if os.path.exists(p):
        with open(p, "rb") as f:
            mode, bl = parse_blocks_text(f.read())
        assert mode == "R"
        ref = [size for size, _ in bl]
    return blocks, ref, S


# ---------------------------------------------------------------- 6. golden sessions
def test_golden_inputs_measure_the_oracles_size(oracle, shafa):
    import torch
    every, every_want, with_ref = [], [], 0
    for case in F_CASES:
        blocks, ref, S = _session_blocks(shafa, case)
        try:
            want = [len(oracle.rle_encode(b)) for b in blocks]
            if ref is not None:
                assert want == ref, f"{case}: the oracle's sizes are not the reference's"
                with_ref += 1
            got_n, got_rc = _measure(shafa, _Blocks(blocks))
            assert not any(got_rc) and got_n == want, f"{case}: sizes {got_n[:6]} codes {got_rc[:6]}, the oracle encodes {want[:6]}"
            every += [torch.from_numpy(np.ascontiguousarray(b)).to(_dev()) for b in blocks]
            every_want += want
        finally:
            if S is not None:
                S.close()
    assert with_ref == 17 and len(every) > 1000, (with_ref, len(every))
    # all sessions in one call, assembled on the device
    off, pos = [], 0
    for t in every:
        off.append(pos)
        pos += _al16(t.numel()) + 16
    d_in = torch.empty(pos + 16, dtype=torch.uint8, device=_dev())
    for o, t in zip(off, every):
        d_in[o:o + t.numel()].copy_(t)
    sizes = [t.numel() for t in every]
    del every
    nb = len(sizes)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        d_n = torch.tensor(sizes, dtype=torch.int64, device=_dev())
        d_size = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_encoded_size_dev(st, d_in, off, sizes, d_n, d_size)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        assert not any(errs) and d_size.cpu().tolist() == every_want
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. fuzz
def test_fuzz_equals_the_oracle_and_the_encoder(oracle, shafa):
    import torch
    blocks = fuzz_inputs()
    assert len(blocks) > 100
    want = [len(oracle.rle_encode(b)) for b in blocks]
    blk = _Blocks(blocks)
    nb = len(blocks)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        got_n, got_rc = _measure(shafa, blk, bt, st)
        bad = [(i, blocks[i].size, got_n[i], got_rc[i], want[i]) for i in range(nb) if (got_n[i], got_rc[i]) != (want[i], 0)]
        assert not bad, f"(block, bytes, size, code, the oracle's size): {bad[:10]}"
        room = [2 * n + 3 for n in blk.n]
        ooff, pos = [], 0
        for r in room:
            ooff.append(pos)
            pos += _al16(r) + 16
        d_out = torch.empty(pos + 16, dtype=torch.uint8, device=_dev())
        d_enc_n = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_encode(st, blk.d_in, blk.off, blk.n, d_out, ooff, room, d_enc_n)
        _, enc_rc = bt.finish(st, nb, raise_on_error=False)
        assert not any(enc_rc)
        assert d_enc_n.cpu().tolist() == got_n
    finally:
        bt.close()


# ---------------------------------------------------------------- 8. whole 64 MiB blocks
def test_64_mib_blocks(oracle, shafa):
    rng = np.random.default_rng(3)
    zipf = shafa.zipf_table(1.2)[rng.integers(0, 65536, M64)]
    blocks = [np.full(M64, 7, dtype=np.uint8), np.tile(np.array([0, 1], dtype=np.uint8), M64 // 2), zipf]
    want = [len(oracle.rle_encode(b)) for b in blocks]
    assert want[0] == 3 * (M64 // 255) + 3 and want[1] == 2 * M64
    got_n, got_rc = _measure(shafa, _Blocks(blocks))
    assert not any(got_rc) and got_n == want, (got_n, want)


# ---------------------------------------------------------------- 9. capacities, sentinels, the input
def test_a_block_past_its_capacity_fails_alone(oracle, shafa):
    import torch
    blocks = [np.frombuffer(bytes([65, 65, 65, 65, 66, 0] * 700), dtype=np.uint8), np.full(9000, 3, dtype=np.uint8),
              np.frombuffer(bytes([0, 5, 5, 0, 0, 200] * 2000), dtype=np.uint8), np.zeros(0, dtype=np.uint8)]
    want = [len(oracle.rle_encode(b)) for b in blocks]
    blk = _Blocks(blocks)
    blk.d_n[1] = blk.cap[1] + 1
    before = blk.d_in.clone()
    nb = len(blocks)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        words = torch.full((nb + 8,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_encoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, words[4:4 + nb])
        _, errs = bt.finish(st, nb, raise_on_error=False)
        w = words.cpu().tolist()
        assert errs == [0, shafa.OUTSIDE_MODULE, 0, 0], errs
        assert w[4:4 + nb] == [want[0], 0, want[2], 0], w
        assert w[:4] == [SENT] * 4 and w[4 + nb:] == [SENT] * 4
        assert torch.equal(blk.d_in, before)
    finally:
        bt.close()


# ---------------------------------------------------------------- 10. enqueue only
def test_the_call_only_enqueues(shafa):
    import torch
    rng = np.random.default_rng(5)
    blocks = [rng.integers(1, 256, 70000, dtype=np.uint8) for _ in range(6)]
    want = [rle_size_by_runs(b) for b in blocks]
    blk = _Blocks(blocks)
    nb = len(blocks)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        d_size = torch.zeros(nb, dtype=torch.int64, device=_dev())
        bt.rle_encoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size)     # warm-up: the batch grows here
        bt.finish(st, nb)
        assert d_size.cpu().tolist() == want
        d_size.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)
        bt.rle_encoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size)
        busy = not st.query()
        bt.finish(st, nb)
        assert busy, "the stream had drained when the call returned: something synchronised"
        assert d_size.cpu().tolist() == want
    finally:
        bt.close()


# ---------------------------------------------------------------- 11. the grid
def _big_and_small():
    rng = np.random.default_rng(8)
    big = _run_heavy(11, M64, run=300)
    big[5 * TILE:9 * TILE + 77] = 0                                    # a zero run over whole tiles
    small = []
    for i in range(2100):
        s = _run_heavy(1000 + i, 1024, run=40) if i % 3 == 0 else rng.integers(0, 256, 1024, dtype=np.uint8)
        small.append(s)
    return small[:1000] + [big] + small[1000:]


def test_one_large_block_among_thousands_of_small_ones(oracle, shafa):
    blocks = _big_and_small()
    caps = [b.size for b in blocks]
    assert (M64 // TILE) * len(blocks) * 256 > 1 << 32
    want = [len(oracle.rle_encode(b)) for b in blocks]
    got_n, got_rc = _measure(shafa, _Blocks(blocks, caps))
    assert not any(got_rc)
    assert got_n == want


def _same_files(got, want, what):
    assert isinstance(got, dict), (what, got)
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert _bytes(got[k]) == _bytes(want[k]), f"{what}: {k} differs"


def test_the_same_mix_through_compress_many(shafa):
    import torch
    files = _big_and_small()
    d_in = torch.from_numpy(np.concatenate(files)).to(_dev())
    res = shafa.compress_many(d_in, [f.size for f in files], M64)
    assert len(res) == len(files)
    kinds = set()
    pos = 0
    for i, f in enumerate(files):
        want = shafa.compress_files(d_in[pos:pos + f.size], M64)
        _same_files(res[i], want, f"file {i}")
        kinds.add(".rle" in want)
        pos += f.size
    assert kinds == {True, False}
    assert ".rle" in res[1000]


# ---------------------------------------------------------------- 12. the drivers take exact regions
def _guarded(shafa, monkeypatch):
    """count rle_encode_tiles' calls; each call's output buffer is filled with 0xA5 before the launch"""
    calls = []
    real = shafa.Batch.rle_encode_tiles

    def wrapper(self, *a, **k):
        a[4].fill_(0xA5)
        calls.append(a)
        return real(self, *a, **k)

    monkeypatch.setattr(shafa.Batch, "rle_encode_tiles", wrapper)
    return calls


def _check_exact(call, want_sizes, want_in_n):
    """one captured rle_encode_tiles call: (stream, d_in, in_off, in_n, d_out, out_off, out_cap, d_out_n, ...)"""
    _, _, in_off, in_n, d_out, out_off, out_cap, d_out_n = call[:8]
    nb = len(want_sizes)
    assert list(in_n) == want_in_n and len(in_off) == nb
    assert [int(c) for c in out_cap] == want_sizes
    assert d_out_n[:nb].cpu().tolist() == want_sizes                   # every region is filled exactly
    host = d_out.cpu().numpy()
    ends = list(out_off[1:]) + [host.size]
    for b in range(nb):
        lo = out_off[b] + want_sizes[b]
        assert ends[b] >= lo and (host[lo:ends[b]] == 0xA5).all(), f"block {b}: bytes behind its region were written"
    assert host.size >= out_off[-1] + want_sizes[-1] + 16


def test_compress_files_encodes_into_exact_regions(oracle, shafa, monkeypatch):
    import torch
    N = 65536
    data = np.concatenate([_run_heavy(20 + i, N, run=r) for i, r in enumerate((96, 5, 300, 4, 1000, 17))] + [_run_heavy(9, 777, run=9)])
    sizes = split_blocks(shafa, data.size, N)
    want = [len(oracle.rle_encode(b)) for b in _cut(data, sizes)]
    calls = _guarded(shafa, monkeypatch)
    files = shafa.compress_files(torch.from_numpy(data).to(_dev()), N)
    assert len(calls) == 1 and ".rle" in files
    _check_exact(calls[0], want, sizes)
    assert files[".rle"].numel() == sum(want)
    calls.clear()
    rng = np.random.default_rng(4)
    files = shafa.compress_files(torch.from_numpy(rng.integers(0, 256, 5 * N + 9, dtype=np.uint8)).to(_dev()), N)
    assert not calls and ".shaf" in files and ".rle" not in files


def test_compress_many_encodes_only_the_files_that_take_rle(oracle, shafa, monkeypatch):
    import torch
    N = 65536
    rng = np.random.default_rng(6)
    datas = []
    for i in range(24):
        n = int(rng.choice([1024, 5000, N, 3 * N + 100, 2 * N]))
        datas.append(_run_heavy(50 + i, n, run=int(rng.choice([5, 64, 400]))) if i % 3 != 1 else rng.integers(0, 256, n, dtype=np.uint8))
    d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
    q = shafa.rle_encoded_sizes(d_in, [d.size for d in datas], N)
    calls = _guarded(shafa, monkeypatch)
    res = shafa.compress_many(d_in, [d.size for d in datas], N)
    assert len(calls) == 1
    want, want_in = [], []
    for i, d in enumerate(datas):
        assert isinstance(res[i], dict), (i, res[i])
        assert (".rle" in res[i]) == (i % 3 != 1) == q[i][0], i
        if ".rle" in res[i]:
            blocks = _cut(d, split_blocks(shafa, d.size, N))
            sizes = [len(oracle.rle_encode(b)) for b in blocks]
            assert q[i][1] == sizes
            want += sizes
            want_in += [b.size for b in blocks]
    _check_exact(calls[0], want, want_in)                              # RLE files first, in the order given
    calls.clear()
    plain = [d for i, d in enumerate(datas) if i % 3 == 1]
    res = shafa.compress_many([torch.from_numpy(d).to(_dev()) for d in plain], None, N)
    assert not calls and all(isinstance(r, dict) and ".shaf" in r for r in res)


# ---------------------------------------------------------------- 13. parity, round trips, synchronisations
def _round_trip_args(files):
    if ".rle" in files:
        return [dict(rle=files[".rle"], freq=files[".rle.freq"]), dict(shaf=files[".rle.shaf"], cod=files[".rle.cod"])]
    return [dict(shaf=files[".shaf"], cod=files[".cod"], decode_rle=False)]


@pytest.mark.parametrize("key,cases", GROUPS, ids=[f"b{k[0]}-c{k[1]}" for k, _ in GROUPS])
def test_drivers_agree_round_trip_and_synchronise_twice(shafa, key, cases, monkeypatch):
    import torch
    from test_gpu_pack import test_compress_files_reproduce_reference_files as reference_parity
    b, c = key
    kw = dict(force_rle=c == "r", force_freq=c == "f")
    bs = BLOCK.get(b, 65536)
    datas, sessions = [], []
    try:
        for case in cases:
            reference_parity(shafa, case)                              # compress_files equals the reference's files
            man = _manifest(case)
            data, S = _case_input(shafa, case, man, man["cmds"][0]["argv"][0])
            if S is not None:
                sessions.append(S)
            datas.append(data)
        d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
        fin = _count_calls(shafa, monkeypatch, "finish")
        res = shafa.compress_many(d_in, [d.size for d in datas], bs, **kw)
        groups = len(fin) // (1 if c == "r" else 2)
        assert len(fin) == groups * (1 if c == "r" else 2) and 1 <= groups <= 2, len(fin)
        pos = 0
        for case, data, got in zip(cases, datas, res):
            fin.clear()
            want = shafa.compress_files(d_in[pos:pos + data.size], bs, **kw)
            assert len(fin) == (1 if c == "r" else 2), (case, len(fin))
            pos += data.size
            _same_files(got, want, case)
            if data.size % bs == 1:                                    # a last block of one byte: refused as the CLI refuses it
                continue
            for args in _round_trip_args(got):
                assert _bytes(shafa.decompress_files(**args)) == data.tobytes(), (case, sorted(args))
                assert _bytes(shafa.decompress_many([args])[0]) == data.tobytes(), (case, sorted(args))
    finally:
        for S in sessions:
            S.close()


# ---------------------------------------------------------------- 14. memory
def _peak(shafa, d_in, bs):
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    files = shafa.compress_files(d_in, bs)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, files


def test_peak_memory_follows_the_measured_sizes(oracle, shafa):
    import torch
    n = 256 << 20
    # the code's own regions: encoder output c + c / 2 + 64 per block of capacity c, the .shaf / .rle files by the same
    # capacities, tile histograms 512 bytes per 32 KiB; worst-case RLE regions were 2 n + 3
    enc = lambda c: c + c // 2 + 64                                    # noqa: E731
    small = n // 32
    assert 2 * enc(n) + small < 4 * n < 5 * n < (2 * n + 3) + 2 * enc(n)                       # plain: this chain, the old one
    zt = torch.from_numpy(shafa.zipf_table(1.2)).to(_dev())
    g = torch.Generator(device=_dev())
    g.manual_seed(12)
    d_plain = zt[torch.randint(0, 65536, (n,), device=_dev(), generator=g)]
    peak, files = _peak(shafa, d_plain, M64)
    print(f"plain: peak {peak} bytes = {peak / n:.3f} n")
    assert ".shaf" in files and ".rle" not in files
    assert peak < 4 * n, f"{peak / n:.3f} n"
    del d_plain, files
    data = _run_heavy(31, n, run=96)
    r = sum(len(oracle.rle_encode(b)) for b in _cut(data, [M64] * (n // M64)))
    assert r <= 0.2 * n, r / n
    assert 2 * r + 2 * enc(r) + small < 2 * n < 2 * (2 * n + 3) + 2 * enc(2 * n + 3)           # RLE: this chain, the old one
    peak, files = _peak(shafa, torch.from_numpy(data).to(_dev()), M64)
    print(f"run-heavy: RLE {r / n:.3f} n, peak {peak} bytes = {peak / n:.3f} n")
    assert ".rle" in files and files[".rle"].numel() == r
    assert peak < 2 * n, f"{peak / n:.3f} n"


# ---------------------------------------------------------------- 15. the query
@pytest.mark.parametrize("key,cases", GROUPS, ids=[f"b{k[0]}-c{k[1]}" for k, _ in GROUPS])
def test_rle_encoded_sizes_of_golden_sessions(oracle, shafa, key, cases):
    import torch
    b, c = key
    bs = BLOCK.get(b, 65536)
    datas, sessions = [], []
    try:
        for case in cases:
            man = _manifest(case)
            data, S = _case_input(shafa, case, man, man["cmds"][0]["argv"][0])
            if S is not None:
                sessions.append(S)
            datas.append(data)
        tiny = np.full(1023, 4, dtype=np.uint8)
        d_in = torch.from_numpy(np.concatenate(datas + [tiny])).to(_dev())
        res = shafa.rle_encoded_sizes(d_in, [d.size for d in datas] + [tiny.size], bs)
        assert len(res) == len(cases) + 1
        assert isinstance(res[-1], shafa.ShafaError) and res[-1].code == shafa.FILE_TOO_SMALL
        for case, data, got in zip(cases, datas, res):
            man = _manifest(case)
            fn = man["cmds"][0]["argv"][0]
            use, sizes = got
            assert type(use) is bool and all(type(x) is int for x in sizes)
            assert sizes == [len(oracle.rle_encode(x)) for x in _cut(data, split_blocks(shafa, data.size, bs))], case
            if c != "r":                                               # -c r: the reference did not choose
                assert use == (fn + ".rle.freq" in man["files"]), case
    finally:
        for S in sessions:
            S.close()
    with pytest.raises(ValueError):
        shafa.rle_encoded_sizes(torch.zeros(4096, dtype=torch.uint8), [4096])

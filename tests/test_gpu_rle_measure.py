"""The RLE size pass (shafa_hipd_rle_decoded_size_dev, csrc/rle_measure.hip), the exact regions it gives the two decompress
drivers, and the queries built on it (shafa.decoded_sizes, shafa.decompress_range).

3. every RLE block of every golden session measures what the oracle decodes, session by session and all in one call;
4. seeded fuzz: size and code equal the oracle's and rle_decode_dev's (out_cap = RLE_DECODE_MAX) on the same inputs.  A block
   the decoder refuses keeps the size of its complete tokens in the decoder's d_out_n, the size pass (and the oracle) say 0:
   sizes are compared with the decoder's where it succeeds, codes everywhere;
5. exactly SHAFA_RLE_DECODE_MAX measures that value, one literal more is FILE_UNRECOGNIZABLE;
6. a block past its capacity is OUTSIDE_MODULE alone; nothing around d_out_n is written, the input is not changed;
7. the call only enqueues;
8. one 64 MiB block next to 2 100 blocks of 1 KiB (8 192 x 2 101 tiles x 256 lanes > 2^32) in one call;
9. the drivers decode run-heavy files in ONE rle_decode_dev call where worst-case regions took more than two groups;
10. decoded_sizes on every golden decode session, in every form it has;
11. decompress_range against slices of decompress_files' tensor."""
import os

import numpy as np
import pytest

from oracle_lib import parse_blocks_text
from test_gpu_pack import _case_input
from test_gpu_unpack import _bytes, _dev, _man, _opt, _session, _t, BLOCK, DECODED, GOLD

pytestmark = pytest.mark.gpu

SENT = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64
TILE = 8192


def _al16(n):
    return (n + 15) // 16 * 16


class _Blocks:
    """RLE streams in 16-aligned regions of one device buffer, their sizes in device memory"""

    def __init__(self, streams, caps=None):
        import torch
        self.n = [len(s) for s in streams]
        self.cap = list(caps) if caps is not None else list(self.n)
        self.off, pos = [], 0
        for c in self.cap:
            self.off.append(pos)
            pos += _al16(c) + 16
        host = np.full(pos + 16, 0xEE, dtype=np.uint8)
        for o, s in zip(self.off, streams):
            host[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s
        self.host = host
        self.d_in = torch.from_numpy(host).to(_dev())
        self.d_n = torch.tensor(self.n, dtype=torch.int64, device=_dev())


def _measure(shafa, blk, bt=None, st=None):
    """one size pass over blk -> (sizes, codes)"""
    import torch
    nb = len(blk.n)
    own = bt is None
    bt = bt or shafa.Batch(nb, 1 << 20)
    st = st or torch.cuda.Stream(device=_dev())
    try:
        d_size = torch.full((nb,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_decoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        return d_size.cpu().numpy().view(np.uint64).tolist(), errs
    finally:
        if own:
            bt.close()


def _oracle_sizes(oracle, shafa, streams):
    want_n, want_rc = [], []
    for s in streams:
        rc, out = oracle.rle_decode(s, cap=int(shafa.RLE_DECODE_MAX))
        want_rc.append(rc)
        want_n.append(out.size)
    return want_n, want_rc


# ---------------------------------------------------------------- 3. golden sessions
def _rle_cases():
    out = []
    for c in sorted(os.listdir(GOLD)):
        if os.path.exists(os.path.join(GOLD, c, "manifest.json")):
            man = _man(c)
            fn = man["cmds"][0]["argv"][0]
            if fn + ".rle" in man["files"] or fn + ".rle.shaf" in man["files"]:
                out.append(c)
    return out


RLE_CASES = _rle_cases()


def _rle_blocks(shafa, case):
    """the session's RLE streams, one per block: compress_files on its input with its options, the .rle cut by the .rle.freq"""
    import torch
    man = _man(case)
    argv = man["cmds"][0]["argv"]
    data, S = _case_input(shafa, case, man, argv[0])
    try:
        c = _opt(argv, "-c")
        files = shafa.compress_files(torch.from_numpy(data).to(_dev()), BLOCK.get(_opt(argv, "-b"), 65536),
                                     force_rle=c == "r", force_freq=c == "f")
        assert ".rle" in files and ".rle.freq" in files, (case, sorted(files))
        rle = files[".rle"].cpu().numpy()
        mode, blocks = parse_blocks_text(_bytes(files[".rle.freq"]))
        assert mode == "R"
        out, pos = [], 0
        for size, _ in blocks:
            out.append(rle[pos:pos + size])
            pos += size
        assert pos == rle.size
        return out
    finally:
        if S is not None:
            S.close()


def test_rle_case_list():
    assert len(RLE_CASES) == 20, RLE_CASES


def test_golden_sessions_measure_what_the_oracle_decodes(oracle, shafa):
    every, every_want = [], []
    for case in RLE_CASES:
        streams = _rle_blocks(shafa, case)
        want_n, want_rc = _oracle_sizes(oracle, shafa, streams)
        assert not any(want_rc), case
        got_n, got_rc = _measure(shafa, _Blocks(streams))
        assert got_rc == want_rc and got_n == want_n, f"{case}: sizes {got_n} codes {got_rc}, the oracle decodes {want_n}"
        every += streams
        every_want += want_n
    got_n, got_rc = _measure(shafa, _Blocks(every))
    assert not any(got_rc) and got_n == every_want


# ---------------------------------------------------------------- 4. fuzz
def fuzz_streams(seed=20261016):
    """byte strings that walk every path of the size pass: zero-heavy streams, ends in S1 and S2, a 0,0,0 triple, counts of
    0 / 1 / 255, lengths around 1, 2, 3, 31, 32, 33 and one tile +- 1, tile boundaries after the escape and after the symbol"""
    rng = np.random.default_rng(seed)
    out = [b"", b"\x00", b"\x05", b"\x00\x00", b"\x00\x07", b"\x07\x00", b"\x00\x00\x00", b"\x00\x09\x00", b"\x00\x09\x01",
           b"\x00\x09\xff", b"\x01\x00\x00", b"\x00\x00\x00\x00", b"\x00\x00\x00\x00\x00", b"\x00\x00\x00\x00\x00\x00"]

    def tokens(n_bytes, p_triple, p_zero):
        """about n_bytes of whole tokens"""
        b = bytearray()
        while len(b) < n_bytes:
            if rng.random() < p_triple:
                sym = 0 if rng.random() < p_zero else int(rng.integers(0, 256))
                cnt = int(rng.choice([0, 1, 255, int(rng.integers(0, 256))]))
                b += bytes([0, sym, cnt])
            else:
                b.append(int(rng.integers(1, 256)))
        return bytes(b)

    for n in (1, 2, 3, 4, 30, 31, 32, 33, 34, 63, 64, 65, 95, 96, 97, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1,
              3 * TILE + 5):
        for p, pz in ((0.0, 0.0), (0.05, 0.2), (0.5, 0.5), (1.0, 0.0), (1.0, 1.0)):
            s = tokens(n + 3, p, pz)
            out.append(s[:n])                                          # cut anywhere: may end in S1 or S2
            s = tokens(n, p, pz)
            out.append(s)                                              # whole tokens
            out.append(s + b"\x00")                                    # ends in S1
            out.append(s + b"\x00\x41")                                # ends in S2
    for lead in range(0, 6):                                           # the escape, the symbol and the count on either side
        for at in (TILE, 2 * TILE):                                    # of a tile boundary, in literal and in zero-heavy text
            for fill in (b"\x41", b"\x00\x00\x02"):
                head = (fill * (at // len(fill) + 2))[:at - lead - (at - lead) % len(fill)]
                head = b"\x42" * (at - lead - len(head)) + head
                out.append(head + b"\x00\x21\x04" * 3 + b"\x43" * 40)
                out.append(head + b"\x00\x00\x00" * 3 + b"\x00\x00\xff")
    for n in (TILE * 2 + 17, TILE * 5):                                # zero-heavy: all-zero bytes in the three alignments
        out.append(bytes(n))
        out.append(b"\x05" + bytes(n))
        out.append(b"\x05\x06" + bytes(n))
    out.append(rng.integers(0, 256, 5 * TILE + 100, dtype=np.uint8).tobytes())
    out.append((rng.integers(0, 4, 4 * TILE + 7, dtype=np.uint8) * (rng.integers(0, 2, 4 * TILE + 7, dtype=np.uint8))).tobytes())
    return out


def test_fuzz_equals_the_oracle_and_the_decoder(oracle, shafa):
    import torch
    streams = fuzz_streams()
    assert len(streams) > 400
    want_n, want_rc = _oracle_sizes(oracle, shafa, streams)
    assert set(want_rc) == {0, shafa.FILE_UNRECOGNIZABLE}
    assert any(rc == 0 and n for rc, n in zip(want_rc, want_n)) and want_rc.count(shafa.FILE_UNRECOGNIZABLE) > 50
    blk = _Blocks(streams)
    nb = len(streams)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        got_n, got_rc = _measure(shafa, blk, bt, st)
        bad = [(i, len(streams[i]), got_n[i], got_rc[i], want_n[i], want_rc[i]) for i in range(nb)
               if (got_n[i], got_rc[i]) != (want_n[i], want_rc[i])]
        assert not bad, f"(stream, bytes, size, code, oracle's size, code): {bad[:10]}"
        MAX = int(shafa.RLE_DECODE_MAX)
        room = [min(MAX, 85 * n + 2) for n in blk.n]                   # what any stream of n bytes can yield
        ooff, pos = [], 0
        for r in room:
            ooff.append(pos)
            pos += _al16(r) + 16
        d_out = torch.empty(pos + 16, dtype=torch.uint8, device=_dev())
        d_dec_n = torch.zeros(nb, dtype=torch.int64, device=_dev())
        bt.rle_decode_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_out, ooff, [MAX] * nb, d_dec_n)
        _, dec_rc = bt.finish(st, nb, raise_on_error=False)
        dec_n = d_dec_n.cpu().numpy().view(np.uint64).tolist()
        assert dec_rc == got_rc
        assert [n for n, rc in zip(dec_n, dec_rc) if rc == 0] == [n for n, rc in zip(got_n, got_rc) if rc == 0]
    finally:
        bt.close()


# ---------------------------------------------------------------- 5. the maximum
def test_the_maximum(oracle, shafa):
    MAX = int(shafa.RLE_DECODE_MAX)
    n_tr = MAX // 255
    exact = np.concatenate([np.tile(np.array([0, 1, 255], dtype=np.uint8), n_tr), np.full(MAX - 255 * n_tr, 7, dtype=np.uint8)])
    over = np.concatenate([exact, np.array([9], dtype=np.uint8)])
    got_n, got_rc = _measure(shafa, _Blocks([exact, over, exact[:3 * 1000]]))
    assert got_rc == [0, shafa.FILE_UNRECOGNIZABLE, 0], got_rc
    assert got_n == [MAX, 0, 255 * 1000], got_n


# ---------------------------------------------------------------- 6. capacities, sentinels, the input
def test_a_block_past_its_capacity_fails_alone(oracle, shafa):
    import torch
    streams = [bytes([65, 0, 66, 9] * 700), bytes([1, 2, 3] * 3000), bytes([0, 5, 0, 0, 0, 200] * 2000), b""]
    want_n, _ = _oracle_sizes(oracle, shafa, streams)
    blk = _Blocks(streams)
    blk.d_n[1] = blk.cap[1] + 1
    before = blk.d_in.clone()
    nb = len(streams)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        words = torch.full((nb + 8,), SENT, dtype=torch.int64, device=_dev())
        bt.rle_decoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, words[4:4 + nb])
        _, errs = bt.finish(st, nb, raise_on_error=False)
        w = words.cpu().tolist()
        assert errs == [0, shafa.OUTSIDE_MODULE, 0, 0], errs
        assert w[4:4 + nb] == [want_n[0], 0, want_n[2], 0], w
        assert w[:4] == [SENT] * 4 and w[4 + nb:] == [SENT] * 4
        assert torch.equal(blk.d_in, before)
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. enqueue only
def test_the_call_only_enqueues(shafa):
    import torch
    rng = np.random.default_rng(5)
    streams = [rng.integers(1, 256, 70000, dtype=np.uint8) for _ in range(6)]
    blk = _Blocks(streams)
    nb = len(streams)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        d_size = torch.zeros(nb, dtype=torch.int64, device=_dev())
        bt.rle_decoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size)     # warm-up: the batch grows here
        bt.finish(st, nb)
        want = d_size.cpu().tolist()
        assert want == [70000] * nb
        d_size.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)
        bt.rle_decoded_size_dev(st, blk.d_in, blk.off, blk.cap, blk.d_n, d_size)
        busy = not st.query()
        bt.finish(st, nb)
        assert busy, "the stream had drained when the call returned: something synchronised"
        assert d_size.cpu().tolist() == want
    finally:
        bt.close()


# ---------------------------------------------------------------- 8. the grid
def test_one_large_block_among_thousands_of_small_ones(oracle, shafa):
    big_n = 64 << 20
    pat = np.concatenate([np.arange(1, 62, dtype=np.uint8), np.array([0, 9, 3], dtype=np.uint8)])    # 64 bytes in, 64 out
    big = np.concatenate([np.array([70, 71], dtype=np.uint8), np.tile(pat, big_n // 64 - 1)])         # triples straddle tiles
    rng = np.random.default_rng(8)
    small = []
    for i in range(2100):
        s = rng.integers(0, 256, 1024, dtype=np.uint8)
        s[rng.random(1024) < 0.3] = 0
        small.append(s)
    streams = small[:1000] + [big] + small[1000:]
    caps = [1024] * 1000 + [big_n] + [1024] * 1100
    assert (big_n // TILE) * len(streams) * 256 > 1 << 32
    want_n, want_rc = _oracle_sizes(oracle, shafa, streams)
    assert want_n[1000] == 2 + (big_n // 64 - 1) * 64 and want_rc[1000] == 0
    got_n, got_rc = _measure(shafa, _Blocks(streams, caps))
    assert got_rc == want_rc
    assert got_n == want_n


# ---------------------------------------------------------------- 9. the drivers take exact regions
def _run_heavy(seed, n, run=96):
    rng = np.random.default_rng(seed)
    syms = rng.integers(1, 256, n // run + 1, dtype=np.uint8)
    syms[1:][syms[1:] == syms[:-1]] ^= 1                               # neighbours differ (1 ^ 1 = 0 is a symbol like any other)
    return np.repeat(syms, run)[:n].copy()


def _count_calls(shafa, monkeypatch, name):
    calls = []
    real = getattr(shafa.Batch, name)

    def wrapper(self, *a, **k):
        calls.append(a)
        return real(self, *a, **k)

    monkeypatch.setattr(shafa.Batch, name, wrapper)
    return calls


def _worst(shafa, n):
    return _al16(min(int(shafa.RLE_DECODE_MAX), 85 * n + 2))


def test_decompress_many_decodes_run_heavy_files_in_one_call(shafa, monkeypatch):
    import torch
    F, N = 64, 65536
    datas = [_run_heavy(100 + i, N) for i in range(F)]
    sets = shafa.compress_many(torch.from_numpy(np.concatenate(datas)).to(_dev()), [N] * F, N, force_rle=True)
    rle_n = [s[".rle"].numel() for s in sets]                          # one block a file: the .rle is the block
    max_bytes = F * _al16(N)
    assert sum(_al16(N) for _ in range(F)) <= max_bytes
    assert sum(_worst(shafa, n) for n in rle_n) > 2 * max_bytes, rle_n[:4]
    calls = _count_calls(shafa, monkeypatch, "rle_decode_dev")
    res = shafa.decompress_many([dict(rle=s[".rle"], freq=s[".rle.freq"]) for s in sets], max_bytes=max_bytes)
    assert len(calls) == 1, len(calls)
    assert all(_bytes(r) == d.tobytes() for r, d in zip(res, datas))
    calls.clear()
    res = shafa.decompress_many([dict(shaf=s[".rle.shaf"], cod=s[".rle.cod"]) for s in sets], max_bytes=max_bytes)
    assert len(calls) == 1, len(calls)
    assert all(_bytes(r) == d.tobytes() for r, d in zip(res, datas))


def test_decompress_files_decodes_a_run_heavy_file_in_one_call(shafa, monkeypatch):
    import torch
    NB, N = 12, 65536
    data = _run_heavy(7, NB * N)
    files = shafa.compress_files(torch.from_numpy(data).to(_dev()), N, force_rle=True)
    mode, blocks = parse_blocks_text(_bytes(files[".rle.freq"]))
    rle_n = [size for size, _ in blocks]
    assert mode == "R" and len(rle_n) == NB
    max_bytes = NB * _al16(N)
    assert sum(_worst(shafa, n) for n in rle_n) > 2 * max_bytes, rle_n
    calls = _count_calls(shafa, monkeypatch, "rle_decode_dev")
    out = shafa.decompress_files(rle=files[".rle"], freq=files[".rle.freq"], max_bytes=max_bytes)
    assert len(calls) == 1, len(calls)
    assert _bytes(out) == data.tobytes()
    calls.clear()
    out = shafa.decompress_files(shaf=files[".rle.shaf"], cod=files[".rle.cod"], max_bytes=max_bytes)
    assert len(calls) == 1, len(calls)
    assert _bytes(out) == data.tobytes()


# ---------------------------------------------------------------- 10. decoded_sizes
def _forms(files):
    """the forms a compress_files result can be asked in -> [(name, arguments of the queries, decode_rle of decompress_files)]"""
    if ".rle" in files:
        return [("rle + freq", dict(rle=files[".rle"], freq=files[".rle.freq"]), {}),
                ("shaf + cod, mode R", dict(shaf=files[".rle.shaf"], cod=files[".rle.cod"]), dict(decode_rle=True))]
    return [("shaf + cod, mode N", dict(shaf=files[".shaf"], cod=files[".cod"]), dict(decode_rle=False))]


def _cut(buf, sizes):
    out, pos = [], 0
    for n in sizes:
        out.append(buf[pos:pos + n])
        pos += n
    assert pos == len(buf)
    return out


@pytest.mark.parametrize("case", DECODED)
def test_decoded_sizes_of_golden_sessions(oracle, shafa, case, monkeypatch):
    import torch
    man = _man(case)
    argv = man["cmds"][0]["argv"]
    data, S = _case_input(shafa, case, man, argv[0])
    try:
        c = _opt(argv, "-c")
        files = shafa.compress_files(torch.from_numpy(data).to(_dev()), BLOCK.get(_opt(argv, "-b"), 65536),
                                     force_rle=c == "r", force_freq=c == "f")
        del data
        for name, args, kw in _forms(files):
            try:
                whole = shafa.decompress_files(**args, **kw).numel()
            except shafa.ShafaError as e1:             # test_gpu_unpack: a last block of one byte, refused as the CLI refuses it
                with pytest.raises(shafa.ShafaError) as e2:
                    shafa.decoded_sizes(**args)
                assert e2.value.code == e1.code == shafa.FILE_UNRECOGNIZABLE, (case, name)
                continue
            if "mode N" in name:
                mode, blocks = parse_blocks_text(_bytes(files[".cod"]))
                assert mode == "N"
                want = [size for size, _ in blocks]
                sf_calls = _count_calls(shafa, monkeypatch, "sf_decode_dev")
                up_calls = _count_calls(shafa, monkeypatch, "unpack_payloads")
                got = shafa.decoded_sizes(**args)
                assert not sf_calls and not up_calls, (case, len(sf_calls), len(up_calls))
                monkeypatch.undo()
            else:
                mode, blocks = parse_blocks_text(_bytes(files[".rle.freq"]))
                rle = files[".rle"].cpu().numpy()
                want = [oracle.rle_decode(s, cap=int(shafa.RLE_DECODE_MAX))[1].size for s in _cut(rle, [n for n, _ in blocks])]
                got = shafa.decoded_sizes(**args)
            assert all(type(n) is int for n in got)
            assert got == want, f"{case}, {name}: {got[:8]} != {want[:8]}"
            assert sum(got) == whole, (case, name)
    finally:
        if S is not None:
            S.close()


# ---------------------------------------------------------------- 11. decompress_range
def _ranges(total, bs):
    r = [(5, 100), (bs - 10, 9), (bs - 7, 7), (bs - 3, 10), (bs, 1), (bs + 1, 3 * bs), (2 * bs - 1, 2 * bs + 2),
         (0, 1), (total - 1, 1), (0, total), (0, total + 1000), (total - 5, 50), (total, 10), (total + 7, 10), (17, 0), (total, 0)]
    return [(o, n) for o, n in r if o >= 0]


def _check_ranges(shafa, args, kw, bs, monkeypatch, label):
    whole = shafa.decompress_files(**args, **kw)
    total = whole.numel()
    host = whole.cpu().numpy()
    for off, n in _ranges(total, bs):
        calls = _count_calls(shafa, monkeypatch, "sf_decode_dev") if kw.get("decode_rle") is False else None
        got = shafa.decompress_range(off, n, **args)
        assert got.dtype == whole.dtype and got.is_cuda
        assert got.cpu().numpy().tobytes() == host[off:off + n].tobytes(), f"{label}: [{off}, {off + n}) of {total}"
        if calls is not None:
            lo, hi = min(off, total), min(off + n, total)
            cover = 0 if lo >= hi else (hi - 1) // bs - lo // bs + 1     # mode N: every block but the last has bs bytes
            assert sum(len(a[2]) for a in calls) == cover and len(calls) == (1 if cover else 0), (label, off, n, cover)
            monkeypatch.undo()
    return total


@pytest.mark.parametrize("case", ["runs_default", "edges_forced_rle", "uniform_no_rle", "textlike_m"])
def test_decompress_range_on_golden_sessions(shafa, case, monkeypatch):
    import torch
    man = _man(case)
    argv = man["cmds"][0]["argv"]
    data, S = _case_input(shafa, case, man, argv[0])
    assert S is None
    bs = BLOCK.get(_opt(argv, "-b"), 65536)
    c = _opt(argv, "-c")
    files = shafa.compress_files(torch.from_numpy(data).to(_dev()), bs, force_rle=c == "r", force_freq=c == "f")
    for name, args, kw in _forms(files):
        assert _check_ranges(shafa, args, kw, bs, monkeypatch, f"{case}, {name}") == data.size


def test_decompress_range_on_a_round_trip(shafa, monkeypatch):
    rle, plain = _session(shafa)                                       # 5 blocks of 64 KiB and 300 bytes, both kinds
    seen = set()
    for files in (rle, plain):
        for name, args, kw in _forms({k: _t(v, 3) for k, v in files.items()}):
            assert _check_ranges(shafa, args, kw, 65536, monkeypatch, name) == 5 * 65536 + 300
            seen.add(name)
    assert len(seen) == 3
    with pytest.raises(ValueError):
        shafa.decompress_range(-1, 5, shaf=_t(plain[".shaf"]), cod=_t(plain[".cod"]))
    with pytest.raises(ValueError):
        shafa.decompress_range(0, -5, shaf=_t(plain[".shaf"]), cod=_t(plain[".cod"]))


def test_decompress_range_raises_for_damage_inside_the_range(shafa):
    rle, _ = _session(shafa)
    mode, blocks = parse_blocks_text(rle[".rle.freq"])
    sizes = [n for n, _ in blocks]
    end2 = sum(sizes[:3])                                              # block 2 is made to end inside a triple
    bad = bytearray(rle[".rle"])
    bad[end2 - 4:end2] = b"\x41\x41\x41\x00"                        # whatever the state in front of them: ends in S1
    args = dict(rle=_t(bytes(bad)), freq=_t(rle[".rle.freq"]))
    with pytest.raises(shafa.ShafaError) as e1:
        shafa.decompress_files(**args)
    with pytest.raises(shafa.ShafaError) as e2:
        shafa.decompress_range(2 * 65536 + 100, 1000, **args)
    assert e1.value.code == e2.value.code == shafa.FILE_UNRECOGNIZABLE
    with pytest.raises(shafa.ShafaError) as e3:
        shafa.decoded_sizes(**args)
    assert e3.value.code == shafa.FILE_UNRECOGNIZABLE

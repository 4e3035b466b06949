"""shafa.build_index / read_ranges / read_range: a seek index over a file set in device memory, and byte ranges read through it.

1. index values against the CPU, every checkpoint: bit offsets = the cumulative sum of the oracle table's len[] over the
   SF-decoded bytes (8 a byte for .rle + .freq); states, pending symbols and decoded offsets = a plain Python walk of the .rle bytes;
2. shapes the checkpoints must land on, built by hand on a runs stream and asserted from the CPU walk to occur: a checkpoint in
   state 1, one in state 2 (the pending symbol matters), a count byte of 0, a block of an exact multiple of span, a block
   shorter than span, several {0, s, 255} triples whose output holds a 100-byte range inside one span; a block of one distinct
   symbol has an empty payload, which Module D refuses in a .shaf (tests/test_gpu_unpack.py): build_index raises what
   decompress_files raises for it;
3. reads: a fixed list and 200 seeded ranges in one call, against slices of the input and of decompress_files;
4. a block whose table holds a 40-bit code is unindexed and read through the block decoders;
5. faults: damaged sets raise decompress_files' code from build_index; payload bytes overwritten after indexing give bytes or
   ShafaError, and the guard bytes around out stay untouched;
6. the shape of the call: one synchronisation, a launch count and a peak allocation that do not grow with ranges / block size."""
import ctypes as C

import numpy as np
import pytest

import pkgload
from test_gpu_rle_measure import _count_calls
from test_gpu_unpack import _bytes, _dev, _t

pytestmark = pytest.mark.gpu

BS = 4096
_SETS = {}


def _text_file(mode, sizes, texts):
    """a .cod / .freq: "@<mode>@<n>", "@<size>@<text>" per block, "@0" """
    out = b"@" + mode + b"@" + str(len(sizes)).encode()
    for n, t in zip(sizes, texts):
        out += b"@" + str(n).encode() + b"@" + t
    return out + b"@0"


def _lens(table):
    return np.frombuffer(bytes(table.len), dtype=np.uint8).astype(np.int64)


def _synth():
    return pkgload.load_submodule("synth")


def _blocks(data, bs):
    return [data[a:a + bs] for a in range(0, len(data), bs)]


def _sets(shafa, oracle, n, bs):
    """name -> (original bytes, file arguments, per block (SF-decoded bytes, len[] of its table)), made once"""
    import torch
    if (n, bs) not in _SETS:
        synth = _synth()
        zt = synth.zipf_table(1.2)
        plain, runs = synth.gen_bytes(31 + n, n, zt), synth.runs_stream(32 + n, n, zt)
        fp = shafa.compress_files(torch.from_numpy(plain).to(_dev()), bs)
        fr = shafa.compress_files(torch.from_numpy(runs).to(_dev()), bs, force_rle=True)
        assert ".shaf" in fp and ".rle.shaf" in fr
        lens = lambda b: _lens(oracle.sf_build(oracle.hist256(b)))
        rle = [oracle.rle_encode(b) for b in _blocks(runs, bs)]
        eight = np.full(256, 8, dtype=np.int64)
        _SETS[(n, bs)] = {
            "N": (plain, dict(shaf=fp[".shaf"], cod=fp[".cod"]), [(b, lens(b)) for b in _blocks(plain, bs)]),
            "rle+freq": (runs, dict(rle=fr[".rle"], freq=fr[".rle.freq"]), [(r, eight) for r in rle]),
            "R": (runs, dict(shaf=fr[".rle.shaf"], cod=fr[".rle.cod"]), [(r, lens(r)) for r in rle])}
    return _SETS[(n, bs)]


def _walk(rle, span):
    """the RLE machine over .rle bytes -> per checkpoint (state, pending symbol, decoded offset), and the decoded size"""
    out, state, off = [], 0, 0
    for i, v in enumerate(rle.tolist()):
        if i % span == 0:
            out.append((state, int(rle[i - 1]) if state == 2 else 0, off))
        if state == 0:
            if v:
                off += 1
            else:
                state = 1
        elif state == 1:
            state = 2
        else:
            off += v if v else 1
            state = 0
    assert state == 0
    return out or [(0, 0, 0)], off


def _expected(blocks, span, is_rle):
    """the index's words and block table from the CPU: [(w0, w1)] over all blocks, [(decoded size, symbols, first checkpoint)]"""
    words, table = [], []
    for sfb, lens in blocks:
        bits = np.concatenate([[0], np.cumsum(lens[sfb])])
        n = len(sfb)
        ck, size = _walk(sfb, span) if is_rle else ([(0, 0, k) for k in range(0, max(n, 1), span)], n)
        assert len(ck) == max(1, -(-n // span))
        table.append((size, n, len(words)))
        for k, (state, pend, off) in enumerate(ck):
            words.append((int(bits[k * span]) | pend << 48 | state << 56, off))
    return words, table


def _check_index(idx, blocks, span, is_rle):
    words, table = _expected(blocks, span, is_rle)
    got = idx.checkpoints.cpu().numpy().view(np.uint64).reshape(-1, 2)
    assert got.shape[0] == len(words)
    want = np.array(words, dtype=np.uint64)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not bad.size, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert [(b.decoded_size, b.n_symbols, b.first_checkpoint) for b in idx.blocks] == table
    assert all(b.indexed for b in idx.blocks) and idx.span == span
    assert idx.decoded_size == sum(t[0] for t in table)


def _ranges(n, bs, span, seed):
    """the fixed list, then 200 seeded ranges of 0 to 3 blocks"""
    fixed = [(0, 0), (n // 2, 0), (0, 1), (n - 1, 1), (span - 3, 7), (bs - 5, 11), (n - 10, 50), (n + 5, 3), (0, n), (0, n + 9),
             (100, 300), (250, 300)]
    rng = np.random.default_rng(seed)
    return fixed + [(int(rng.integers(0, n)), int(rng.integers(0, 3 * bs + 1))) for _ in range(200)]


def _check_reads(shafa, idx, data, kw, ranges, full=None):
    out, offs = shafa.read_ranges(idx, ranges, **kw)
    got = out.cpu().numpy()
    assert len(offs) == len(ranges) + 1 and offs[0] == 0 and offs[-1] == got.size
    for i, (o, n) in enumerate(ranges):
        want = data[o:o + n]
        assert offs[i + 1] - offs[i] == want.size, (i, o, n)
        assert got[offs[i]:offs[i + 1]].tobytes() == want.tobytes(), (i, o, n)
        if full is not None:
            assert want.tobytes() == full[o:o + n].tobytes()
    for o, n in ranges[:8]:
        assert _bytes(shafa.read_range(idx, o, n, **kw)) == data[o:o + n].tobytes(), (o, n)


@pytest.mark.parametrize("span", [256, 1024])
@pytest.mark.parametrize("n", [3 * BS + 33, 1024])
def test_index_and_reads_against_the_cpu(shafa, oracle, n, span):
    for name, (data, kw, blocks) in _sets(shafa, oracle, n, BS).items():
        idx = shafa.build_index(span=span, **kw)
        assert idx.mode == {"N": "N", "R": "R", "rle+freq": "rle"}[name]
        assert idx.file_lengths == tuple(v.numel() for v in kw.values())
        _check_index(idx, blocks, span, name != "N")
        full = shafa.decompress_files(decode_rle=name != "N", **kw).cpu().numpy()
        assert full.tobytes() == data.tobytes()
        _check_reads(shafa, idx, data, kw, _ranges(n, BS, span, 7 + span), full)
        if n > BS:                                                   # groups of one block give the same index
            again = shafa.build_index(span=span, max_bytes=1, **kw)
            assert (again.checkpoints == idx.checkpoints).all() and again.blocks == idx.blocks


def test_large_blocks_span_8192(shafa, oracle):
    n, bs, span = 3 * 65536 + 777, 65536, 8192
    for name, (data, kw, blocks) in _sets(shafa, oracle, n, bs).items():
        idx = shafa.build_index(span=span, **kw)
        _check_index(idx, blocks, span, name != "N")
        _check_reads(shafa, idx, data, kw, _ranges(n, bs, span, 99))


# ---------------------------------------------------------------- 2. shapes made by hand
SPAN = 256


def _hand_blocks():
    rng = np.random.default_rng(5)
    lit = lambda k: rng.integers(1, 256, k).astype(np.uint8)
    tri = lambda s, c: np.array([0, s, c], dtype=np.uint8)
    a = np.concatenate([lit(254), tri(7, 0), lit(2 * SPAN - 257)])                   # 512 bytes: checkpoint 1 in state 2, count 0
    b = np.concatenate([lit(255), tri(9, 200)] + [tri(5, 255)] * 90 + [lit(172)])    # checkpoint 1 in state 1; 90 long runs
    c = lit(100)                                                                   # shorter than span
    return [a, b, c]


def _rld(rle):
    out, i, v = [], 0, rle.tolist()
    while i < len(v):
        if v[i]:
            out.append(v[i])
            i += 1
        else:
            out += [v[i + 1]] * (v[i + 2] or 1)
            i += 3
    return np.array(out, dtype=np.uint8)


def _hand_files(shafa, blocks):
    """hand-made .rle blocks with their .freq, and the .shaf + .cod that Modules T and C make of them"""
    rle = np.concatenate(blocks)
    freq = _text_file(b"R", [len(b) for b in blocks],
                      [shafa.freq_format(np.bincount(b, minlength=256).astype(np.uint64)) for b in blocks])
    d_rle, d_freq = _t(rle.tobytes(), 3), _t(freq)
    cod = shafa.build_cod(d_freq)
    shaf = shafa.encode_files(d_rle, cod)
    data = np.concatenate([_rld(b) for b in blocks])
    tabs = [shafa.cod_parse(t) for t in _bytes(cod).split(b"@")[4::2] if t]
    assert all(rc == 0 for rc, _ in tabs)
    return blocks, data, dict(rle=d_rle, freq=d_freq), dict(shaf=shaf, cod=cod), [_lens(t) for _, t in tabs]


@pytest.fixture(scope="module")
def hand(shafa):
    return _hand_files(shafa, _hand_blocks())


def test_the_shapes_occur(hand):
    blocks = hand[0]
    cks = [_walk(b, SPAN)[0] for b in blocks]
    assert cks[0][1][:2] == (2, 7) and blocks[0][SPAN] == 0                # state 2, pending 7, and the count byte is 0
    assert cks[1][1][0] == 1                                               # state 1
    assert len(blocks[0]) == 2 * SPAN and len(cks[0]) == 2                 # an exact multiple of span
    assert len(blocks[2]) < SPAN and len(cks[2]) == 1                      # shorter than span
    # span 1 of block 1 is {0, 5, 255} triples nearly throughout: its output holds 100-byte ranges whole
    assert len(cks[1]) == 3 and cks[1][2][2] - cks[1][1][2] > 20000
    assert {c[0] for ck in cks for c in ck} == {0, 1, 2}


@pytest.mark.parametrize("form", ["rle+freq", "R"])
def test_hand_made_shapes(shafa, hand, form):
    blocks, data, kw_rle, kw_sf, lens = hand
    kw = kw_rle if form == "rle+freq" else kw_sf
    assert len(lens) == 3
    full = shafa.decompress_files(**kw).cpu().numpy()
    assert full.tobytes() == data.tobytes()
    idx = shafa.build_index(span=SPAN, **kw)
    eight = np.full(256, 8, dtype=np.int64)
    _check_index(idx, [(b, eight if form == "rle+freq" else l) for b, l in zip(blocks, lens)], SPAN, True)
    s1 = idx.starts[1]
    c1 = _walk(blocks[1], SPAN)[0][1][2]
    inside = [(s1 + c1 + 300, 100), (s1 + c1 + 254, 100), (s1 + c1 + 5000, 100)]           # inside one span's runs
    seams = [(idx.starts[1] - 3, 6), (idx.starts[2] - 50, 100), (250, 10), (253, 1), (254, 1), (255, 3)]
    _check_reads(shafa, idx, data, kw, inside + seams + _ranges(len(data), 4096, SPAN, 3), full)


def test_a_block_of_one_symbol_is_refused_as_by_module_d(shafa):
    import torch
    zt = _synth().zipf_table(1.2)
    data = np.concatenate([_synth().gen_bytes(3, BS, zt), np.full(BS, 120, dtype=np.uint8)])
    f = shafa.compress_files(torch.from_numpy(data).to(_dev()), BS)
    kw = dict(shaf=f[".shaf"], cod=f[".cod"])
    assert b"@0@" in _bytes(kw["shaf"])                                     # the empty payload
    with pytest.raises(shafa.ShafaError) as want:
        shafa.decompress_files(decode_rle=False, **kw)
    with pytest.raises(shafa.ShafaError) as got:
        shafa.build_index(**kw)
    assert got.value.code == want.value.code == shafa.FILE_UNRECOGNIZABLE


# ---------------------------------------------------------------- 4. unindexed blocks
def test_a_40_bit_code_is_read_by_the_block_decoders(shafa, oracle):
    import torch
    zt = _synth().zipf_table(1.2)
    rng = np.random.default_rng(11)
    mid = rng.choice(np.array([65, 66, 67, 68], dtype=np.uint8), 3000, p=[0.6, 0.25, 0.1, 0.05])
    blocks = [_synth().gen_bytes(41, 4096, zt), mid, _synth().gen_bytes(42, 2500, zt)]
    codes = [""] * 256
    codes[65], codes[66], codes[67], codes[68], codes[69] = "0", "10", "110", "111" + "0" * 37, "111" + "0" * 36 + "1"
    tabs = [shafa.sf_build_codes(oracle.hist256(blocks[0])), shafa.CodeTable.from_strings(codes),
            shafa.sf_build_codes(oracle.hist256(blocks[2]))]
    data = np.concatenate(blocks)
    cod = _t(_text_file(b"N", [len(b) for b in blocks], [shafa.cod_format(t) for t in tabs]))
    shaf = shafa.encode_files(torch.from_numpy(data).to(_dev()), cod)
    kw = dict(shaf=shaf, cod=cod)
    assert shafa.decompress_files(decode_rle=False, **kw).cpu().numpy().tobytes() == data.tobytes()
    idx = shafa.build_index(span=256, **kw)
    assert [b.indexed for b in idx.blocks] == [True, False, True]
    ck = idx.checkpoints.cpu().numpy().view(np.uint64).reshape(-1, 2)
    f1 = idx.blocks[1].first_checkpoint
    assert (ck[f1] == 0).all() and (ck[f1 + 1:idx.blocks[2].first_checkpoint] == 0).all()   # checkpoint 0 only
    ranges = [(4096, 3000), (5000, 17), (4000, 200), (7000, 300), (0, len(data)), (4095, 2), (7095, 2)]
    _check_reads(shafa, idx, data, kw, ranges + _ranges(len(data), 4096, 256, 21))


# ---------------------------------------------------------------- 5. faults
def test_build_index_raises_what_decompress_files_raises(shafa, oracle):
    sets = _sets(shafa, oracle, 3 * BS + 33, BS)
    _, kw, _ = sets["N"]
    shaf, cod = _bytes(kw["shaf"]), _bytes(kw["cod"])
    cases = [("cut .shaf", dict(kw, shaf=_t(shaf[:len(shaf) - 100], 1)), False),
             ("truncated .cod", dict(kw, cod=_t(cod[:len(cod) * 3 // 5])), False)]
    start = len(shaf) * 2 // 5
    for i in range(start, start + 4000, 37):
        bad = dict(kw, shaf=_t(shaf[:i] + bytes([shaf[i] ^ 0xFF]) + shaf[i + 1:], 2))
        try:
            shafa.decompress_files(decode_rle=False, **bad)
        except shafa.ShafaError:
            cases.append(("flipped payload byte", bad, False))
            break
    _, kw_r, _ = sets["R"]
    cod_r = _bytes(kw_r["cod"])
    cases.append(("truncated mode-R .cod", dict(kw_r, cod=_t(cod_r[:len(cod_r) * 3 // 5])), True))
    _, kw_f, _ = sets["rle+freq"]
    freq = _bytes(kw_f["freq"])
    cases.append(("truncated .rle.freq", dict(kw_f, freq=_t(freq[:len(freq) - 9])), True))
    cases.append(("cut .rle", dict(kw_f, rle=_t(_bytes(kw_f["rle"])[:-50])), True))
    rle = bytearray(_bytes(kw_f["rle"]))
    rle[-2:] = b"\x00\x07"                                                  # the stream ends inside a triple
    cases.append(("open triple", dict(kw_f, rle=_t(bytes(rle))), True))
    assert len(cases) >= 6
    for what, bad, decode_rle in cases:
        with pytest.raises(shafa.ShafaError) as want:
            shafa.decompress_files(decode_rle=decode_rle, **bad)
        for mb in (None, 1):
            with pytest.raises(shafa.ShafaError) as got:
                shafa.build_index(max_bytes=mb, **bad)
            assert got.value.code == want.value.code, (what, mb, got.value, want.value)


@pytest.mark.parametrize("name", ["N", "R", "rle+freq"])
def test_overwritten_payloads_give_bytes_or_an_error(shafa, oracle, name, monkeypatch):
    n = 3 * BS + 33
    data, kw, _ = _sets(shafa, oracle, n, BS)[name]
    idx = shafa.build_index(span=256, **kw)
    _overwrite_payloads(shafa, monkeypatch, name, kw, idx, n, _ranges(n, BS, 256, 5), range(6))


def _overwrite_payloads(shafa, monkeypatch, name, kw, idx, n, ranges, trials):
    """per trial: 64 payload bytes of one block overwritten after indexing, one read_ranges call over `ranges` whose out lies
    inside guard bytes -> bytes or FILE_UNRECOGNIZABLE, and the guards are what they were"""
    import torch
    pay = "shaf" if "shaf" in kw else "rle"
    want_n = sum(min(o + k, n) - min(o, n) for o, k in ranges)
    guard = 4096
    real_empty = torch.empty
    made = []

    def empty(*a, **k):                                                    # out, inside guard bytes
        if a and a[0] == want_n and k.get("dtype") == torch.uint8 and not made:
            made.append(torch.full((want_n + 2 * guard,), 0xA5, dtype=torch.uint8, device=k["device"]))
            return made[0][guard:guard + want_n]
        return real_empty(*a, **k)

    rng = np.random.default_rng(17)
    outcomes = set()
    for trial in trials:
        raw = bytearray(_bytes(kw[pay]))
        blk = idx.blocks[trial % len(idx.blocks)]
        a = blk.payload_offset + int(rng.integers(0, max(1, blk.payload_size - 64)))
        fill = [bytes(64), b"\xff" * 64, rng.integers(0, 256, 64).astype(np.uint8).tobytes()][trial % 3]
        raw[a:a + 64] = fill[:max(0, min(64, blk.payload_offset + blk.payload_size - a))]
        assert len(raw) == kw[pay].numel()
        bad = dict(kw, **{pay: _t(bytes(raw), 1)})
        made.clear()
        monkeypatch.setattr(torch, "empty", empty)
        try:
            out, offs = shafa.read_ranges(idx, ranges, **bad)
            assert out.numel() == want_n == offs[-1]
            outcomes.add("bytes")
        except shafa.ShafaError as e:
            assert e.code == shafa.FILE_UNRECOGNIZABLE, e
            outcomes.add("error")
        finally:
            monkeypatch.setattr(torch, "empty", real_empty)
        torch.cuda.synchronize()
        assert made, "out was not allocated through the guard"
        g = made[0].cpu().numpy()
        assert (g[:guard] == 0xA5).all() and (g[guard + want_n:] == 0xA5).all(), (name, trial)
    print(name, sorted(outcomes))


# ---------------------------------------------------------------- 6. the shape of the call
def test_one_synchronisation_and_launches_that_do_not_grow(shafa, oracle, monkeypatch):
    n = 3 * BS + 33
    for name in ("N", "R", "rle+freq"):
        data, kw, _ = _sets(shafa, oracle, n, BS)[name]
        idx = shafa.build_index(**kw)
        counts = {}
        for k in ("finish", "read_spans_dev", "unpack_cod", "sf_decode_dev", "rle_decode_dev", "unpack_payloads", "pack_payloads"):
            counts[k] = _count_calls(shafa, monkeypatch, k)
        seen = []
        for ranges in (_ranges(n, BS, 1024, 1)[:3], _ranges(n, BS, 1024, 1)):
            for c in counts.values():
                c.clear()
            shafa.read_ranges(idx, ranges, **kw)
            seen.append({k: len(c) for k, c in counts.items()})
        want = dict(finish=1, read_spans_dev=1, unpack_cod=0 if name == "rle+freq" else 1, sf_decode_dev=0, rle_decode_dev=0,
                    unpack_payloads=0, pack_payloads=0)
        assert seen[0] == seen[1] == want, (name, seen)
        monkeypatch.undo()


def test_peak_allocation_does_not_grow_with_the_block_size(shafa, oracle):
    import torch
    peaks = {}
    for n, bs in ((3 * BS + 33, BS), (3 * 65536 + 777, 65536)):
        for name in ("N", "R"):
            data, kw, _ = _sets(shafa, oracle, n, bs)[name]
            idx = shafa.build_index(span=1024, **kw)
            ranges = [(n // 2, 500), (17, 300), (n - 400, 400)]
            shafa.read_ranges(idx, ranges, **kw)                             # warm-up: code objects
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out, _ = shafa.read_ranges(idx, ranges, **kw)
            torch.cuda.synchronize()
            tables = (kw["cod"].numel() // 258 + 1) * (C.sizeof(shafa.CodeTable) + 8)
            peaks[(name, bs)] = torch.cuda.max_memory_allocated() - base - out.numel() - tables
            assert out.cpu().numpy().tobytes() == b"".join(data[o:o + k].tobytes() for o, k in ranges)
    print(peaks)
    for name in ("N", "R"):
        assert peaks[(name, 65536)] <= peaks[(name, BS)] + 4096, peaks       # nothing proportional to a block

"""shafa.verify_files: does a file set held in device memory still decode to its original?  The oracle is the existing
driver: with out = decompress_files(the same files), verify_files raises what that call raises, and otherwise returns
Verify(out == d_in, the first index at which they differ (the smaller length when one is a prefix of the other), out.numel()).

1. every golden session that stores its input next to a .shaf + .cod or a .rle + .freq of it: Verify(True, None, len(input));
2. synthetic sets (compress_files on synth streams: Zipf for mode N, a runs stream with force_rle for mode R) of 1024,
   3 x 4096 + 1, 3 x 4096 + 33 and 5 x 65536 + 15 bytes, in all three file forms, at max_bytes = default, 65536 and 1: the
   same answers.  At 3 x 4096 + 1 the last block is one byte, a block of one symbol, which Module D refuses in a .shaf
   (tests/test_gpu_unpack.py): where decompress_files raises for that, verify_files raises the same, whatever d_in holds;
3. planted differences: first_diff is exact;
4. d_in shorter, longer, empty, and at storage offset 3;
5. faulty files raise decompress_files' code, with or without a difference in d_in;
6. no decoded file: the peak stays half a decoded size below decompress_files', no pack runs, and the synchronisations are
   the parse's and the measure's (as in decompress_files), one per mode-N group, and one at the end of the RLE groups."""
import json
import os

import numpy as np
import pytest

import pkgload
from test_gpu_rle_measure import _count_calls
from test_gpu_unpack import GOLD, _bytes, _dev, _t

pytestmark = pytest.mark.gpu


def _oracle(shafa, d_in, **kw):
    """the definition: from decompress_files and a comparison on the host -> a Verify, or the ShafaError it raises"""
    try:
        out = shafa.decompress_files(**kw)
    except shafa.ShafaError as e:
        return e
    a, b = out.cpu().numpy(), d_in.cpu().numpy().reshape(-1)
    m = min(a.size, b.size)
    d = np.flatnonzero(a[:m] != b[:m])
    if a.size == b.size and not d.size:
        return shafa.Verify(True, None, a.size)
    return shafa.Verify(False, int(d[0]) if d.size else m, a.size)


def _same(shafa, d_in, want=None, **kw):
    """verify_files(d_in, **kw) against the oracle (or `want`, an oracle's answer for the same arguments) -> the answer"""
    if want is None:
        want = _oracle(shafa, d_in, **{k: v for k, v in kw.items() if k != "max_bytes"})
    if isinstance(want, shafa.ShafaError):
        with pytest.raises(shafa.ShafaError) as e:
            shafa.verify_files(d_in, **kw)
        assert e.value.code == want.code, (e.value, want)
        return want
    got = shafa.verify_files(d_in, **kw)
    assert isinstance(got, shafa.Verify) and got == want, (got, want)
    assert type(got.equal) is bool and type(got.decoded_size) is int and (got.first_diff is None or type(got.first_diff) is int)
    return got


# ---------------------------------------------------------------- 1. golden sessions
def _golden():
    """(case, input, {file arguments: stored names}, decode_rle) from the manifests; a .cod the session damaged on purpose is
    no file of its input"""
    out = []
    for case in sorted(os.listdir(GOLD)):
        p = os.path.join(GOLD, case, "manifest.json")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            man = json.load(f)
        damaged = {cmd[1] for cmd in man["cmds"] if isinstance(cmd, list) and cmd[0] == "__corrupt_cod__"}
        stored = lambda k: k in man["files"] and k not in damaged and os.path.exists(os.path.join(GOLD, case, k))
        for x in sorted(man["files"]):
            if not stored(x) or "." in x:
                continue
            if stored(x + ".shaf") and stored(x + ".cod"):
                out.append((case, x, dict(shaf=x + ".shaf", cod=x + ".cod"), False))
            if stored(x + ".rle.shaf") and stored(x + ".rle.cod"):
                out.append((case, x, dict(shaf=x + ".rle.shaf", cod=x + ".rle.cod"), True))
            if stored(x + ".rle") and stored(x + ".rle.freq"):
                out.append((case, x, dict(rle=x + ".rle", freq=x + ".rle.freq"), True))
    return out


GOLDEN = _golden()


def _read(case, name):
    with open(os.path.join(GOLD, case, name), "rb") as f:
        return f.read()


def test_golden_list():
    got = {(c, tuple(sorted(f))) for c, _, f, _ in GOLDEN}
    assert {("uniform_no_rle", ("cod", "shaf")), ("textlike_m", ("cod", "shaf")), ("runs_default", ("cod", "shaf")),
            ("runs_default", ("freq", "rle")), ("edges_forced_rle", ("cod", "shaf")), ("edge_tail_7", ("freq", "rle")),
            ("runs_force_freq", ("freq", "rle")), ("uniform_forced_both", ("freq", "rle")), ("tiny_1024", ("cod", "shaf")),
            ("cli_errors", ("freq", "rle"))} <= got, sorted(got)


@pytest.mark.parametrize("case,inp,names,decode_rle", GOLDEN, ids=[f"{c}-{'-'.join(sorted(f))}" for c, _, f, _ in GOLDEN])
def test_golden_sets_verify(shafa, case, inp, names, decode_rle):
    data = _read(case, inp)
    kw = {k: _t(_read(case, v), 5 if k in ("shaf", "rle") else 0) for k, v in names.items()}
    d_in = _t(data, 9)
    want = _oracle(shafa, d_in, decode_rle=decode_rle, **kw)
    if isinstance(want, shafa.ShafaError):
        # a last block of one byte is a block of one symbol: Module D refuses its empty codes (tests/test_gpu_unpack.py)
        assert case == "edge_tail_1" and "shaf" in names and want.code == shafa.FILE_UNRECOGNIZABLE, (case, want)
        _same(shafa, d_in, want, decode_rle=decode_rle, **kw)
        return
    assert want == shafa.Verify(True, None, len(data))
    assert shafa.verify_files(d_in, decode_rle=decode_rle, **kw) == shafa.Verify(True, None, len(data))


# ---------------------------------------------------------------- 2 .. 5. synthetic sets
SIZES = [(1024, 4096), (3 * 4096 + 1, 4096), (3 * 4096 + 33, 4096), (5 * 65536 + 15, 65536)]
_SETS = {}


def _sets(shafa, n, bs):
    """(name, d_in, file arguments) of the three file forms at this size, made once: mode N from a Zipf stream; rle + freq and
    mode-R shaf + cod from a runs stream; that pair with decode_rle=False against the .rle bytes"""
    import torch
    if (n, bs) not in _SETS:
        synth = pkgload.load_submodule("synth")
        zt = synth.zipf_table(1.2)
        plain = torch.from_numpy(synth.gen_bytes(31 + n, n, zt)).to(_dev())
        runs = torch.from_numpy(synth.runs_stream(32 + n, n, zt)).to(_dev())
        fp = shafa.compress_files(plain, bs)
        fr = shafa.compress_files(runs, bs, force_rle=True)
        assert ".shaf" in fp and ".rle.shaf" in fr, (sorted(fp), sorted(fr))
        _SETS[(n, bs)] = [("N", plain, dict(shaf=fp[".shaf"], cod=fp[".cod"], decode_rle=False)),
                          ("rle+freq", runs, dict(rle=fr[".rle"], freq=fr[".rle.freq"])),
                          ("R", runs, dict(shaf=fr[".rle.shaf"], cod=fr[".rle.cod"])),
                          ("R as .rle", fr[".rle"], dict(shaf=fr[".rle.shaf"], cod=fr[".rle.cod"], decode_rle=False))]
    return _SETS[(n, bs)]


def _blocks_of(n, bs):
    return [(a, min(a + bs, n)) for a in range(0, n, bs)]


def _plant(d_in, *at):
    x = d_in.clone()
    for i in at:
        x[i] ^= 0x40
    return x


@pytest.mark.parametrize("n,bs", SIZES, ids=[str(n) for n, _ in SIZES])
def test_synthetic_sets(shafa, n, bs):
    import torch
    for name, d_in, kw in _sets(shafa, n, bs):
        N = d_in.numel()                                             # the decoded size: n, or the .rle's length
        want = _oracle(shafa, d_in, **kw)
        # a last block of one byte is a block of one symbol: Module D refuses its empty codes (tests/test_gpu_unpack.py), so
        # a .shaf of such a set has no decoded file, and every call below raises what decompress_files raises
        refused = isinstance(want, shafa.ShafaError)
        if refused:
            assert n % bs == 1 and "shaf" in kw and want.code == shafa.FILE_UNRECOGNIZABLE, (name, want)
        else:
            assert want == shafa.Verify(True, None, N), name
        inputs = {"equal": (d_in, want)}
        # 3. planted differences (block borders: of the input's blocks for the three forms that decode to it)
        spots = [(0,), (N - 1,), (N // 2, N - 1)]
        if name != "R as .rle" and n > bs:
            spots += [(bs - 1,), (bs,), (bs + 5, 2 * bs + 7)]
        for at in spots:
            inputs[f"differs at {at}"] = (_plant(d_in, *at), shafa.Verify(False, at[0], N))
        # 4. lengths and alignment
        inputs["shorter"] = (d_in[:N - 1], shafa.Verify(False, N - 1, N))
        inputs["longer"] = (torch.cat([d_in, d_in[:1]]), shafa.Verify(False, N, N))
        inputs["longer and differs"] = (torch.cat([_plant(d_in, 7), d_in[:1]]), shafa.Verify(False, 7, N))
        inputs["empty"] = (d_in[:0], shafa.Verify(False, 0, N))
        inputs["a block short"] = (d_in[:max(N - bs, 1)].clone(), shafa.Verify(False, max(N - bs, 1), N))
        off3 = torch.cat([d_in[:3], d_in])[3:]
        assert off3.storage_offset() == 3 and off3.data_ptr() % 16 == 3
        inputs["at storage offset 3"] = (off3, want)
        inputs["at storage offset 3, differs"] = (torch.cat([d_in[:3], _plant(d_in, N - 1)])[3:], shafa.Verify(False, N - 1, N))
        for what, (x, expect) in inputs.items():
            if refused:                                              # faults come before any difference
                for mb in (None, 65536, 1):
                    _same(shafa, x, want, max_bytes=mb, **kw)
                continue
            if what in ("equal", "differs at (0,)", "shorter"):      # the expectations above are the oracle's
                assert _oracle(shafa, x, **kw) == expect, (name, what)
            for mb in (None, 65536, 1):
                got = shafa.verify_files(x, max_bytes=mb, **kw)
                assert got == expect, (name, what, mb, got, expect)


def test_empty_file_set(shafa):
    import torch
    # a .freq / .cod that announces no block: the empty file
    for kw in (dict(rle=_t(b""), freq=_t(b"@R@0@0")), dict(shaf=_t(b"@0"), cod=_t(b"@N@0@0"), decode_rle=False)):
        for d_in in (torch.zeros(0, dtype=torch.uint8, device=_dev()), _t(b"abc", 1)):
            want = _oracle(shafa, d_in, **kw)
            if not isinstance(want, shafa.ShafaError):
                assert want == shafa.Verify(d_in.numel() == 0, None if d_in.numel() == 0 else 0, 0)
            _same(shafa, d_in, want, **kw)


def test_bad_d_in(shafa):
    import torch
    _, d_in, kw = _sets(shafa, *SIZES[0])[0]
    for bad in (d_in.cpu(), d_in.to(torch.int8), torch.cat([d_in, d_in])[::2], None):
        with pytest.raises(ValueError):
            shafa.verify_files(bad, **kw)


# ---------------------------------------------------------------- 5. faults come first
def test_faults_raise_what_decompress_files_raises(shafa):
    n, bs = SIZES[2]
    sets = {name: (d_in, kw) for name, d_in, kw in _sets(shafa, n, bs)}
    cases = []
    # a flipped payload byte in the .shaf that makes the decoder fail: look for one in block 2's payload
    d_in, kw = sets["N"]
    shaf = _bytes(kw["shaf"])
    start = len(shaf) * 2 // 5
    for i in range(start, start + 4000, 37):
        bad = dict(kw, shaf=_t(shaf[:i] + bytes([shaf[i] ^ 0xFF]) + shaf[i + 1:], 2))
        if isinstance(_oracle(shafa, d_in, **bad), shafa.ShafaError):
            cases.append(("flipped payload byte", d_in, bad))
            break
    else:
        # every flip decoded to other bytes of the same length: then it is a difference, not a fault
        got = _same(shafa, d_in, **bad)
        assert got.equal is False
    # a cut payload (the block's announced size no longer fits the file)
    cases.append(("cut .shaf", d_in, dict(kw, shaf=_t(shaf[:len(shaf) - 100], 1))))
    # a truncated .cod: a parse fault behind good blocks
    cod = _bytes(kw["cod"])
    cases.append(("truncated .cod", d_in, dict(kw, cod=_t(cod[:len(cod) * 3 // 5]))))
    d_r, kw_r = sets["R"]
    cod_r = _bytes(kw_r["cod"])
    cases.append(("truncated mode-R .cod", d_r, dict(kw_r, cod=_t(cod_r[:len(cod_r) * 3 // 5]))))
    d_f, kw_f = sets["rle+freq"]
    freq = _bytes(kw_f["freq"])
    cases.append(("truncated .rle.freq", d_f, dict(kw_f, freq=_t(freq[:len(freq) - 9]))))
    cases.append(("cut .rle", d_f, dict(kw_f, rle=_t(_bytes(kw_f["rle"])[:-50]))))
    # a mode-N .cod where RLE decoding is asked for
    cases.append(("mode N, decode_rle", d_in, dict(kw, decode_rle=True)))
    codes = {}
    for what, x, bad in cases:
        want = _oracle(shafa, x, **bad)
        assert isinstance(want, shafa.ShafaError), what
        codes[what] = want.code
        for y in (x, _plant(x, 0), _plant(x, x.numel() - 1), x[:100]):
            for mb in (None, 65536):
                _same(shafa, y, want, max_bytes=mb, **bad)
    assert codes["mode N, decode_rle"] == shafa.FILE_UNRECOGNIZABLE
    assert len(cases) >= 6


# ---------------------------------------------------------------- 6. bounded memory, launches, synchronisations
NB, BS = 256, 65536


@pytest.fixture(scope="module")
def wide_sets(shafa):
    """a mode-N set and an .rle + .freq set of 256 blocks of 64 KiB"""
    import torch
    synth = pkgload.load_submodule("synth")
    zt = synth.zipf_table(1.2)
    plain = torch.from_numpy(synth.gen_bytes(77, NB * BS, zt)).to(_dev())
    runs = torch.from_numpy(np.tile(synth.runs_stream(78, 16 * BS, zt), NB // 16)).to(_dev())
    fp = shafa.compress_files(plain, BS)
    fr = shafa.compress_files(runs, BS, force_rle=True)
    assert ".shaf" in fp
    return {"N": (plain, dict(shaf=fp[".shaf"], cod=fp[".cod"], decode_rle=False)),
            "rle+freq": (runs, dict(rle=fr[".rle"], freq=fr[".rle.freq"])),
            "R": (runs, dict(shaf=fr[".rle.shaf"], cod=fr[".rle.cod"]))}


@pytest.mark.parametrize("name", ["N", "rle+freq"])
def test_peak_memory_stays_below_the_decoding_driver(shafa, wide_sets, name):
    import torch
    d_in, kw = wide_sets[name]
    n = d_in.numel()
    MB = 1 << 20
    shafa.verify_files(d_in[:BS], max_bytes=MB, **kw)                   # warm-up: code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = shafa.decompress_files(max_bytes=MB, **kw)
    torch.cuda.synchronize()
    peak_d = torch.cuda.max_memory_allocated()
    assert out.numel() == n
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    got = shafa.verify_files(d_in, max_bytes=MB, **kw)
    torch.cuda.synchronize()
    peak_v = torch.cuda.max_memory_allocated()
    assert got == shafa.Verify(True, None, n)
    print(f"{name}: peak decompress_files {peak_d}, verify_files {peak_v}, decoded {n}")
    assert peak_v <= peak_d - n // 2, (peak_v, peak_d, n)


@pytest.mark.parametrize("name", ["N", "rle+freq", "R"])
def test_launches_and_synchronisations(shafa, wide_sets, monkeypatch, name):
    d_in, kw = wide_sets[name]
    n = d_in.numel()
    MB = 1 << 20
    fin = _count_calls(shafa, monkeypatch, "finish")
    shafa.decompress_files(max_bytes=MB, **kw)
    base = len(fin)
    assert base == {"N": 2, "rle+freq": 3, "R": 4}[name]                # parse (+ SF decode) (+ measure) + the last one
    fin.clear()
    packs = _count_calls(shafa, monkeypatch, "pack_payloads")
    cmp_calls = _count_calls(shafa, monkeypatch, "compare_dev")
    sf = _count_calls(shafa, monkeypatch, "sf_decode_dev")
    rld = _count_calls(shafa, monkeypatch, "rle_decode_dev")
    got = shafa.verify_files(_plant(d_in, n - 3), max_bytes=MB, **kw)
    assert got == shafa.Verify(False, n - 3, n)
    assert not packs, len(packs)
    if name == "N":
        # groups of whole blocks whose decoded bytes and payloads fit 1 MiB: at least 16 (the decoded bytes alone), at most 32
        groups = len(cmp_calls)
        assert 16 < groups <= 32 and len(sf) == groups and not rld
        assert len(fin) == 1 + groups                                   # the parse, and each group's own
    else:
        groups = len(cmp_calls)
        assert groups == len(rld) == NB * BS // MB                      # exact regions: 16 blocks a group
        assert len(sf) == (1 if name == "R" else 0)
        assert len(fin) == base                                         # parse (+ SF decode) + measure + one at the end

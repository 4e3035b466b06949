"""shafa.checksum_files: the CRC-32 and the length of what a file set held in device memory decodes to, without the decoded
file.  The oracle is the existing driver: with out = decompress_files(the same arguments), checksum_files raises what that
call raises, and otherwise returns Checksum(zlib.crc32(out), out.numel()).

1. every golden session that stores a .shaf + .cod or a .rle + .freq: against zlib.crc32 of the stored original where the
   session stores it, else against decompress_files' output;
2. synthetic sets (test_gpu_verify_files' : mode N, rle + freq, mode R with and without decode_rle, at 1024, 3 x 4096 + 1,
   3 x 4096 + 33 and 5 x 65536 + 15 bytes) at max_bytes = default, 65536 and 1; at 3 x 4096 + 1 the last block is one byte,
   where a .shaf has no decoded file and checksum_files raises decompress_files' error;
3. a single changed payload byte changes the CRC, or raises exactly what decompress_files raises;
4. faulty files raise decompress_files' code;
5. no decoded file: the peak stays half a decoded size below decompress_files', no pack runs, and the synchronisations number
   no more than verify_files' for the same arguments."""
import json
import os
import zlib

import pytest

from test_gpu_rle_measure import _count_calls
from test_gpu_unpack import GOLD, _bytes, _t
from test_gpu_verify_files import BS, NB, SIZES, _read, _sets, wide_sets  # noqa: F401  (wide_sets: a fixture)

pytestmark = pytest.mark.gpu


def _oracle(shafa, **kw):
    """the definition: from decompress_files and zlib on the host -> a Checksum, or the ShafaError it raises"""
    try:
        out = shafa.decompress_files(**{k: v for k, v in kw.items() if k != "max_bytes"})
    except shafa.ShafaError as e:
        return e
    return shafa.Checksum(zlib.crc32(_bytes(out)), out.numel())


def _same(shafa, want=None, **kw):
    """checksum_files(**kw) against the oracle (or `want`, an oracle's answer for the same arguments) -> the answer"""
    if want is None:
        want = _oracle(shafa, **kw)
    if isinstance(want, shafa.ShafaError):
        with pytest.raises(shafa.ShafaError) as e:
            shafa.checksum_files(**kw)
        assert e.value.code == want.code, (e.value, want)
        return want
    got = shafa.checksum_files(**kw)
    assert isinstance(got, shafa.Checksum) and got == want, (got, want)
    assert type(got.crc32) is int and type(got.decoded_size) is int and 0 <= got.crc32 < 1 << 32
    return got


# ---------------------------------------------------------------- 1. golden sessions
def _golden():
    """(case, {file arguments: stored names}, decode_rle, the stored original's name or None) from the manifests; a .cod the
    session damaged on purpose is left out (the faults are 4.'s)"""
    out = []
    for case in sorted(os.listdir(GOLD)):
        p = os.path.join(GOLD, case, "manifest.json")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            man = json.load(f)
        damaged = {cmd[1] for cmd in man["cmds"] if isinstance(cmd, list) and cmd[0] == "__corrupt_cod__"}
        stored = lambda k: k in man["files"] and k not in damaged and os.path.exists(os.path.join(GOLD, case, k))
        for k in sorted(man["files"]):
            if k.endswith(".shaf") and stored(k) and stored(k[:-5] + ".cod"):
                base = k[:-5]
                rle = base.endswith(".rle")
                orig = base[:-4] if rle else base
                out.append((case, dict(shaf=k, cod=base + ".cod"), rle, orig if stored(orig) else None))
            if k.endswith(".rle") and stored(k) and stored(k + ".freq"):
                out.append((case, dict(rle=k, freq=k + ".freq"), True, k[:-4] if stored(k[:-4]) else None))
    return out


GOLDEN = _golden()


def test_golden_list():
    got = {(c, tuple(sorted(f)), o is not None) for c, f, _, o in GOLDEN}
    assert {("uniform_no_rle", ("cod", "shaf"), True), ("runs_default", ("cod", "shaf"), True),
            ("runs_default", ("freq", "rle"), True), ("tiny_1024", ("cod", "shaf"), True)} <= got, sorted(got)


@pytest.mark.parametrize("case,names,decode_rle,orig", GOLDEN, ids=[f"{c}-{'-'.join(sorted(f))}" for c, f, _, _ in GOLDEN])
def test_golden_sets(shafa, case, names, decode_rle, orig):
    kw = {k: _t(_read(case, v), 5 if k in ("shaf", "rle") else 0) for k, v in names.items()}
    want = _oracle(shafa, decode_rle=decode_rle, **kw)
    if isinstance(want, shafa.ShafaError):
        # a last block of one byte is a block of one symbol: Module D refuses its empty codes (tests/test_gpu_unpack.py)
        assert want.code == shafa.FILE_UNRECOGNIZABLE and "shaf" in names, (case, want)
    elif orig is not None:
        data = _read(case, orig)
        assert want == shafa.Checksum(zlib.crc32(data), len(data)), case
    _same(shafa, want, decode_rle=decode_rle, **kw)


# ---------------------------------------------------------------- 2. synthetic sets
@pytest.mark.parametrize("n,bs", SIZES, ids=[str(n) for n, _ in SIZES])
def test_synthetic_sets(shafa, n, bs):
    for name, d_in, kw in _sets(shafa, n, bs):
        want = _oracle(shafa, **kw)
        if isinstance(want, shafa.ShafaError):
            assert n % bs == 1 and "shaf" in kw and want.code == shafa.FILE_UNRECOGNIZABLE, (name, want)
        else:
            assert want == shafa.Checksum(zlib.crc32(_bytes(d_in)), d_in.numel()), name
            assert shafa.crc32(d_in) == want.crc32, name                 # the digest taken from the original in place
        for mb in (None, 65536, 1):
            _same(shafa, want, max_bytes=mb, **kw)


def test_empty_file_set(shafa):
    for kw in (dict(rle=_t(b""), freq=_t(b"@R@0@0")), dict(shaf=_t(b"@0"), cod=_t(b"@N@0@0"), decode_rle=False)):
        want = _oracle(shafa, **kw)
        if not isinstance(want, shafa.ShafaError):
            assert want == shafa.Checksum(0, 0)
        _same(shafa, want, **kw)


# ---------------------------------------------------------------- 3. one changed payload byte
def test_changed_payload_byte(shafa):
    n, bs = SIZES[2]
    sets = {name: (d_in, kw) for name, d_in, kw in _sets(shafa, n, bs)}
    seen = {"raised": 0, "changed": 0}
    for name, key in (("N", "shaf"), ("rle+freq", "rle"), ("R", "shaf")):
        d_in, kw = sets[name]
        good = _same(shafa, **kw)
        assert good.crc32 == zlib.crc32(_bytes(d_in))
        payload = _bytes(kw[key])
        for i in sorted({len(payload) // 7, len(payload) * 2 // 5, len(payload) * 2 // 5 + 37, len(payload) - 2}):
            bad = dict(kw, **{key: _t(payload[:i] + bytes([payload[i] ^ 0x10]) + payload[i + 1:], 2)})
            want = _oracle(shafa, **bad)
            for mb in (None, 65536):
                _same(shafa, want, max_bytes=mb, **bad)
            if isinstance(want, shafa.ShafaError):
                seen["raised"] += 1
            elif _bytes(shafa.decompress_files(**bad)) != _bytes(d_in):
                assert want.crc32 != good.crc32, (name, i)
                seen["changed"] += 1
    assert seen["changed"] + seen["raised"] >= 6, seen


# ---------------------------------------------------------------- 4. faults
def test_faults_raise_what_decompress_files_raises(shafa):
    n, bs = SIZES[2]
    sets = {name: kw for name, _, kw in _sets(shafa, n, bs)}
    kw, kw_r, kw_f = sets["N"], sets["R"], sets["rle+freq"]
    shaf, cod, cod_r, freq = _bytes(kw["shaf"]), _bytes(kw["cod"]), _bytes(kw_r["cod"]), _bytes(kw_f["freq"])
    cases = [("cut .shaf", dict(kw, shaf=_t(shaf[:len(shaf) - 100], 1))),
             ("truncated .cod", dict(kw, cod=_t(cod[:len(cod) * 3 // 5]))),
             ("truncated mode-R .cod", dict(kw_r, cod=_t(cod_r[:len(cod_r) * 3 // 5]))),
             ("truncated .rle.freq", dict(kw_f, freq=_t(freq[:len(freq) - 9]))),
             ("cut .rle", dict(kw_f, rle=_t(_bytes(kw_f["rle"])[:-50]))),
             ("mode N, decode_rle", dict(kw, decode_rle=True)),
             ("bad header", dict(kw, cod=_t(b"@X@1@5@" + cod[7:])))]
    codes = {}
    for what, bad in cases:
        want = _oracle(shafa, **bad)
        assert isinstance(want, shafa.ShafaError), what
        codes[what] = want.code
        for mb in (None, 65536, 1):
            _same(shafa, want, max_bytes=mb, **bad)
    assert codes["mode N, decode_rle"] == shafa.FILE_UNRECOGNIZABLE


# ---------------------------------------------------------------- 5. bounded memory, launches, synchronisations
@pytest.mark.parametrize("name", ["N", "rle+freq"])
def test_peak_memory_stays_below_the_decoding_driver(shafa, wide_sets, name):  # noqa: F811
    import torch
    d_in, kw = wide_sets[name]
    n = d_in.numel()
    MB = 1 << 20
    shafa.checksum_files(max_bytes=MB, **kw)                            # warm-up: code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    out = shafa.decompress_files(max_bytes=MB, **kw)
    torch.cuda.synchronize()
    peak_d = torch.cuda.max_memory_allocated() - resident
    assert out.numel() == n
    want = shafa.Checksum(zlib.crc32(_bytes(out)), n)
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    got = shafa.checksum_files(max_bytes=MB, **kw)
    torch.cuda.synchronize()
    peak_c = torch.cuda.max_memory_allocated() - resident
    assert got == want
    print(f"{name}: peak beyond the resident bytes: decompress_files {peak_d}, checksum_files {peak_c}, decoded {n}")
    assert peak_c < peak_d and peak_c <= peak_d - n // 2, (peak_c, peak_d, n)


@pytest.mark.parametrize("name", ["N", "rle+freq", "R"])
def test_launches_and_synchronisations(shafa, wide_sets, monkeypatch, name):  # noqa: F811
    d_in, kw = wide_sets[name]
    n = d_in.numel()
    MB = 1 << 20
    fin = _count_calls(shafa, monkeypatch, "finish")
    assert shafa.verify_files(d_in, max_bytes=MB, **kw) == shafa.Verify(True, None, n)
    syncs_verify = len(fin)
    fin.clear()
    packs = _count_calls(shafa, monkeypatch, "pack_payloads")
    crcs = _count_calls(shafa, monkeypatch, "crc32_dev")
    joins = _count_calls(shafa, monkeypatch, "crc32_combine_dev")
    cmps = _count_calls(shafa, monkeypatch, "compare_dev")
    got = shafa.checksum_files(max_bytes=MB, **kw)
    assert got == shafa.Checksum(shafa.crc32(d_in), n)
    fin_checksum = len(fin) - 1                                          # shafa.crc32's own
    assert not packs and not cmps
    assert len(joins) == 2 and len(crcs) >= NB * BS // MB + 1            # one combine each for checksum_files and crc32
    assert fin_checksum <= syncs_verify, (fin_checksum, syncs_verify)

"""shafa.find_files: where a pattern occurs in the file a file set held in device memory decodes to.  The oracle is Python on
the host over decompress_files' bytes: i = data.find(pat); while i >= 0: ...; i = data.find(pat, i + 1); find_files raises
what decompress_files raises.

1. the synthetic sets of tests/test_gpu_verify_files.py (1024, 3 x 4096 + 1, 3 x 4096 + 33 and 5 x 65536 + 15 bytes; mode N,
   .rle + .freq, mode R with and without decode_rle) at max_bytes = default, 65536 and 1 (every block a group of its own).
   The patterns are taken from the decoded file itself: the 1, 4, 9 and 256 bytes that straddle each block border, so a match
   on every block seam and, at max_bytes = 1, on every group seam is certain to exist; one pattern does not occur;
2. faulty and damaged sets raise decompress_files' code; the empty set gives Found(0, [], 0);
3. no decoded file: the peak stays half a decoded size below decompress_files', no pack runs, and finish is called no more
   often than by verify_files."""
import numpy as np
import pytest

from test_gpu_rle_measure import _count_calls
from test_gpu_unpack import _bytes, _dev, _t
from test_gpu_verify_files import BS, NB, SIZES, _sets, wide_sets      # noqa: F401  (wide_sets is a fixture)
from test_gpu_verify_files import _oracle as _verify_oracle

pytestmark = pytest.mark.gpu


def _all(data, pat):
    k, out = data.find(pat), []
    while k >= 0:
        out.append(k)
        k = data.find(pat, k + 1)
    return out


def _same(shafa, got, want, size, max_hits=65536):
    assert isinstance(got, shafa.Found) and type(got.count) is int and type(got.size) is int
    assert got.count == len(want) and got.size == size, (got.count, len(want), got.size, size)
    assert got.positions.dtype == np.int64 and got.positions.tolist() == want[:max_hits]


def _absent(data, seed):
    rng = np.random.default_rng(seed)
    while True:
        pat = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        if data.find(pat) < 0:
            return pat


def _borders(shafa, name, kw, n, bs):
    """where the decoded file's blocks meet: the input's blocks, or for a mode-R pair read as .rle bytes the sizes its .cod
    announces ("@R@count@size@codes@size@codes ...")"""
    if name == "R as .rle":
        f = _bytes(kw["cod"]).split(b"@")
        sizes = [int(x) for x in f[3:3 + 2 * int(f[2]):2]]
        assert f[1] == b"R" and len(sizes) == int(f[2])
    else:
        sizes = [min(bs, n - a) for a in range(0, n, bs)]
    return list(np.cumsum(sizes))[:-1], sum(sizes)


@pytest.mark.parametrize("n,bs", SIZES, ids=[str(n) for n, _ in SIZES])
def test_three_forms(shafa, n, bs):
    for name, _, kw in _sets(shafa, n, bs):
        try:
            data = _bytes(shafa.decompress_files(**kw))
        except shafa.ShafaError as e:
            # a last block of one byte is a block of one symbol: Module D refuses its empty codes in a .shaf
            assert n % bs == 1 and "shaf" in kw and e.code == shafa.FILE_UNRECOGNIZABLE, (name, e)
            for mb in (None, 65536, 1):
                with pytest.raises(shafa.ShafaError) as got:
                    shafa.find_files(b"ab", max_bytes=mb, **kw)
                assert got.value.code == e.code, (name, mb)
            continue
        borders, total = _borders(shafa, name, kw, n, bs)
        assert total == len(data), name
        pats = {data[10:10 + m] for m in (1, 4, 9, 256)}
        for B in borders:
            pats |= {data[B - m // 2:B - m // 2 + m] for m in (1, 4, 9, 256) if B - m // 2 >= 0 and B - m // 2 + m <= len(data)}
        near = not borders                                           # a reported match just in front of a block border
        for pat in sorted(pats) + [_absent(data, n)]:
            want = _all(data, pat)
            for mb in (None, 65536, 1):
                got = shafa.find_files(pat, max_bytes=mb, **kw)
                _same(shafa, got, want, len(data))
                near = near or any(((B - got.positions > 0) & (B - got.positions < len(pat))).any() for B in borders)
        assert near, name
        assert shafa.find_files(_absent(data, n), **kw).count == 0
        # few hits kept, and none: the count stays exact
        pat = data[10:11]
        want = _all(data, pat)
        for mh in (0, 1, 7):
            for mb in (None, 1):
                _same(shafa, shafa.find_files(pat, max_hits=mh, max_bytes=mb, **kw), want, len(data), mh)


def test_short_blocks_and_long_patterns(shafa):
    """the smallest blocks the host cuts (512 bytes) under the longest patterns, and a last block shorter than the pattern:
    the head of the last group is the whole group"""
    import torch
    rng = np.random.default_rng(5)
    data = rng.integers(97, 101, 5 * 512 + 9, dtype=np.uint8)
    d_in = torch.from_numpy(data).to(_dev())
    fs = shafa.compress_files(d_in, 512)
    assert ".shaf" in fs
    kw = dict(shaf=fs[".shaf"], cod=fs[".cod"], decode_rle=False)
    raw = data.tobytes()
    assert _bytes(shafa.decompress_files(**kw)) == raw and shafa.decoded_sizes(shaf=kw["shaf"], cod=kw["cod"]) == [512] * 5 + [9]
    for pat in (raw[500:756], raw[2310:2566], raw[-70:], raw[-9:], raw[-10:], raw[2559:2561], raw[1000:1300][:255], b"ab", b"a"):
        want = _all(raw, pat)
        assert want
        for mb in (None, 1, 700, 4096):
            _same(shafa, shafa.find_files(pat, max_bytes=mb, **kw), want, len(raw))


def test_empty_file_set(shafa):
    for kw in (dict(rle=_t(b""), freq=_t(b"@R@0@0")), dict(shaf=_t(b"@0"), cod=_t(b"@N@0@0"), decode_rle=False)):
        try:
            out = shafa.decompress_files(**kw)
        except shafa.ShafaError as e:
            with pytest.raises(shafa.ShafaError) as got:
                shafa.find_files(b"a", **kw)
            assert got.value.code == e.code
            continue
        assert out.numel() == 0
        got = shafa.find_files(b"a", **kw)
        assert got.count == 0 and got.size == 0 and got.positions.size == 0 and got.positions.dtype == np.int64


def test_faults_raise_what_decompress_files_raises(shafa):
    """the cases of tests/test_gpu_verify_files.py, built the same way"""
    n, bs = SIZES[2]
    sets = {name: (d_in, kw) for name, d_in, kw in _sets(shafa, n, bs)}
    cases = []
    d_in, kw = sets["N"]
    shaf = _bytes(kw["shaf"])
    start = len(shaf) * 2 // 5
    for i in range(start, start + 4000, 37):                         # a flipped payload byte that makes the decoder fail
        bad = dict(kw, shaf=_t(shaf[:i] + bytes([shaf[i] ^ 0xFF]) + shaf[i + 1:], 2))
        if isinstance(_verify_oracle(shafa, d_in, **bad), shafa.ShafaError):
            cases.append(("flipped payload byte", bad))
            break
    cases.append(("cut .shaf", dict(kw, shaf=_t(shaf[:len(shaf) - 100], 1))))
    cod = _bytes(kw["cod"])
    cases.append(("truncated .cod", dict(kw, cod=_t(cod[:len(cod) * 3 // 5]))))
    _, kw_r = sets["R"]
    cod_r = _bytes(kw_r["cod"])
    cases.append(("truncated mode-R .cod", dict(kw_r, cod=_t(cod_r[:len(cod_r) * 3 // 5]))))
    _, kw_f = sets["rle+freq"]
    freq = _bytes(kw_f["freq"])
    cases.append(("truncated .rle.freq", dict(kw_f, freq=_t(freq[:len(freq) - 9]))))
    cases.append(("cut .rle", dict(kw_f, rle=_t(_bytes(kw_f["rle"])[:-50]))))
    cases.append(("mode N, decode_rle", dict(kw, decode_rle=True)))
    assert len(cases) >= 6
    pat = _bytes(d_in)[:3]
    for what, bad in cases:
        with pytest.raises(shafa.ShafaError) as want:
            shafa.decompress_files(**bad)
        for mb in (None, 65536, 1):
            for mh in (65536, 0):
                with pytest.raises(shafa.ShafaError) as got:
                    shafa.find_files(pat, max_bytes=mb, max_hits=mh, **bad)
                assert got.value.code == want.value.code, (what, mb, got.value, want.value)


# ---------------------------------------------------------------- bounded memory, launches, synchronisations
MB = 1 << 20


@pytest.fixture(scope="module")
def wide_data(wide_sets):
    return {name: _bytes(d_in) for name, (d_in, _) in wide_sets.items() if name != "R"}


def _wide_patterns(data):
    """over block borders that are group borders at 1 MiB, and one that is rare"""
    return [data[B - 5:B + 4] for B in (BS, 16 * BS, 17 * BS, 128 * BS)] + [data[16 * BS - 100:16 * BS + 156], _absent(data, 1)]


@pytest.mark.parametrize("name", ["N", "rle+freq", "R"])
def test_wide_sets_against_the_original(shafa, wide_sets, wide_data, name):
    _, kw = wide_sets[name]
    data = wide_data["rle+freq" if name == "R" else name]
    for pat in _wide_patterns(data):
        _same(shafa, shafa.find_files(pat, max_bytes=MB, **kw), _all(data, pat), NB * BS)


@pytest.mark.parametrize("name", ["N", "rle+freq"])
def test_peak_memory_stays_below_the_decoding_driver(shafa, wide_sets, wide_data, name):
    import torch
    d_in, kw = wide_sets[name]
    n = d_in.numel()
    pat = wide_data[name][BS - 5:BS + 4]
    shafa.find_files(pat, max_bytes=MB, **kw)                          # warm-up: code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = shafa.decompress_files(max_bytes=MB, **kw)
    torch.cuda.synchronize()
    peak_d = torch.cuda.max_memory_allocated()
    assert out.numel() == n
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    got = shafa.find_files(pat, max_bytes=MB, **kw)
    torch.cuda.synchronize()
    peak_f = torch.cuda.max_memory_allocated()
    assert got.count >= 1 and got.size == n
    print(f"{name}: peak decompress_files {peak_d}, find_files {peak_f}, decoded {n}")
    assert peak_f <= peak_d - n // 2, (peak_f, peak_d, n)


@pytest.mark.parametrize("name", ["N", "rle+freq", "R"])
def test_launches_and_synchronisations(shafa, wide_sets, wide_data, monkeypatch, name):
    d_in, kw = wide_sets[name]
    n = d_in.numel()
    pat = wide_data["rle+freq" if name == "R" else name][16 * BS - 5:16 * BS + 4]
    fin = _count_calls(shafa, monkeypatch, "finish")
    assert shafa.verify_files(d_in, max_bytes=MB, **kw) == shafa.Verify(True, None, n)
    base = len(fin)
    fin.clear()
    packs = _count_calls(shafa, monkeypatch, "pack_payloads")
    finds = _count_calls(shafa, monkeypatch, "find_dev")
    got = shafa.find_files(pat, max_bytes=MB, **kw)
    assert got.count >= 1 and got.size == n
    assert not packs, len(packs)
    assert len(fin) <= base, (len(fin), base)
    groups = (len(finds) + 1) // 2                                     # a group's own call, and a seam's for all but the first
    assert len(finds) == 2 * groups - 1 and groups >= NB * BS // MB

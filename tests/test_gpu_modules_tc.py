"""Modules T and C alone on files held in device memory: shafa_hipd_unpack_freq (csrc/unpack.hip), shafa.build_cod and
shafa.encode_files.

1. build_cod reproduces the stored .cod of every golden directory that stores a .freq and its .cod;
2. encode_files reproduces the stored .shaf of every golden directory that stores the input, its .cod and its .shaf;
3. unpack_freq equals the C host's parser (shafa.freq_parse) and framing on hand-made texts, block counts and alignments;
4. build_cod / encode_files reproduce compress_files' own files, and decompress_files returns the input;
5. faulty files raise the code the C host's Module T / Module C return on the same bytes (ctypes, in process);
6. nothing is written outside the caller's arrays;
7. unpack_freq only enqueues."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_unpack import GOLD, _bytes, _dev, _files, _t, _u64

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CANARY = 0xA5A5A5A5A5A5A5A5


# ---------------------------------------------------------------- 1, 2. golden files
def _man(case):
    with open(os.path.join(GOLD, case, "manifest.json")) as f:
        return json.load(f)


def _golden():
    """from the manifests: (case, X.freq, X.cod) and (case, X, X.cod, X.shaf) whose files are all stored; a .cod that the
    session damaged on purpose after Module T wrote it (a __corrupt_cod__ step) is no product of its .freq"""
    t, c = [], []
    for case in sorted(os.listdir(GOLD)):
        if not os.path.exists(os.path.join(GOLD, case, "manifest.json")):
            continue
        man = _man(case)
        damaged = {cmd[1] for cmd in man["cmds"] if isinstance(cmd, list) and cmd[0] == "__corrupt_cod__"}
        stored = lambda k: k in man["files"] and os.path.exists(os.path.join(GOLD, case, k))
        for k in sorted(man["files"]):
            if not k.endswith(".cod") or k in damaged or not stored(k):
                continue
            x = k[:-len(".cod")]
            if stored(x + ".freq"):
                t.append((case, x + ".freq", k))
            if stored(x) and stored(x + ".shaf"):
                c.append((case, x, k, x + ".shaf"))
    return t, c


GOLD_T, GOLD_C = _golden()


def _read(case, name):
    with open(os.path.join(GOLD, case, name), "rb") as f:
        return f.read()


def _golden_lists_are_complete():
    t, c = {x[0] for x in GOLD_T}, {x[0] for x in GOLD_C}
    assert {"t_handmade", "uniform_no_rle", "textlike_m", "runs_default", "edges_forced_rle", "edge_tail_1", "edge_tail_7",
            "edge_tail_15", "edge_exact_K", "full_longtail_M", "full_zipf_M", "full_alt01_M"} <= t, sorted(t)
    assert {"uniform_no_rle", "textlike_m", "runs_default", "edges_forced_rle", "edge_tail_1", "edge_tail_7",
            "edge_tail_15"} <= c, sorted(c)
    assert "edge_bad_cod_mid" not in t


@pytest.mark.parametrize("case,freq,cod", GOLD_T, ids=[x[0] for x in GOLD_T])
def test_module_t_golden(shafa, case, freq, cod):
    _golden_lists_are_complete()
    want = _read(case, cod)
    for mis in (0, 7):
        assert _bytes(shafa.build_cod(_t(_read(case, freq), mis))) == want, f"{case}/{cod} (alignment {mis})"


@pytest.mark.parametrize("case,inp,cod,shaf", GOLD_C, ids=[x[0] for x in GOLD_C])
def test_module_c_golden(shafa, case, inp, cod, shaf):
    want = _read(case, shaf)
    for mis in (0, 3):
        got = shafa.encode_files(_t(_read(case, inp), mis), _t(_read(case, cod), 16 - mis & 15))
        assert _bytes(got) == want, f"{case}/{shaf} (alignment {mis})"


# ---------------------------------------------------------------- 3. parser parity
def _join(fields):
    return b";".join(fields)


def _texts():
    """name -> a block text, by hand; what each must give is the C host's answer (shafa.freq_parse)"""
    d20 = str(U64).encode()                                       # 20 digits
    t = {}
    t["zeros"] = _join([b"0"] + [b""] * 255)                      # 255 empty fields after one value
    t["ones"] = _join([b"1"] + [b""] * 255)
    t["max"] = _join([d20] + [b""] * 100 + [b"0"] + [b""] * 154)
    t["wraps to 0"] = _join([b"18446744073709551616", b"7"] + [b""] * 254)
    t["wraps to 4"] = _join([b"18446744073709551620"] + [b"1"] * 255)
    t["30 digits"] = _join([b"5"] * 9 + [b"123456789012345678901234567890"] + [b""] * 246)
    t["leading zeros"] = _join([b"000123", b"0000", b"00000000000000000000000000009"] + [b"01"] * 253)
    t["alternating"] = _join([str(3 * i + 1).encode() if i % 2 == 0 else b"" for i in range(256)])
    t["empty pairs"] = _join([str(i * i).encode() if i % 3 == 0 else b"" for i in range(256)])
    t["distinct"] = _join([str((i * 0x9E3779B97F4A7C15) & U64).encode() for i in range(256)])
    t["last only"] = _join([b"9"] + [b""] * 254 + [b"77"])
    t["field 0 empty"] = _join([b""] + [b"1"] * 255)
    t["only separators"] = b";" * 255
    t["255 fields"] = _join([b"4"] * 255)
    t["257 fields"] = _join([b"4"] * 257)
    t["letter"] = _join([b"12"] * 100 + [b"1a2"] + [b"3"] * 155)
    t["minus"] = _join([b"-1"] + [b"3"] * 255)
    t["space"] = _join([b"1"] * 255 + [b"2 "])
    t["nul before"] = _join([b"12"] * 17 + [b"1\x002"] + [b"3"] * 238)
    t["nul at 0"] = b"\x00" + _join([b"1"] * 256)
    t["nul in field 255"] = _join([b"8"] * 255 + [b"12\x0034"])
    t["nul and garbage after"] = _join([b"6"] * 256) + b"\x00;;x y;z\x00;9"
    t["one long field"] = _join([b"9" * 4000] + [b""] * 255)
    t["exactly 5375"] = _join([d20] * 256)
    assert len(t["exactly 5375"]) == 5375
    return t


def _freq_file(mode, sizes, texts, count=None):
    out = b"@" + mode + b"@" + str(len(sizes) if count is None else count).encode()
    for n, x in zip(sizes, texts):
        out += b"@" + str(int(n)).encode() + b"@" + x
    return out + b"@0"


def _host_counts(shafa, text):
    rc, f = shafa.freq_parse(text)
    return rc, ([int(x) for x in f] if rc == 0 else [0] * 256)


def _unpack(shafa, bt, st, mb, d_file):
    import torch
    dev = _dev()
    d_info = torch.zeros(8, dtype=torch.int64, device=dev)
    d_sizes = torch.full((mb,), -1, dtype=torch.int64, device=dev)
    d_counts = torch.full((mb * 256,), -1, dtype=torch.int64, device=dev)
    bt.unpack_freq(st, mb, d_file, d_info, d_sizes, d_counts)
    rc, errs = bt.finish(st, mb, raise_on_error=False)
    return _u64(d_info), _u64(d_sizes), np.array(_u64(d_counts), dtype=np.uint64).reshape(mb, 256), errs


def _hand_made_texts_cover_both_answers(shafa):
    rcs = {k: shafa.freq_parse(v)[0] for k, v in _texts().items()}
    bad = {k for k, rc in rcs.items() if rc}
    assert bad == {"field 0 empty", "only separators", "255 fields", "257 fields", "letter", "minus", "space", "nul before",
                   "nul at 0"}, bad
    assert set(rcs.values()) == {0, shafa.FILE_UNRECOGNIZABLE}
    f = shafa.freq_parse(_texts()["wraps to 0"])[1]
    assert int(f[0]) == 0 and int(f[1]) == 7
    assert int(shafa.freq_parse(_texts()["max"])[1][100]) == U64


@pytest.mark.parametrize("nb", [1, 2, 65, 300])
def test_parser_parity(shafa, nb):
    import torch
    pool = list(_texts().items())
    rng = np.random.default_rng(500 + nb)
    pick = list(range(len(pool))) if nb >= len(pool) else []
    pick += [int(rng.integers(len(pool))) for _ in range(nb - len(pick))]
    if nb == 2:
        pick = [[k for k, _ in pool].index("exactly 5375"), [k for k, _ in pool].index("letter")]
    rng.shuffle(pick)
    texts = [pool[i][1] for i in pick]
    edges = [0, 1, 9, 10, 1 << 63, U64, 1 << 64, (1 << 64) + 5]    # the last two wrap (read_u64)
    sizes = [edges[int(rng.integers(len(edges)))] if rng.random() < 0.5 else int(rng.integers(0, 1 << 40))
             for _ in range(nb)]
    file = _freq_file(b"NR"[nb & 1:][:1], sizes, texts)
    want = [_host_counts(shafa, x) for x in texts]
    mb = max(shafa.unpack_max_blocks(len(file), "counts"), nb) + 1
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(mb, 1 << 20)
    try:
        for mis in (range(16) if nb <= 2 else (0, 9)):
            d_file = _t(file, mis)
            info, got_sizes, counts, errs = _unpack(shafa, bt, st, mb, d_file)
            assert info[:6] == [0, ord("NR"[nb & 1]), nb, nb, nb, max(s & U64 for s in sizes)], info
            assert got_sizes == [s & U64 for s in sizes] + [0] * (mb - nb)
            for b in range(mb):
                rc, f = want[b] if b < nb else (0, [0] * 256)
                assert errs[b] == rc, f"block {b} ({pool[pick[b]][0] if b < nb else 'beyond'}), alignment {mis}"
                assert counts[b].tolist() == f, f"block {b} ({pool[pick[b]][0] if b < nb else 'beyond'}), alignment {mis}"
    finally:
        bt.close()


def test_frame_failure_and_fewer_slots_than_blocks(shafa):
    import torch
    _hand_made_texts_cover_both_answers(shafa)
    T = _texts()
    too_long = _join([str(U64).encode()] * 255 + [b"1" * 21])
    assert len(too_long) == 5376
    names = ["distinct", "letter", None, "ones", "alternating"]
    texts = [too_long if k is None else T[k] for k in names]
    file = _freq_file(b"N", [11, 22, 33, 44, 55], texts)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(8, 1 << 20)
    try:
        # a text of 5 376 bytes fails the frame: the blocks behind it are zeroed and silent, the ones before it are parsed
        info, sizes, counts, errs = _unpack(shafa, bt, st, 8, _t(file, 13))
        assert info[:6] == [0, ord("N"), 5, 5, 2, 22], info
        assert sizes == [11, 22, 0, 0, 0, 0, 0, 0]
        assert errs == [0, shafa.FILE_UNRECOGNIZABLE, shafa.FILE_STREAM_FAILED, 0, 0, 0, 0, 0]
        assert counts[0].tolist() == _host_counts(shafa, T["distinct"])[1] and not counts[1:].any()
        # the same file without that block, into three slots: the header's count stays, three blocks are looked at
        file = _freq_file(b"R", [11, 22, 44, 55], [x for x in texts if x is not too_long])
        info, sizes, counts, errs = _unpack(shafa, bt, st, 3, _t(file, 2))
        assert info[:6] == [0, ord("R"), 4, 3, 3, 44], info
        assert sizes == [11, 22, 44] and errs == [0, shafa.FILE_UNRECOGNIZABLE, 0]
        assert counts[2].tolist() == [1] * 256 and not counts[1].any()
        # bad headers: block 0 reports it, nothing is parsed
        for head in (b"", b"@", b"#N@1", b"@N@", b"@N@x", b"@N@9999"):
            info, sizes, counts, errs = _unpack(shafa, bt, st, 3, _t(head + file[4:] if head else b"", 1))
            assert info[0] == shafa.FILE_STREAM_FAILED and errs == [shafa.FILE_STREAM_FAILED, 0, 0], head
            assert sizes == [0, 0, 0] and not counts.any(), head
    finally:
        bt.close()


# ---------------------------------------------------------------- 4. round trips against the project's own chain
def _stream(shafa, kind, n, seed):
    synth = __import__("pkgload").load_submodule("synth")
    if kind == "zipf":
        return synth.gen_bytes(seed, n, synth.zipf_table(1.2))
    if kind == "runs":
        return synth.runs_stream(seed, n, synth.zipf_table(1.2))
    return synth.gen_bytes(seed, n)


@pytest.mark.parametrize("bs", [65536, 50001])
@pytest.mark.parametrize("kind", ["zipf", "runs", "uniform"])
def test_round_trip(shafa, kind, bs):
    import torch
    data = np.ascontiguousarray(_stream(shafa, kind, 3 * bs + 1234, 900 + bs % 100))
    for force_rle in (False, True):
        files = _files(shafa, data, bs, force_rle=force_rle)
        stem = ".rle" if ".rle.shaf" in files else ""
        assert not force_rle or stem
        src = files[".rle"] if stem else data.tobytes()
        for mis in (0, 5):
            cod = shafa.build_cod(_t(files[stem + ".freq"], mis))
            assert _bytes(cod) == files[stem + ".cod"], (kind, bs, force_rle, mis)
            shaf = shafa.encode_files(_t(src, mis), cod)            # mis = 5: a misaligned d_in view, gathered
            assert _bytes(shaf) == files[stem + ".shaf"], (kind, bs, force_rle, mis)
        back = shafa.decompress_files(shaf=shaf, cod=cod, decode_rle=bool(stem))
        assert _bytes(back) == data.tobytes(), (kind, bs, force_rle)
        # bytes of d_in beyond the sum of the sizes are ignored
        more = shafa.encode_files(torch.cat([_t(src), _t(b"tail that no block covers")]), _t(files[stem + ".cod"], 9))
        assert _bytes(more) == files[stem + ".shaf"]


# ---------------------------------------------------------------- 5. errors against the C host
def _host_module(shafa, tmp_path, module, files):
    """write the files to tmp_path as x<suffix> and run host/modules.c's get_shafa_codes ("t") or shafa_compress ("c") on
    them -> (rc, the bytes of the file it wrote)"""
    H = shafa.host()
    libc = C.CDLL(None)
    libc.strdup.restype = C.c_void_p
    libc.strdup.argtypes = [C.c_char_p]
    libc.free.argtypes = [C.c_void_p]
    C.c_bool.in_dll(H, "SHAFA_VERBOSE").value = False
    d = tmp_path / f"m{len(os.listdir(tmp_path))}"
    d.mkdir()
    for k, b in files.items():
        (d / ("x" + k)).write_bytes(b)
    base = str(d / "x")
    if module == "t":
        H.get_shafa_codes.argtypes = [C.c_char_p]
        H.get_shafa_codes.restype = C.c_int
        rc = H.get_shafa_codes(base.encode())
        written = base + ".cod"
    else:
        H.shafa_compress.argtypes = [C.POINTER(C.c_void_p)]
        H.shafa_compress.restype = C.c_int
        p = C.c_void_p(libc.strdup(base.encode()))
        rc = H.shafa_compress(C.byref(p))
        written = C.string_at(p.value).decode()
        libc.free(p)
    out = None
    if rc == 0:
        with open(written, "rb") as f:
            out = f.read()
    return rc, out


def _dev_module(shafa, module, files, mis=0):
    try:
        if module == "t":
            return 0, _bytes(shafa.build_cod(_t(files[".freq"], mis)))
        return 0, _bytes(shafa.encode_files(_t(files[""], mis), _t(files[".cod"], (mis * 7) % 16)))
    except shafa.ShafaError as e:
        return e.code, None


def _blocks(text):
    """.freq / .cod -> (head, [(size, text)], tail)"""
    parts = text.split(b"@")
    head = b"@".join(parts[:3])
    blocks = [(parts[3 + 2 * i], parts[4 + 2 * i]) for i in range((len(parts) - 4) // 2)]
    return head, blocks, b"@" + b"@".join(parts[3 + 2 * len(blocks):])


def _mut(text, edits):
    """block k's (size, text) replaced by edits[k](size, text)"""
    head, blocks, tail = _blocks(text)
    assert head + b"".join(b"@" + s + b"@" + x for s, x in blocks) + tail == text
    for k, fn in edits.items():
        blocks[k] = fn(*blocks[k])
    return head + b"".join(b"@" + s + b"@" + x for s, x in blocks) + tail


@pytest.fixture(scope="module")
def session(shafa):
    """a mode-N session of five blocks and a ragged sixth whose symbols stay below 200 (so that a larger byte has no code)"""
    synth = __import__("pkgload").load_submodule("synth")
    data = np.ascontiguousarray(synth.gen_bytes(78, 5 * 65536 + 300, synth.zipf_table(1.2, 200)))
    files = _files(shafa, data, 65536, force_plain=True)
    assert data.max() < 200 and ".rle.shaf" not in files
    return dict(files, **{"": data.tobytes()})


def test_module_t_errors_match_host(shafa, tmp_path, session):
    freq = session[".freq"]
    bad_count = lambda s, x: (s, x.replace(b";", b"x;", 1))
    bad_frame = lambda s, x: (s + b"a", x)
    cases = {
        "intact": freq,
        "empty file": b"",
        "no @": b"#" + freq[1:],
        "no second @": b"@N#" + freq[3:],
        "no count": b"@N@" + freq[freq.index(b"@", 3):],
        "count too large": b"@N@99999" + freq[freq.index(b"@", 3):],
        "25-digit count": b"@N@" + b"1" * 25 + freq[freq.index(b"@", 3):],
        "mode X": b"@X" + freq[2:],
        "mode R": b"@R" + freq[2:],
        "count 0": b"@N@0",
        "count 0, mode R, a tail": b"@R@0@0",
        "fewer blocks than there are": b"@N@3" + freq[4:],
        "no last @": freq[:-2],
        "truncated mid text": freq[:len(freq) // 2],
        "empty text": _mut(freq, {2: lambda s, x: (s, b"")}),
        "empty size": _mut(freq, {1: lambda s, x: (b"", x)}),
        "bad count field in block 3": _mut(freq, {3: bad_count}),
        "256th separator in block 0": _mut(freq, {0: lambda s, x: (s, x + b";")}),
        "NUL in block 4": _mut(freq, {4: lambda s, x: (s, x[:40] + b"\x00" + x[41:])}),
        "two faults: counts in 1, frame in 4": _mut(freq, {1: bad_count, 4: bad_frame}),
        "two faults: frame in 1, counts in 4": _mut(freq, {1: bad_frame, 4: bad_count}),
        "two faults: counts in 2 and 5": _mut(freq, {2: bad_count, 5: lambda s, x: (s, b";" + x)}),
    }
    seen = set()
    for name, text in cases.items():
        want = _host_module(shafa, tmp_path, "t", {".freq": text})
        got = _dev_module(shafa, "t", {".freq": text}, mis=len(name) % 16)
        assert got == want, f"{name}: device {got[0]}, host {want[0]}"
        seen.add(want[0])
    assert seen == {0, shafa.FILE_STREAM_FAILED, shafa.FILE_UNRECOGNIZABLE}, seen
    assert _dev_module(shafa, "t", {".freq": b"@N@0"}) == (0, b"@N@0@0")
    assert _dev_module(shafa, "t", {".freq": b"@X" + freq[2:]})[0] == shafa.FILE_UNRECOGNIZABLE


def test_module_c_errors_match_host(shafa, tmp_path, session):
    cod, data = session[".cod"], session[""]
    no_code = bytearray(data)
    no_code[2 * 65536 + 777] = 250
    cases = {
        "intact": (data, cod),
        "no @": (data, b"#" + cod[1:]),
        "no count": (data, b"@N@" + cod[cod.index(b"@", 3):]),
        "count too large": (data, b"@N@99999" + cod[cod.index(b"@", 3):]),
        "empty file": (data, b""),
        "mode X": (data, b"@X" + cod[2:]),
        "count 0": (data, b"@N@0@0"),
        "count 0, no input": (b"", b"@R@0"),
        "no last @": (data, cod[:-2]),
        "truncated mid text": (data, cod[:len(cod) // 2]),
        "bad table in block 3": (data, _mut(cod, {3: lambda s, x: (s, x.replace(b"0", b"2", 1))})),
        "257 fields in block 0": (data, _mut(cod, {0: lambda s, x: (s, x + b";")})),
        "block 4 larger than what is left": (data, _mut(cod, {4: lambda s, x: (str(2 * 65536 + 1).encode(), x)})),
        "input one byte short": (data[:-1], cod),
        "input longer": (data + b"more", cod),
        "a symbol without a code in block 2": (bytes(no_code), cod),
    }
    seen = set()
    for name, (d, c) in cases.items():
        want = _host_module(shafa, tmp_path, "c", {"": d, ".cod": c})
        got = _dev_module(shafa, "c", {"": d, ".cod": c}, mis=len(name) % 16)
        assert got == want, f"{name}: device {got[0]}, host {want[0]}"
        seen.add(want[0])
    assert seen == {0, shafa.FILE_STREAM_FAILED, shafa.FILE_UNRECOGNIZABLE}, seen
    assert _dev_module(shafa, "c", {"": data, ".cod": b"@N@0@0"}) == (0, b"@0")
    assert _dev_module(shafa, "c", {"": data, ".cod": b"@X" + cod[2:]}) == (0, session[".shaf"])
    assert _dev_module(shafa, "c", {"": bytes(no_code), ".cod": cod})[0] == shafa.FILE_UNRECOGNIZABLE


# ---------------------------------------------------------------- 6. nothing outside the arrays
def test_nothing_written_outside(shafa):
    import torch
    T = _texts()
    names = ["distinct", "letter", "max", "alternating", "exactly 5375", "ones", "nul before"]
    file = _freq_file(b"N", list(range(100, 107)), [T[k] for k in names])
    dev = _dev()
    g = 256
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(16, 1 << 20)
    try:
        for mb in (4, 7, 12):                                  # fewer slots than blocks, as many, more
            info = torch.full((8 + 2 * g,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
            sizes = torch.full((mb + 2 * g,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
            counts = torch.full(((mb + 2) * 256,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
            d_file = _t(file, 11)
            bt.unpack_freq(st, mb, d_file, info[g:g + 8], sizes[g:g + mb], counts[256:256 + mb * 256])
            _, errs = bt.finish(st, mb, raise_on_error=False)
            k = min(mb, 7)
            assert errs[:k] == [shafa.FILE_UNRECOGNIZABLE if n in ("letter", "nul before") else 0 for n in names[:k]]
            for a, n in ((info, 8), (sizes, mb)):
                v = a.cpu().numpy().view(np.uint64)
                assert (v[:g] == CANARY).all() and (v[g + n:] == CANARY).all()
            v = counts.cpu().numpy().view(np.uint64)
            assert (v[:256] == CANARY).all() and (v[256 + mb * 256:] == CANARY).all()
            assert not (v[256:256 + mb * 256] == CANARY).any()
            assert _u64(sizes[g:g + mb]) == list(range(100, 100 + k)) + [0] * (mb - k)
            assert v[256:512].tolist() == _host_counts(shafa, T["distinct"])[1]
    finally:
        bt.close()


# ---------------------------------------------------------------- 7. enqueue only
def test_no_synchronisation_inside_unpack_freq(shafa):
    import torch
    T = _texts()
    pool = [T[k] for k in ("distinct", "alternating", "max", "ones")]
    nb = 64
    file = _freq_file(b"N", [7] * nb, [pool[b % 4] for b in range(nb)])
    dev = _dev()
    d_file = _t(file, 6)
    mb = shafa.unpack_max_blocks(len(file), "counts")
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    sizes = torch.zeros(mb, dtype=torch.int64, device=dev)
    counts = torch.zeros(mb * 256, dtype=torch.int64, device=dev)
    bt = shafa.Batch(mb, 1 << 20)
    st = torch.cuda.Stream(device=dev)
    try:
        bt.unpack_freq(st, mb, d_file, info, sizes, counts)             # warm-up: the batch grows here
        bt.finish(st, mb)
        counts.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)
        bt.unpack_freq(st, mb, d_file, info, sizes, counts)
        busy = not st.query()
        bt.finish(st, mb)
        assert busy, "the stream had drained when the call returned: something synchronised"
        got = np.array(_u64(counts), dtype=np.uint64).reshape(mb, 256)
        for b in range(nb):
            assert got[b].tolist() == _host_counts(shafa, pool[b % 4])[1]
    finally:
        bt.close()

"""Files held in device memory, parsed and decoded there (shafa_hipd_unpack_cod / _unpack_rle_freq / _unpack_shaf /
_unpack_payloads, csrc/unpack.hip) and shafa.decompress_files, which chains them with the device decoders.

1. decompress_files reproduces every golden session's decoded__* file from the files compress_files makes;
2. unpack_cod / unpack_shaf equal the C host's parser (shafa.cod_parse) and a walk written from shaf_read_u64;
3. compress_files -> decompress_files round trips: block sizes, forced RLE / plain, misaligned files, RLE in groups;
4. a corpus of single-fault files raises the code the C host's Module D returns on the same bytes (ctypes, in process);
5. nothing is written outside the caller's arrays and regions;
6. the calls only enqueue."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_pack import _case_input, _cod_text, _opt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BLOCK = {"K": 655360, "m": 8 << 20, "M": 64 << 20}
GUARD = 256
FILL = 0xA5


def _dev():
    import torch
    return torch.device("cuda", 0)


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _t(b, mis=0):
    """bytes -> a uint8 CUDA tensor view whose address is `mis` bytes past a 256-byte boundary"""
    import torch
    base = torch.zeros(len(b) + 512, dtype=torch.uint8, device=_dev())
    k = (-base.data_ptr()) % 256 + mis
    v = base[k:k + len(b)]
    if len(b):
        v.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return v


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


# ---------------------------------------------------------------- the C host's Module D, in process
def _host_decode(shafa, tmp_path, files, decode_rle=True):
    """write the files to tmp_path and run host/modules.c's shafa_decompress or rle_decompress on them -> (rc, bytes)"""
    H = shafa.host()
    libc = C.CDLL(None)
    libc.strdup.restype = C.c_void_p
    libc.strdup.argtypes = [C.c_char_p]
    libc.free.argtypes = [C.c_void_p]
    C.c_bool.in_dll(H, "SHAFA_VERBOSE").value = False
    d = tmp_path / f"h{len(os.listdir(tmp_path))}"
    d.mkdir()
    for k, b in files.items():
        (d / ("x" + k)).write_bytes(b)
    if ".shaf" in files or ".rle.shaf" in files:
        name = "x.rle.shaf" if ".rle.shaf" in files else "x.shaf"
        fn = H.shafa_decompress
        fn.argtypes = [C.POINTER(C.c_void_p), C.c_bool]
        args = (decode_rle,)
    else:
        name = "x.rle"
        fn = H.rle_decompress
        fn.argtypes = [C.POINTER(C.c_void_p)]
        args = ()
    fn.restype = C.c_int
    p = C.c_void_p(libc.strdup(str(d / name).encode()))
    rc = fn(C.byref(p), *args)
    out = None
    if rc == 0:
        with open(C.string_at(p.value).decode(), "rb") as f:
            out = f.read()
    libc.free(p)
    return rc, out


def _dev_decode(shafa, files, decode_rle=True, mis=0, **kw):
    """decompress_files on the same files -> (rc, bytes)"""
    if ".rle.shaf" in files or ".shaf" in files:
        k = ".rle" if ".rle.shaf" in files else ""
        args = dict(shaf=_t(files[k + ".shaf"], mis), cod=_t(files[k + ".cod"], (mis * 7) % 16), decode_rle=decode_rle)
    else:
        args = dict(rle=_t(files[".rle"], mis), freq=_t(files[".rle.freq"], (mis * 3) % 16))
    try:
        return 0, _bytes(shafa.decompress_files(**args, **kw))
    except shafa.ShafaError as e:
        return e.code, None


def _files(shafa, data, bs, force_rle=False, force_plain=False):
    """compress_files -> {suffix: bytes}; force_plain: the input has no RLE session (mode N)"""
    import torch
    out = shafa.compress_files(torch.from_numpy(np.ascontiguousarray(data)).to(_dev()), bs, force_rle=force_rle)
    got = {k: _bytes(v) for k, v in out.items()}
    if force_plain:
        assert ".shaf" in got, sorted(got)
    return got


# ---------------------------------------------------------------- 1. golden sessions
def _man(case):
    with open(os.path.join(GOLD, case, "manifest.json")) as f:
        return json.load(f)


def _decoded_cases():
    out = []
    for c in sorted(os.listdir(GOLD)):
        p = os.path.join(GOLD, c, "manifest.json")
        if os.path.exists(p) and any(k.startswith("decoded__") for k in _man(c)["files"]):
            out.append(c)
    return out


DECODED = _decoded_cases()


def _decode_rcs(man):
    """decoded__* name -> the exit status of the reference command whose output the session copied under that name"""
    cmds = [c if isinstance(c, dict) else {"argv": c, "rc": 0} for c in man["cmds"]]
    return {n["argv"][2]: c["rc"] for c, n in zip(cmds, cmds[1:])
            if n["argv"][0] == "__copy__" and n["argv"][2].startswith("decoded__")}


def test_golden_list_is_complete():
    assert len(DECODED) == 19, DECODED


@pytest.mark.parametrize("case", DECODED)
def test_golden_sessions_decode(shafa, case):
    import torch
    man = _man(case)
    argv = man["cmds"][0]["argv"]
    fn = argv[0]
    data, S = _case_input(shafa, case, man, fn)
    try:
        assert _sha(data.tobytes()) == man["files"][fn]["sha256"]
        c = _opt(argv, "-c")
        bs = BLOCK.get(_opt(argv, "-b"), 65536)
        files = shafa.compress_files(torch.from_numpy(data).to(_dev()), bs, force_rle=c == "r", force_freq=c == "f")
        del data
        checked = 0
        rcs = _decode_rcs(man)
        for key, meta in man["files"].items():
            if not key.startswith("decoded__"):
                continue
            kind = key[len("decoded__"):]
            if kind == "rle_only":
                run = lambda: shafa.decompress_files(rle=files[".rle"], freq=files[".rle.freq"])
            elif kind == "sf_rle":
                run = lambda: shafa.decompress_files(shaf=files[".rle.shaf"], cod=files[".rle.cod"], decode_rle=True)
            else:                                       # sf / sf_only: `X.shaf -m d`, or `X.rle.shaf -m d -d s`
                k = ".rle" if ".rle.shaf" in files else ""
                run = lambda: shafa.decompress_files(shaf=files[k + ".shaf"], cod=files[k + ".cod"], decode_rle=False)
            checked += 1
            if rcs[key] != 0:
                # the reference crashed (a last block of one byte: a single-symbol block, every code empty, d.c:533) and
                # left a partial file; ours refuses that block as the CLI does (tests/test_cli.py)
                with pytest.raises(shafa.ShafaError) as e:
                    run()
                assert e.value.code == shafa.FILE_UNRECOGNIZABLE
                continue
            out = run()
            assert out.numel() == meta["size"], f"{case}/{key}: {out.numel()} bytes, the reference wrote {meta['size']}"
            assert _sha(_bytes(out)) == meta["sha256"], f"{case}/{key} differs from the reference's"
        assert checked
    finally:
        if S is not None:
            S.close()


# ---------------------------------------------------------------- 2. parse parity
def _random_table(shafa, rng, kind):
    t = shafa.CodeTable()
    if kind == "empty":
        return t
    nsym = int(rng.integers(1, 257))
    syms = rng.choice(256, nsym, replace=False)
    budget = 33151 - 255                                 # SHAFA_COD_BLOCK_MAX: a longer text is a framing error
    for s in syms:
        ln = int(rng.choice([0, 1, 2, 7, 8, 9, 31, 32, 33, 64, 100, 254, 255])) if kind == "wild" else int(rng.integers(1, 20))
        ln = min(ln, budget)
        budget -= ln
        t.len[s] = ln
        for i in range(ln):
            if rng.random() < 0.5:
                t.bits[s][i >> 3] |= 0x80 >> (i & 7)
    return t


def _cod_file(mode, sizes, texts):
    out = b"@" + mode + b"@" + str(len(sizes)).encode()
    for n, t in zip(sizes, texts):
        out += b"@" + str(int(n)).encode() + b"@" + t
    return out + b"@0"


def _shaf_walk(b):
    """shaf_read_u64 (host/modules.c) over a .shaf: -> [(off, n)], or the index of the failing block (-1: the header)"""
    def rd(p, trailing):
        w = b[p:p + 32]
        if len(w) < 2 or w[0:1] != b"@":
            return None
        i, x = 1, 0
        while i < len(w) and 48 <= w[i] <= 57 and i <= 20:
            x = (x * 10 + w[i] - 48) % (1 << 64)
            i += 1
        if i == 1:
            return None
        if trailing:
            if i >= len(w) or w[i:i + 1] != b"@":
                return None
            i += 1
        return x, p + i
    h = rd(0, False)
    if h is None:
        return -1
    count, p = h
    out = []
    for k in range(count):
        r = rd(p, True)
        if r is None or r[0] > len(b) - r[1]:
            return k
        out.append((r[1], r[0]))
        p = r[1] + r[0]
    return out


@pytest.mark.parametrize("nb", [1, 2, 37, 300])
def test_parse_parity(shafa, nb):
    import torch
    rng = np.random.default_rng(100 + nb)
    kinds = ["wild", "plain", "empty"]
    tables = [_random_table(shafa, rng, kinds[int(rng.integers(3))]) for _ in range(nb)]
    texts = [_cod_text(shafa, t) for t in tables]
    edges = [0, 1, 9, 10, 2 ** 63, 2 ** 64 - 1]
    sizes = [edges[int(rng.integers(len(edges)))] if rng.random() < 0.5 else int(rng.integers(0, 1 << 40))
             for _ in range(nb)]
    cod = _cod_file(b"R", sizes, texts)
    pays = [rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8).tobytes() for _ in range(nb)]
    shaf = b"@" + str(nb).encode() + b"".join(b"@" + str(len(p)).encode() + b"@" + p for p in pays)
    dev = _dev()
    mb = shafa.unpack_max_blocks(len(cod), "cod")
    assert mb >= nb
    tsz = C.sizeof(shafa.CodeTable)
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(mb, 1 << 20)
    try:
        for mis in (0, 5):
            d_info = torch.zeros(8, dtype=torch.int64, device=dev)
            d_sizes = torch.full((mb,), -1, dtype=torch.int64, device=dev)
            d_tab = torch.full((mb * tsz,), 7, dtype=torch.uint8, device=dev)
            d_off = torch.full((mb,), -1, dtype=torch.int64, device=dev)
            d_n = torch.full((mb,), -1, dtype=torch.int64, device=dev)
            # the inputs are held until the stream is through: a tensor torch frees may be handed out again at once
            d_cod, d_shaf = _t(cod, mis), _t(shaf, 15 - mis)
            bt.unpack_cod(st, mb, d_cod, d_info, d_sizes, d_tab)
            bt.unpack_shaf(st, mb, d_shaf, d_info[3:4], d_off, d_n)
            rc, errs = bt.finish(st, mb, raise_on_error=False)
            assert rc == 0, errs
            info = _u64(d_info)
            assert info[:6] == [0, ord("R"), nb, nb, nb, max(sizes)], info
            assert _u64(d_sizes) == sizes + [0] * (mb - nb)
            raw = _bytes(d_tab)
            for b in range(mb):
                want = bytes(shafa.cod_parse(texts[b])[1]) if b < nb else bytes(tsz)
                if b < nb:
                    assert shafa.cod_parse(texts[b])[0] == 0
                assert raw[b * tsz:(b + 1) * tsz] == want, f"table {b}"
            walk = _shaf_walk(shaf)
            assert [(o, n) for o, n in zip(_u64(d_off), _u64(d_n))][:nb] == walk
            assert _u64(d_n)[nb:] == [0] * (mb - nb)
    finally:
        bt.close()


# ---------------------------------------------------------------- 3. round trips
@pytest.mark.parametrize("n,bs", [(1024, 512), (70001, 512), (200003, 65536), (655360 * 2 + 77, 655360),
                                  (3 * (8 << 20) + 12345, 8 << 20), ((64 << 20) + 999, 64 << 20)])
@pytest.mark.parametrize("kind", ["zipf", "runs"])
def test_round_trip(shafa, n, bs, kind):
    import golden.make_golden as mg
    zt = mg.zipf_table(1.2)
    data = mg.gen_bytes(7000 + n % 1000, n) if kind == "zipf" else mg.runs_stream(8000 + n % 1000, n, zt)
    for force_rle in ((False, True) if n < (8 << 20) else (False,)):
        files = _files(shafa, data, bs, force_rle=force_rle)
        stem = ".rle" if ".rle.shaf" in files else ""
        for mis in ((0, 1, 9, 15) if n < (1 << 20) else (0, 3)):
            rc, out = _dev_decode(shafa, files, decode_rle=bool(stem), mis=mis)
            assert rc == 0 and out == data.tobytes(), (kind, n, bs, force_rle, mis, rc)
            if stem:
                rc, out = _dev_decode(shafa, {k: files[k] for k in (".rle", ".rle.freq")}, mis=mis)
                assert rc == 0 and out == data.tobytes()
                rc, out = _dev_decode(shafa, {k: files[k] for k in (".rle.shaf", ".rle.cod")}, decode_rle=False, mis=mis)
                assert rc == 0 and out == files[".rle"]


def test_rle_groups_match_one_group(shafa):
    import golden.make_golden as mg
    data = mg.runs_stream(31, 40 * 65536 + 5, mg.zipf_table(1.2))
    files = _files(shafa, data, 65536, force_rle=True)
    assert ".rle.shaf" in files
    one = _dev_decode(shafa, files)
    cap = 85 * 65536 + 2
    many = _dev_decode(shafa, files, max_bytes=cap * 4)                 # groups of a few blocks: >= 3 groups
    assert one == many == (0, data.tobytes())
    rle = {k: files[k] for k in (".rle", ".rle.freq")}
    assert _dev_decode(shafa, rle, max_bytes=1) == (0, data.tobytes())  # one block per group


def test_empty_session(shafa):
    """a .cod and .shaf of 0 blocks decode to 0 bytes, as on the host"""
    assert _dev_decode(shafa, {".shaf": b"@0", ".cod": b"@N@0@0"}, decode_rle=False) == (0, b"")


# ---------------------------------------------------------------- 4. single faults against the C host
def _session(shafa):
    import golden.make_golden as mg
    data = mg.runs_stream(77, 5 * 65536 + 300, mg.zipf_table(1.2))
    rle = _files(shafa, data, 65536, force_rle=True)
    plain = _files(shafa, mg.gen_bytes(78, 5 * 65536 + 300), 65536)
    assert ".rle.shaf" in rle and ".shaf" in plain and ".rle.shaf" not in plain
    return rle, plain


def _cod_blocks(cod):
    """.cod -> (head, [(size, text)], tail)"""
    parts = cod.split(b"@")
    head = b"@".join(parts[:3])
    blocks = [(parts[3 + 2 * i], parts[4 + 2 * i]) for i in range((len(parts) - 4) // 2)]
    return head, blocks, b"@" + b"@".join(parts[3 + 2 * len(blocks):])


def _cod_join(head, blocks, tail):
    return head + b"".join(b"@" + s + b"@" + t for s, t in blocks) + tail


def _cod_mut(cod, k, fn):
    head, blocks, tail = _cod_blocks(cod)
    assert _cod_join(head, blocks, tail) == cod
    s, t = blocks[k]
    blocks[k] = fn(s, t)
    return _cod_join(head, blocks, tail)


def _shaf_mut(shaf, k, fn):
    walk = _shaf_walk(shaf)
    off, n = walk[k]
    hs = shaf.rfind(b"@", 0, off - 1)
    return fn(shaf, hs, off, n)


def _corpus(rle, plain):
    cod, shaf = rle[".rle.cod"], rle[".rle.shaf"]
    c = {}
    fields = lambda t: t.split(b";")
    c["cod bad char"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 2, lambda s, t: (s, t.replace(b"0", b"2", 1)))}), True)
    c["cod 257 fields"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 1, lambda s, t: (s, t + b";"))}), True)
    c["cod 255 fields"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 3, lambda s, t: (s, b";".join(fields(t)[:-1])))}), True)
    c["cod 256-bit code"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 0, lambda s, t: (s, b"1" * 256 + t))}), True)
    c["cod empty text"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 2, lambda s, t: (s, b""))}), True)
    c["cod no trailing @"] = (dict(rle, **{".rle.cod": cod[:cod.rfind(b"@")]}), True)
    c["cod count too large"] = (dict(rle, **{".rle.cod": b"@R@99999" + cod[cod.index(b"@", 3):]}), True)
    c["cod mode N with rle"] = (dict(rle, **{".rle.cod": b"@N" + cod[2:]}), True)
    c["cod mode X"] = (dict(rle, **{".rle.cod": b"@X" + cod[2:]}), True)
    c["cod 25-digit count"] = (dict(rle, **{".rle.cod": b"@R@" + b"1" * 25 + cod[cod.index(b"@", 3):]}), True)
    c["cod bad char, plain"] = (dict(plain, **{".cod": _cod_mut(plain[".cod"], 4, lambda s, t: (s, b"x" + t))}), False)
    c["cod empty size"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 1, lambda s, t: (b"", t))}), True)
    c["cod huge symbol count"] = (dict(rle, **{".rle.cod": _cod_mut(cod, 2, lambda s, t: (b"9" * 12, t))}), True)
    c["shaf 21-digit size"] = (dict(rle, **{".rle.shaf": _shaf_mut(shaf, 1, lambda b, h, o, n: b[:h] + b"@" + b"0" * 21
                                                                    + b[h + 1:])}), True)
    c["shaf missing @"] = (dict(rle, **{".rle.shaf": _shaf_mut(shaf, 2, lambda b, h, o, n: b[:o - 1] + b"0" + b[o:])}), True)
    c["shaf size past end"] = (dict(rle, **{".rle.shaf": _shaf_mut(
        shaf, 4, lambda b, h, o, n: b[:h] + b"@" + str(n + len(b) - o - n + 1).encode() + b"@" + b[o:])}), True)
    c["shaf truncated"] = (dict(rle, **{".rle.shaf": shaf[:-3]}), True)
    c["shaf trailing bytes"] = (dict(rle, **{".rle.shaf": shaf + b"@12@junk"}), True)
    c["shaf other count"] = (dict(rle, **{".rle.shaf": b"@9" + shaf[2:]}), True)
    c["shaf bad header"] = (dict(rle, **{".rle.shaf": b"#" + shaf[1:]}), True)
    freq = rle[".rle.freq"]
    only = {k: rle[k] for k in (".rle", ".rle.freq")}
    c["freq mode N"] = (dict(only, **{".rle.freq": b"@N" + freq[2:]}), None)
    second = freq.index(b"@", freq.index(b"@", 4) + 1)                     # "@<n>@<size>@": the first block's text
    c["freq empty text"] = (dict(only, **{".rle.freq": freq[:second + 1] + freq[freq.index(b"@", second + 1):]}), None)
    c["freq size past end"] = (dict(only, **{".rle.freq": freq[:5] + str(len(rle[".rle"]) + 1).encode()
                                               + freq[freq.index(b"@", 5):]}), None)
    c["rle truncated"] = (dict(only, **{".rle": rle[".rle"][:-1]}), None)
    c["rle trailing bytes"] = (dict(only, **{".rle": rle[".rle"] + b"xyz"}), None)
    c["shaf payload bit flip"] = (dict(rle, **{".rle.shaf": shaf[:-40] + bytes([shaf[-40] ^ 0xFF]) + shaf[-39:]}), True)
    return c


def test_single_fault_corpus_matches_host(shafa, tmp_path):
    rle, plain = _session(shafa)
    cases = _corpus(rle, plain)
    bad = os.path.join(GOLD, "edge_bad_cod_mid")
    stored = {k: open(os.path.join(bad, "g" + k), "rb").read() for k in (".rle.cod", ".rle.freq", ".rle.shaf")}
    cases["edge_bad_cod_mid (stored)"] = ({k: stored[k] for k in (".rle.cod", ".rle.shaf")}, True)
    seen = set()
    for name, (files, decode_rle) in cases.items():
        sf = ".shaf" in files or ".rle.shaf" in files
        want = _host_decode(shafa, tmp_path, files, bool(decode_rle) if sf else True)
        got = _dev_decode(shafa, files, decode_rle=bool(decode_rle) if sf else True, mis=len(name) % 16)
        assert got == want, f"{name}: device {got[0]}, host {want[0]}"
        seen.add(want[0])
    assert {0, shafa.FILE_STREAM_FAILED, shafa.FILE_UNRECOGNIZABLE} <= seen, seen


# ---------------------------------------------------------------- 5. nothing outside the arrays and regions
def test_nothing_written_outside(shafa):
    import torch
    rle, _ = _session(shafa)
    dev = _dev()
    tsz = C.sizeof(shafa.CodeTable)
    head, blocks, tail = _cod_blocks(rle[".rle.cod"])
    damaged = _cod_mut(rle[".rle.cod"], 2, lambda s, t: (s, b"7" + t))
    for cod, want_err in ((rle[".rle.cod"], 0), (damaged, shafa.FILE_UNRECOGNIZABLE)):
        mb = shafa.unpack_max_blocks(len(cod), "cod")
        bt = shafa.Batch(mb, 1 << 20)
        st = torch.cuda.Stream(device=dev)
        try:
            g = GUARD
            info = torch.full((8 + 2 * g,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
            arrs = [torch.full((mb + 2 * g,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev) for _ in range(3)]
            tab = torch.full(((mb + 2) * tsz,), FILL, dtype=torch.uint8, device=dev)
            d_cod, d_shaf = _t(cod, 3), _t(rle[".rle.shaf"], 11)
            bt.unpack_cod(st, mb, d_cod, info[g:g + 8], arrs[0][g:g + mb], tab[tsz:tsz + mb * tsz])
            bt.unpack_shaf(st, mb, d_shaf, info[g + 3:g + 4], arrs[1][g:g + mb], arrs[2][g:g + mb])
            _, errs = bt.finish(st, mb, raise_on_error=False)
            assert (errs[2] if want_err else max(errs)) == want_err, errs
            for a, n in ((info, 8), *((x, mb) for x in arrs)):
                v = a.cpu().numpy().view(np.uint64)
                assert (v[:g] == 0xA5A5A5A5A5A5A5A5).all() and (v[g + n:] == 0xA5A5A5A5A5A5A5A5).all()
            t = tab.cpu().numpy()
            assert (t[:tsz] == FILL).all() and (t[tsz + mb * tsz:] == FILL).all()
            # the payloads into regions with guards: one region too small for its payload (nothing written for it)
            nb = len(blocks)
            pn = _u64(arrs[2][g:g + nb])
            caps = [n if b != 1 else n - 1 for b, n in enumerate(pn)]
            off, pos = [], 16
            for c in caps:
                off.append(pos)
                pos += (c + 15) // 16 * 16 + 64
            dst = torch.full((pos + 64,), FILL, dtype=torch.uint8, device=dev)
            bt.unpack_payloads(st, d_shaf, arrs[1][g:], arrs[2][g:], dst, off, caps)
            _, errs = bt.finish(st, mb, raise_on_error=False)
            assert errs[:nb] == [0, shafa.OUTSIDE_MODULE] + [0] * (nb - 2), errs
            d = _bytes(dst)
            po = _u64(arrs[1][g:g + nb])
            shaf = rle[".rle.shaf"]
            mask = np.zeros(len(d), dtype=bool)
            for b in range(nb):
                if b == 1:
                    continue
                assert d[off[b]:off[b] + pn[b]] == shaf[po[b]:po[b] + pn[b]], f"payload {b}"
                mask[off[b]:off[b] + pn[b]] = True
            assert (np.frombuffer(d, dtype=np.uint8)[~mask] == FILL).all(), "bytes written outside the payloads"
        finally:
            bt.close()


# ---------------------------------------------------------------- 6. enqueue only
def test_no_synchronisation_inside_the_calls(shafa):
    import torch
    import golden.make_golden as mg
    data = mg.runs_stream(5, 4 * 65536 + 17, mg.zipf_table(1.2))
    files = _files(shafa, data, 65536, force_rle=True)
    dev = _dev()
    cod, shaf, rle, freq = (_t(files[k], m) for k, m in ((".rle.cod", 1), (".rle.shaf", 2), (".rle", 3), (".rle.freq", 4)))
    mb = shafa.unpack_max_blocks(cod.numel(), "cod")
    tsz = C.sizeof(shafa.CodeTable)
    info, info2 = (torch.zeros(8, dtype=torch.int64, device=dev) for _ in range(2))
    nsym, poff, pn, roff, rn, dn = (torch.zeros(mb, dtype=torch.int64, device=dev) for _ in range(6))
    tab = torch.zeros(mb * tsz, dtype=torch.uint8, device=dev)
    bt = shafa.Batch(mb, 1 << 20)
    st = torch.cuda.Stream(device=dev)
    # the shapes, from one parse (the driver reads them back; here they are taken once, before the timed enqueue)
    bt.unpack_cod(st, mb, cod, info, nsym, tab)
    bt.unpack_shaf(st, mb, shaf, info[3:4], poff, pn)
    bt.finish(st, mb)
    nb = _u64(info)[3]
    ns, ps = _u64(nsym)[:nb], _u64(pn)[:nb]
    al = lambda v: [sum((x + 15) // 16 * 16 for x in v[:i]) for i in range(len(v))]
    po, so = al(ps), al(ns)
    rcap = [85 * n + 2 for n in ns]
    ro = al(rcap)
    pay = torch.zeros(sum(ps) + 16 * nb + 16, dtype=torch.uint8, device=dev)
    sfo = torch.zeros(sum(ns) + 16 * nb + 16, dtype=torch.uint8, device=dev)
    ro_buf = torch.zeros(sum(rcap) + 16 * nb + 16, dtype=torch.uint8, device=dev)
    out = torch.zeros(data.size + 16, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)

    def enqueue():
        bt.unpack_cod(st, mb, cod, info, nsym, tab)
        bt.unpack_shaf(st, mb, shaf, info[3:4], poff, pn)
        bt.unpack_rle_freq(st, mb, freq, rle.numel(), info2, roff, rn)
        bt.unpack_payloads(st, shaf, poff, pn, pay, po, ps)
        bt.sf_decode_dev(st, pay, po, ps, pn, tab, nsym, sfo, so, ns)
        bt.rle_decode_dev(st, sfo, so, ns, nsym, ro_buf, ro, rcap, dn)
        bt.pack_payloads(st, shafa.FRAME_RAW, ro_buf, ro, rcap, dn, out, out.numel(), d_len)

    try:
        enqueue()                                                       # warm-up: the batch grows here
        bt.finish(st, mb)
        out.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)
        enqueue()
        busy = not st.query()
        bt.finish(st, mb)
        assert busy, "the stream had drained when the calls returned: something synchronised"
        assert int(d_len.item()) == data.size and _bytes(out[:data.size]) == data.tobytes()
    finally:
        bt.close()

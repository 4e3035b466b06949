"""Many file sets per call, parsed and decoded on the device: the segmented parses (shafa_hipd_unpack_cod_files /
_unpack_rle_freq_files / _unpack_shaf_files, csrc/unpack.hip) and shafa.decompress_many.

1. every slot, error word and record of a segmented parse equals the single-file parse of that file (offsets shifted by the
   file's base); nothing is written between the files' slot ranges or around the arrays;
2. all golden decode sessions in one decompress_many call;
3. the single-fault corpus interleaved with intact files: each result equals decompress_files on that entry;
4. compress_many -> decompress_many round trips over 1 000 small files, RLE and plain mixed, in every form;
5. blocks with 33..64-bit codes in several files of one call;
6. more than MANY_GROUP_BLOCKS blocks, and RLE decoding in several groups;
7. the synchronisations of a call do not grow with its file count;
8. the segmented parses only enqueue."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_pack import _cod_text
from test_gpu_unpack import (DECODED, GOLD, _bytes, _case_input, _cod_file, _corpus, _decode_rcs, _dev, _dev_decode, _man,
                             _opt, _session, _sha, _t, _u64, BLOCK)

pytestmark = pytest.mark.gpu

SENT = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64
G = 3                               # free slots in front of every file's range and around every array


def _entry(files, decode_rle=True, mis=0):
    """{suffix: bytes} -> a decompress_many entry (device tensors at `mis` past a 256-byte boundary)"""
    if ".rle.shaf" in files or ".shaf" in files:
        k = ".rle" if ".rle.shaf" in files else ""
        return dict(shaf=_t(files[k + ".shaf"], mis), cod=_t(files[k + ".cod"], (mis * 7) % 16), decode_rle=decode_rle)
    return dict(rle=_t(files[".rle"], mis), freq=_t(files[".rle.freq"], (mis * 3) % 16))


def _result(r):
    import torch
    return (0, _bytes(r)) if isinstance(r, torch.Tensor) else (r.code, None)


# ---------------------------------------------------------------- 1. parse parity
def _parity_sets(shafa):
    rle, plain = _session(shafa)
    corpus = _corpus(rle, plain)
    sets = [rle, plain, {".shaf": b"@0", ".cod": b"@N@0@0"}, {".shaf": b"@1", ".cod": b"#R@1"},
            {k: rle[k] for k in (".rle", ".rle.freq")}, {".rle": b"", ".rle.freq": b"@R@0@0"},
            {".rle": b"xy", ".rle.freq": b"R@1"}]
    for name in ("cod bad char", "cod 257 fields", "cod empty size", "cod count too large", "cod 25-digit count",
                 "shaf 21-digit size", "shaf missing @", "shaf size past end", "shaf truncated", "shaf bad header",
                 "shaf other count", "freq empty text", "freq size past end", "rle truncated", "cod bad char, plain"):
        sets.append(corpus[name][0])
    out = []
    for s in sets:
        if ".rle.shaf" in s or ".shaf" in s:
            k = ".rle" if ".rle.shaf" in s else ""
            out.append(("sf", s[k + ".shaf"], s[k + ".cod"]))
        else:
            out.append(("rf", s[".rle"], s[".rle.freq"]))
    return out


def test_segmented_parse_equals_single_file_parse(shafa):
    import torch
    dev = _dev()
    tsz = C.sizeof(shafa.CodeTable)
    sets = _parity_sets(shafa)
    assert len(sets) >= 20
    for kind in ("sf", "rf"):
        fs = [s for s in sets if s[0] == kind]
        mbs = [shafa.unpack_max_blocks(len(s[2]), "cod" if kind == "sf" else "freq") for s in fs]
        first, pos = [], G
        for i, m in enumerate(mbs):
            pos += i % 3                                               # gaps between some files' slot ranges
            first.append(pos)
            pos += m
        ns = pos + G
        # the files back to back at odd offsets inside two allocations (payload files, texts)
        pays, texts = [s[1] for s in fs], [s[2] for s in fs]

        def pack(blobs, k):
            off, p = [], k
            for i, b in enumerate(blobs):
                off.append(p)
                p += len(b) + 1 + i % 5
            t = torch.zeros(p + 64, dtype=torch.uint8, device=dev)
            for o, b in zip(off, blobs):
                if b:
                    t[o:o + len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
            return t, off
        d_pay, poff = pack(pays, 5)
        d_txt, toff = pack(texts, 9)
        st = torch.cuda.Stream(device=dev)
        bt = shafa.Batch(ns, 1 << 20)
        try:
            nf = len(fs)
            info = torch.full((8 * (nf + 2),), SENT, dtype=torch.int64, device=dev)
            arrs = [torch.full((ns,), SENT, dtype=torch.int64, device=dev) for _ in range(3)]
            tab = torch.full((ns * tsz,), 0xA5, dtype=torch.uint8, device=dev)
            pb, tb = d_pay.data_ptr(), d_txt.data_ptr()
            if kind == "sf":
                bt.unpack_cod_files(st, first, mbs, tb, toff, [len(t) for t in texts], info[8:], arrs[0], tab)
                bt.unpack_shaf_files(st, first, mbs, pb, poff, [len(p) for p in pays], info[8 + 3:], arrs[1], arrs[2])
            else:
                bt.unpack_rle_freq_files(st, first, mbs, tb, toff, [len(t) for t in texts], poff, [len(p) for p in pays],
                                         info[8:], arrs[1], arrs[2])
            _, errs = bt.finish(st, ns, raise_on_error=False)
            iv = _u64(info)
            av = [_u64(a) for a in arrs]
            tv = _bytes(tab)
            owned = np.zeros(ns, dtype=bool)
            for f, (m, s0) in enumerate(zip(mbs, first)):
                owned[s0:s0 + m] = True
                one = shafa.Batch(m, 1 << 20)
                try:
                    i1 = torch.zeros(8, dtype=torch.int64, device=dev)
                    a1 = [torch.zeros(m, dtype=torch.int64, device=dev) for _ in range(3)]
                    t1 = torch.zeros(m * tsz, dtype=torch.uint8, device=dev)
                    dp, dt = _t(pays[f], 3), _t(texts[f], 7)
                    if kind == "sf":
                        one.unpack_cod(st, m, dt, i1, a1[0], t1)
                        one.unpack_shaf(st, m, dp, i1[3:4], a1[1], a1[2])
                    else:
                        one.unpack_rle_freq(st, m, dt, len(pays[f]), i1, a1[1], a1[2])
                    _, e1 = one.finish(st, m, raise_on_error=False)
                finally:
                    one.close()
                info1 = _u64(i1)
                what = f"{kind} file {f}"
                assert iv[8 * (f + 1):8 * (f + 1) + 6] == info1[:6], what
                assert iv[8 * (f + 1) + 6:8 * (f + 2)] == [0xA5A5A5A5A5A5A5A5] * 2, what
                assert errs[s0:s0 + m] == e1[:m], what
                o1, n1 = _u64(a1[1]), _u64(a1[2])
                assert av[2][s0:s0 + m] == n1, what
                framed = info1[4]
                for b in range(m):                                     # framed blocks' offsets from the call's base
                    valid = (o1[b] != 0) if kind == "sf" else b < framed
                    assert av[1][s0 + b] == (o1[b] + poff[f] if valid else 0), (what, b)
                if kind == "sf":
                    assert av[0][s0:s0 + m] == _u64(a1[0]), what
                    assert tv[s0 * tsz:(s0 + m) * tsz] == _bytes(t1), what
            assert iv[:8] == [0xA5A5A5A5A5A5A5A5] * 8 and iv[8 * (nf + 1):] == [0xA5A5A5A5A5A5A5A5] * 8
            for s in np.nonzero(~owned)[0]:
                assert errs[s] == 0, s
                assert av[1][s] == av[2][s] == 0xA5A5A5A5A5A5A5A5 and (kind == "rf" or av[0][s] == 0xA5A5A5A5A5A5A5A5), s
                assert tv[s * tsz:(s + 1) * tsz] == b"\xa5" * tsz, s
        finally:
            bt.close()


# ---------------------------------------------------------------- 2. golden sessions, one call
def test_golden_sessions_in_one_call(shafa):
    import torch
    entries, want, sessions = [], [], []
    try:
        for case in DECODED:
            man = _man(case)
            argv = man["cmds"][0]["argv"]
            fn = argv[0]
            data, S = _case_input(shafa, case, man, fn)
            if S is not None:
                sessions.append(S)
            c = _opt(argv, "-c")
            files = shafa.compress_files(torch.from_numpy(data).to(_dev()), BLOCK.get(_opt(argv, "-b"), 65536),
                                         force_rle=c == "r", force_freq=c == "f")
            del data
            rcs = _decode_rcs(man)
            for key, meta in man["files"].items():
                if not key.startswith("decoded__"):
                    continue
                kind = key[len("decoded__"):]
                if kind == "rle_only":
                    entries.append(dict(rle=files[".rle"], freq=files[".rle.freq"]))
                elif kind == "sf_rle":
                    entries.append(dict(shaf=files[".rle.shaf"], cod=files[".rle.cod"], decode_rle=True))
                else:
                    k = ".rle" if ".rle.shaf" in files else ""
                    entries.append(dict(shaf=files[k + ".shaf"], cod=files[k + ".cod"], decode_rle=False))
                want.append((case, key, rcs[key], meta))
        res = shafa.decompress_many(entries)
        assert len(res) == len(entries)
        for (case, key, rc, meta), r in zip(want, res):
            if rc != 0:                                                # test_gpu_unpack: the reference crashed there
                assert isinstance(r, shafa.ShafaError) and r.code == shafa.FILE_UNRECOGNIZABLE, (case, key, r)
                continue
            assert isinstance(r, torch.Tensor), (case, key, r)
            assert r.numel() == meta["size"] and _sha(_bytes(r)) == meta["sha256"], f"{case}/{key}"
    finally:
        for S in sessions:
            S.close()


# ---------------------------------------------------------------- 3. the fault corpus among intact files
def test_fault_corpus_among_intact_files(shafa):
    import os
    rle, plain = _session(shafa)
    cases = _corpus(rle, plain)
    bad = os.path.join(GOLD, "edge_bad_cod_mid")
    stored = {k: open(os.path.join(bad, "g" + k), "rb").read() for k in (".rle.cod", ".rle.shaf")}
    cases["edge_bad_cod_mid (stored)"] = (stored, True)
    intact = [(rle, True), (plain, False), ({k: rle[k] for k in (".rle", ".rle.freq")}, None), (rle, False)]
    sets = []
    for j, (name, c) in enumerate(cases.items()):
        sets.append((name, c))
        sets.append((f"intact {j}", intact[j % len(intact)]))
    entries, want = [], []
    for j, (name, (files, decode_rle)) in enumerate(sets):
        sf = ".shaf" in files or ".rle.shaf" in files
        d = bool(decode_rle) if sf else True
        entries.append(_entry(files, d, mis=j % 16))
        want.append(_dev_decode(shafa, files, decode_rle=d, mis=(j * 5) % 16))
    got = [_result(r) for r in shafa.decompress_many(entries)]
    seen = set()
    for (name, _), g, w in zip(sets, got, want):
        assert g == w, f"{name}: decompress_many {g[0]}, decompress_files {w[0]}"
        if name.startswith("intact"):
            assert g[0] == 0, name
        seen.add(w[0])
    assert {0, shafa.FILE_STREAM_FAILED, shafa.FILE_UNRECOGNIZABLE} <= seen, seen


# ---------------------------------------------------------------- 4. round trips through compress_many
def _many_inputs(n_files, seed):
    import golden.make_golden as mg
    zt = mg.zipf_table(1.2)
    rng = np.random.default_rng(seed)
    datas = []
    for i in range(n_files):
        n = int(rng.integers(1024, 24000))
        datas.append(mg.runs_stream(seed + i, n, zt) if i % 2 else mg.gen_bytes(seed + i, n))
    return datas


def test_round_trip_1000_files(shafa):
    import torch
    datas = _many_inputs(1000, 9100)
    d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
    sets = shafa.compress_many(d_in, [d.size for d in datas], 16384)
    assert all(isinstance(s, dict) for s in sets)
    n_rle = sum(".rle.shaf" in s for s in sets)
    assert 0 < n_rle < len(sets)
    ent = []
    for s in sets:
        k = ".rle" if ".rle.shaf" in s else ""
        ent.append(dict(shaf=s[k + ".shaf"], cod=s[k + ".cod"], decode_rle=bool(k)))
    for d, r in zip(datas, shafa.decompress_many(ent)):
        assert _bytes(r) == d.tobytes()
    rle_sets = [(d, s) for d, s in zip(datas, sets) if ".rle.shaf" in s]
    res = shafa.decompress_many([dict(shaf=s[".rle.shaf"], cod=s[".rle.cod"], decode_rle=False) for _, s in rle_sets])
    for (_, s), r in zip(rle_sets, res):
        assert torch.equal(r, s[".rle"])
    res = shafa.decompress_many([dict(rle=s[".rle"], freq=s[".rle.freq"]) for _, s in rle_sets])
    for (d, _), r in zip(rle_sets, res):
        assert _bytes(r) == d.tobytes()


# ---------------------------------------------------------------- 5. 33..64-bit codes in several files
def test_long_codes_in_several_files(oracle, shafa):
    from test_gpu_parity import long_code_case, to_shafa_table
    entries, want = [], []
    for f in range(4):
        blocks, texts, pays = [], [], []
        for b in range(3):
            otab, data = long_code_case(oracle, 20000 + 1000 * b + 7 * f, 60 - 3 * b, 0.5, 30 + 3 * f + b)
            tab = to_shafa_table(shafa, otab)
            assert max(bytes(tab.len)) > 32
            enc = shafa.sf_encode(data, tab)
            blocks.append(data)
            texts.append(_cod_text(shafa, tab))
            pays.append(enc.tobytes())
        cod = _cod_file(b"N", [d.size for d in blocks], texts)
        shaf = b"@3" + b"".join(b"@" + str(len(p)).encode() + b"@" + p for p in pays)
        entries.append(dict(shaf=_t(shaf, f), cod=_t(cod, 2 * f), decode_rle=False))
        want.append(np.concatenate(blocks).tobytes())
    for r, w in zip(shafa.decompress_many(entries), want):
        assert _bytes(r) == w


# ---------------------------------------------------------------- 6. groups
def test_more_blocks_than_a_group(shafa):
    import torch
    datas = _many_inputs(48, 9300)
    datas = [np.tile(d, 1 + 200000 // d.size)[:200000 + 37 * i] for i, d in enumerate(datas)]
    d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
    sets = shafa.compress_many(d_in, [d.size for d in datas], 512)
    nblocks = sum(int(_bytes(s[".rle.cod" if ".rle.cod" in s else ".cod"]).split(b"@")[2]) for s in sets)
    assert nblocks > shafa.MANY_GROUP_BLOCKS
    ent = []
    for s in sets:
        k = ".rle" if ".rle.shaf" in s else ""
        ent.append(dict(shaf=s[k + ".shaf"], cod=s[k + ".cod"], decode_rle=bool(k)))
    for d, r in zip(datas, shafa.decompress_many(ent, max_bytes=8 << 20)):      # RLE decoding in several groups
        assert _bytes(r) == d.tobytes()


# ---------------------------------------------------------------- 7. synchronisations
def test_synchronisations_do_not_grow_with_files(shafa, monkeypatch):
    import torch
    datas = _many_inputs(200, 9500)
    d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
    sets = shafa.compress_many(d_in, [d.size for d in datas], 16384, force_rle=True)
    calls = []
    real = shafa.Batch.finish

    def counting(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(shafa.Batch, "finish", counting)
    res = shafa.decompress_many([dict(shaf=s[".rle.shaf"], cod=s[".rle.cod"], decode_rle=False) for s in sets])
    assert len(calls) <= 2, len(calls)
    assert all(torch.equal(r, s[".rle"]) for r, s in zip(res, sets))
    calls.clear()
    res = shafa.decompress_many([dict(shaf=s[".rle.shaf"], cod=s[".rle.cod"], decode_rle=True) for s in sets])
    assert len(calls) <= 4, len(calls)                                 # the docstring's count for one RLE group
    assert all(_bytes(r) == d.tobytes() for r, d in zip(res, datas))
    calls.clear()
    res = shafa.decompress_many([dict(rle=s[".rle"], freq=s[".rle.freq"]) for s in sets])
    assert len(calls) <= 3, len(calls)
    assert all(_bytes(r) == d.tobytes() for r, d in zip(res, datas))


# ---------------------------------------------------------------- 8. enqueue only
def test_no_synchronisation_inside_the_segmented_parses(shafa):
    import torch
    rle, plain = _session(shafa)
    dev = _dev()
    sf_sets = [rle, plain, rle]
    shafs = [s[".rle.shaf"] if ".rle.shaf" in s else s[".shaf"] for s in sf_sets]
    cods = [s[".rle.cod"] if ".rle.cod" in s else s[".cod"] for s in sf_sets]
    mbs = [shafa.unpack_max_blocks(len(c), "cod") for c in cods]
    first = [sum(mbs[:i]) for i in range(3)]
    ns = sum(mbs)
    d_shaf = [_t(b, i) for i, b in enumerate(shafs)]
    d_cod = [_t(b, 4 + i) for i, b in enumerate(cods)]
    d_rle, d_freq = _t(rle[".rle"], 1), _t(rle[".rle.freq"], 2)
    lo = min(t.data_ptr() for t in d_shaf + [d_rle])
    clo = min(t.data_ptr() for t in d_cod + [d_freq])
    tsz = C.sizeof(shafa.CodeTable)
    fmb = shafa.unpack_max_blocks(len(rle[".rle.freq"]), "freq")
    info = torch.zeros(8 * 4, dtype=torch.int64, device=dev)
    nsym, off, n = (torch.zeros(ns + fmb, dtype=torch.int64, device=dev) for _ in range(3))
    tab = torch.zeros(ns * tsz, dtype=torch.uint8, device=dev)
    bt = shafa.Batch(ns + fmb, 1 << 20)
    st = torch.cuda.Stream(device=dev)

    def enqueue():
        bt.unpack_cod_files(st, first, mbs, clo, [t.data_ptr() - clo for t in d_cod], [t.numel() for t in d_cod], info,
                            nsym, tab)
        bt.unpack_shaf_files(st, first, mbs, lo, [t.data_ptr() - lo for t in d_shaf], [t.numel() for t in d_shaf],
                             info[3:], off, n)
        bt.unpack_rle_freq_files(st, [ns], [fmb], clo, [d_freq.data_ptr() - clo], [d_freq.numel()],
                                 [d_rle.data_ptr() - lo], [d_rle.numel()], info[24:], off, n)

    try:
        enqueue()                                                      # warm-up: the batch grows here
        bt.finish(st, ns + fmb)
        want = _u64(info), _u64(n)
        info.zero_()
        n.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)
        enqueue()
        busy = not st.query()
        bt.finish(st, ns + fmb)
        assert busy, "the stream had drained when the calls returned: something synchronised"
        assert (_u64(info), _u64(n)) == want
    finally:
        bt.close()

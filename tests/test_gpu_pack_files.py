"""Many files per call: the segmented packs (shafa_hipd_pack_payloads_files / _pack_cod_files / _pack_freq_files,
csrc/pack.hip) and shafa.compress_many, which chains F -> T -> C -> those packs once for a whole batch of files.

1. compress_many reproduces every golden session whose first command runs Module F, one call per block size and -c flag;
2. on a mixed corpus (edge sizes, RLE and plain content, a file under 1 KiB, files at odd offsets) every file equals
   compress_files on that file alone, under each flag setting, and decodes back to its input; both run one chain, so
   every file the reference binary writes for that file alone is compared with compress_files' as well;
2a. compress_files on a tensor at an odd address (the gather into aligned regions) equals the aligned copy's files, and a
   block size that is no multiple of 16 round-trips at either alignment; a block's error raises the code compress_many's
   entry carries, the size pass's first, then the first in block order;
3. its files decode with our CLI and with the reference binary;
4. each file of a segmented pack equals the host's framing / formatter of its blocks (random partitions, overlaps, gaps,
   per-file modes, 0-byte payloads, all-empty tables);
5. a refused file (too long for its region, or a size past its capacity) writes nothing; the other files are exact;
6. the calls only enqueue;
7. one pack over more than 65 536 blocks (the bulk grid in slices) is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_pack import (BLOCK, F_CASES, F_KEYS, ALL_KEYS, FILL, GOLD, _case_input, _cod_text, _decode_with, _dev,
                           _manifest, _opt, _payload_file, _random_counts, _random_table, _sha, _tables_dev, _text_file,
                           _u64_dev)

pytestmark = pytest.mark.gpu

GUARD = 64


def _groups():
    g = {}
    for case in F_CASES:
        argv = _manifest(case)["cmds"][0]["argv"]
        g.setdefault((_opt(argv, "-b"), _opt(argv, "-c")), []).append(case)
    return sorted(g.items(), key=lambda kv: (str(kv[0][0]), str(kv[0][1])))


GROUPS = _groups()


@pytest.mark.parametrize("key,cases", GROUPS, ids=[f"b{k[0]}-c{k[1]}" for k, _ in GROUPS])
def test_compress_many_reproduces_reference_files(shafa, key, cases):
    import torch
    b, c = key
    datas, sessions = [], []
    try:
        for case in cases:
            man = _manifest(case)
            fn = man["cmds"][0]["argv"][0]
            data, S = _case_input(shafa, case, man, fn)
            if S is not None:
                sessions.append(S)
            assert _sha(data.tobytes()) == man["files"][fn]["sha256"]
            datas.append(data)
        d_in = torch.from_numpy(np.concatenate(datas)).to(_dev())
        res = shafa.compress_many(d_in, [d.size for d in datas], BLOCK.get(b, 65536), force_rle=c == "r", force_freq=c == "f")
        assert len(res) == len(cases)
        for case, files in zip(cases, res):
            assert isinstance(files, dict), (case, files)
            man = _manifest(case)
            argv = man["cmds"][0]["argv"]
            fn = argv[0]
            keys = F_KEYS if _opt(argv, "-m") == "f" else ALL_KEYS
            want = {k for k in keys if fn + k in man["files"]}
            got = {k for k in files if k in keys}
            assert got == want, f"{case}: files {sorted(got)} != the reference's {sorted(want)}"
            for k in sorted(got):
                meta = man["files"][fn + k]
                bts = files[k].cpu().numpy().tobytes()
                stored = os.path.join(GOLD, case, fn + k)
                if os.path.exists(stored):
                    with open(stored, "rb") as f:
                        assert bts == f.read(), f"{case}/{fn + k} differs from the stored file"
                assert len(bts) == meta["size"] and _sha(bts) == meta["sha256"], f"{case}/{fn + k} differs from the reference's"
    finally:
        for S in sessions:
            S.close()


# ---------------------------------------------------------------- a mixed corpus
K = 655360


def _corpus():
    """(sizes, contents) of the mixed corpus: edge sizes at -b K, Zipf / runs (takes RLE) / uniform (does not) content"""
    import golden.make_golden as mg
    zt = mg.zipf_table(1.2)
    sizes = [1024, 1025, 4097, K - 1, K, K + 1023, 3 * K + 17, 1000, 70000, 2048]
    kinds = ["zipf", "runs", "uniform", "runs", "zipf", "uniform", "runs", "zipf", "zipf", "runs"]
    out = []
    for i, (n, k) in enumerate(zip(sizes, kinds)):
        seed = 500 + i
        if k == "runs":
            out.append(mg.runs_stream(seed, n, zt))
        elif k == "uniform":
            out.append(mg.gen_bytes(seed, n))
        else:
            out.append(zt[mg.gen_bytes(seed, 2 * n).view(np.uint16)[:n]] if n else np.zeros(0, np.uint8))
    return sizes, [np.ascontiguousarray(d, dtype=np.uint8) for d in out]


def _packed_at_odd_offsets(datas):
    """the files back to back in one device tensor whose first byte lies 3 bytes past a 16-byte boundary (so the files start
    at odd and unaligned offsets)"""
    import torch
    host = np.concatenate(datas)
    base = torch.zeros(host.size + 64, dtype=torch.uint8, device=_dev())
    k = (-base.data_ptr()) % 16 + 3                                     # 16k + 3
    d_in = base[k:k + host.size]
    d_in.copy_(torch.from_numpy(host).to(_dev()))
    return d_in


def _same_files(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (what, k)


def _spelled(flag, value):
    """[flag, value] as a golden session's command line spells it"""
    for case in F_CASES:
        argv = _manifest(case)["cmds"][0]["argv"]
        if _opt(argv, flag) == value:
            return argv[argv.index(flag):argv.index(flag) + 2]
    raise AssertionError(f"no golden session runs {flag} {value}")


def _reference_files(work, data, args):
    """the files the reference binary writes for `data` as the file "f" in `work`, run with `args`: {".rle": bytes, ...}"""
    import oracle_lib
    for name in os.listdir(work):
        os.remove(os.path.join(work, name))
    data.tofile(os.path.join(work, "f"))
    r = subprocess.run([oracle_lib.REF_BIN, "f"] + args, cwd=work, capture_output=True, timeout=300)
    assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
    out = {}
    for name in sorted(os.listdir(work)):
        if name != "f":
            assert name.startswith("f."), name
            with open(os.path.join(work, name), "rb") as f:
                out[name[1:]] = f.read()
    return out


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)], ids=["default", "c_r", "c_f"])
def test_compress_many_equals_compress_files_per_file(shafa, flags, tmp_path):
    import oracle_lib
    import torch
    force_rle, force_freq = flags
    sizes, datas = _corpus()
    d_in = _packed_at_odd_offsets(datas)
    res = shafa.compress_many(d_in, sizes, K, force_rle=force_rle, force_freq=force_freq)
    assert len(res) == len(sizes)
    modes, wants = set(), {}
    for i, (n, data) in enumerate(zip(sizes, datas)):
        one = torch.from_numpy(data).to(_dev())
        if n < 1024:
            assert isinstance(res[i], shafa.ShafaError) and res[i].code == shafa.FILE_TOO_SMALL, res[i]
            continue
        want = wants[i] = shafa.compress_files(one, K, force_rle=force_rle, force_freq=force_freq)
        assert isinstance(res[i], dict), (i, res[i])
        _same_files(res[i], want, f"file {i} ({n} bytes)")
        modes.add(".rle.cod" in want)
    if not force_rle:
        assert modes == {True, False}, "the corpus should hold RLE and plain files"
    # the two drivers run one chain: the anchor outside it is the reference binary on each file alone
    if not os.path.exists(oracle_lib.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref/shafa)")
    args = _spelled("-b", "K") + (_spelled("-c", "r") if force_rle else _spelled("-c", "f") if force_freq else [])
    assert len(wants) == 9
    for i, want in wants.items():
        ref = _reference_files(str(tmp_path), datas[i], args)
        assert sorted(ref) == sorted(want), (i, sorted(ref), sorted(want))
        for k in ref:
            assert want[k].cpu().numpy().tobytes() == ref[k], f"file {i} ({sizes[i]} bytes): {k} differs from the reference's"


# ---------------------------------------------------------------- compress_files: alignment, block sizes, errors
@pytest.mark.parametrize("i", [6, 5], ids=["runs_3K+17", "uniform_K+1023"])
def test_compress_files_at_an_odd_address_equals_the_aligned_copy(shafa, i):
    import torch
    sizes, datas = _corpus()
    assert sizes[i] == (3 * K + 17, K + 1023)[i == 5]
    aligned = torch.from_numpy(datas[i]).to(_dev())
    odd = _packed_at_odd_offsets([datas[i]])
    assert aligned.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 3 and torch.equal(odd, aligned)
    want = shafa.compress_files(aligned, K)
    assert (".rle.shaf" in want) == (i == 6), sorted(want)
    _same_files(shafa.compress_files(odd, K), want, f"file {i} at an odd address")


def test_compress_files_block_size_no_multiple_of_16_round_trips(shafa):
    import torch
    import golden.make_golden as mg
    n, bs = 200_000, 65537
    data = np.ascontiguousarray(mg.zipf_table(1.2)[mg.gen_bytes(77, 2 * n).view(np.uint16)[:n]], dtype=np.uint8)
    aligned = torch.from_numpy(data).to(_dev())
    odd = _packed_at_odd_offsets([data])
    assert aligned.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 3
    got = []
    for what, d_in in (("aligned", aligned), ("odd", odd)):
        files = shafa.compress_files(d_in, bs)
        if ".rle.shaf" in files:
            back = shafa.decompress_files(shaf=files[".rle.shaf"], cod=files[".rle.cod"])
        else:
            back = shafa.decompress_files(shaf=files[".shaf"], cod=files[".cod"], decode_rle=False)
        assert back.cpu().numpy().tobytes() == data.tobytes(), what
        stem = ".rle" if ".rle.shaf" in files else ""
        assert files[stem + ".shaf"].cpu().numpy().tobytes().startswith(b"@4@"), what      # 3 x 65 537 bytes and 3 389
        got.append(files)
    _same_files(got[1], got[0], "odd against aligned")


ERROR_CASES = {       # {finish call: {block: the code it reports}} -> the file's code
    "size_pass": ({1: {1: 2}}, 2),
    "packs": ({2: {1: 5}}, 5),
    "size_pass_before_packs": ({1: {2: 1}, 2: {0: 2}}, 1),
    "first_in_block_order": ({2: {2: 2, 1: 4}}, 4),
}


@pytest.mark.parametrize("name", list(ERROR_CASES))
def test_compress_files_raises_the_code_compress_many_carries(shafa, monkeypatch, name):
    """No input reaches a block error in the compress chain by itself (the size pass and the packs cannot fail on sizes the
    driver computed, and the encoder's region holds 12 bits a symbol), so Batch.finish reports chosen codes for chosen
    blocks of a three-block file."""
    import torch
    import golden.make_golden as mg
    inject, code = ERROR_CASES[name]
    assert (shafa.OUTSIDE_MODULE, shafa.LACK_OF_MEMORY, shafa.FILE_UNRECOGNIZABLE, shafa.FILE_STREAM_FAILED) == (1, 2, 4, 5)
    d_in = torch.from_numpy(mg.runs_stream(41, 65536 * 2 + 7777, mg.zipf_table(1.2))).to(_dev())
    real = shafa.Batch.finish
    calls = []

    def finish(self, stream, nblocks, raise_on_error=True):
        rc, errs = real(self, stream, nblocks, raise_on_error=False)
        calls.append(nblocks)
        assert rc == 0 and nblocks == 3
        for b, e in inject.get(len(calls), {}).items():
            errs[b] = e
        rc = next((e for e in errs if e), 0)
        if raise_on_error and rc:
            raise shafa.ShafaError(rc, "finish")
        return rc, errs

    monkeypatch.setattr(shafa.Batch, "finish", finish)
    many = shafa.compress_many(d_in, [d_in.numel()], 65536)[0]
    assert len(calls) == 2
    assert isinstance(many, shafa.ShafaError) and many.code == code, many
    calls.clear()
    with pytest.raises(shafa.ShafaError) as e:
        shafa.compress_files(d_in, 65536)
    assert e.value.code == many.code


def test_compress_many_takes_a_list_and_round_trips(shafa):
    import torch
    sizes, datas = _corpus()
    tensors = [torch.from_numpy(d).to(_dev()) for d in datas]
    res = shafa.compress_many(tensors, block_size=K)
    for i, (files, data) in enumerate(zip(res, datas)):
        if data.size < 1024:
            assert isinstance(files, shafa.ShafaError)
            continue
        if ".rle.shaf" in files:
            back = shafa.decompress_files(shaf=files[".rle.shaf"], cod=files[".rle.cod"])
            assert back.cpu().numpy().tobytes() == data.tobytes(), f"file {i}: .rle.shaf / .rle.cod"
            back = shafa.decompress_files(rle=files[".rle"], freq=files[".rle.freq"])
        else:
            back = shafa.decompress_files(shaf=files[".shaf"], cod=files[".cod"], decode_rle=False)
        assert back.cpu().numpy().tobytes() == data.tobytes(), f"file {i} does not decode back"


def _two_small(shafa, tmp_path):
    """one RLE and one plain file of compress_many written to tmp_path: [(name, input bytes)]"""
    import torch
    import golden.make_golden as mg
    runs = mg.runs_stream(41, 65536 * 2 + 777, mg.zipf_table(1.2))
    plain = mg.gen_bytes(4001, 65536 + 12345)
    res = shafa.compress_many(torch.from_numpy(np.concatenate([runs, plain])).to(_dev()), [runs.size, plain.size], 65536)
    out = []
    for name, files, data in (("r", res[0], runs), ("p", res[1], plain)):
        stem = ".rle" if name == "r" else ""
        assert (stem + ".shaf") in files, sorted(files)
        for k in (stem + ".cod", stem + ".shaf"):
            files[k].cpu().numpy().tofile(str(tmp_path / (name + k)))
        out.append((name + stem + ".shaf", data.tobytes()))
    return out


def test_compress_many_files_decode_with_our_cli(shafa, tmp_path):
    for name, want in _two_small(shafa, tmp_path):
        _decode_with(shafa.CLI_PATH, str(tmp_path), name, want)


def test_compress_many_files_decode_with_reference_binary(shafa, tmp_path):
    import oracle_lib
    if not os.path.exists(oracle_lib.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref/shafa)")
    for name, want in _two_small(shafa, tmp_path):
        _decode_with(oracle_lib.REF_BIN, str(tmp_path), name, want)


# ---------------------------------------------------------------- the segmented packs against the host's framing
class Regions:
    """one device buffer of per-file regions at misalignments 0..15, each followed by GUARD guard bytes"""

    def __init__(self, caps, rng):
        import torch
        self.off, pos = [], 0
        for c in caps:
            pos += int(rng.integers(0, 16))
            self.off.append(pos)
            pos += c + GUARD
        self.caps = list(caps)
        self.t = torch.full((pos + 16,), FILL, dtype=torch.uint8, device=_dev())
        self.n = torch.zeros(len(caps), dtype=torch.int64, device=_dev())

    def check(self, f, want):
        got = self.t[self.off[f]:self.off[f] + self.caps[f] + GUARD].cpu().numpy().tobytes()
        n = int(self.n[f].item())
        assert n == len(want), (f, n, len(want))
        assert got[:n] == want, f"file {f} differs from the host's"
        assert got[n:] == bytes([FILL]) * (len(got) - n), f"file {f}: bytes written past its length"

    def untouched(self, f):
        got = self.t[self.off[f]:self.off[f] + self.caps[f] + GUARD].cpu().numpy()
        assert (got == FILL).all(), f"file {f}: bytes written to a refused file's region"


def _partition(rng, nb, nf):
    """nf files over blocks [0, nb): ranges that tile, skip, overlap and repeat"""
    first, count = [], []
    for f in range(nf):
        r = rng.random()
        if r < 0.15 and first:                                             # the same range as an earlier file
            j = int(rng.integers(len(first)))
            first.append(first[j])
            count.append(count[j])
            continue
        a = int(rng.integers(0, nb))
        first.append(a)
        count.append(int(rng.integers(1, min(nb - a, 40) + 1)))
    return first, count


def _payload_blocks(rng, nb):
    sizes = [0 if rng.random() < 0.15 else int(rng.integers(1, 5000)) if rng.random() < 0.9 else int(rng.integers(1, 200000))
             for _ in range(nb)]
    caps = [s + int(rng.integers(0, 40)) for s in sizes]
    off, pos = [], 0
    for c in caps:
        off.append(pos)
        pos += (c + 15) // 16 * 16 + 16 * int(rng.integers(0, 2))
    src = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    return sizes, caps, off, src


@pytest.mark.parametrize("nb,nf,seed", [(1, 1, 1), (5, 3, 2), (40, 17, 3), (300, 64, 4)])
def test_pack_files_equal_host_framing(shafa, nb, nf, seed):
    import torch
    rng = np.random.default_rng(900 + seed)
    first, count = _partition(rng, nb, nf)
    sizes, caps, off, src = _payload_blocks(rng, nb)
    d_src, d_n = torch.from_numpy(src).to(_dev()), _u64_dev(sizes)
    blocks = [src[o:o + n].tobytes() for o, n in zip(off, sizes)]
    kinds_t, kinds_f = ["random", "long", "empty", "sparse"], ["random", "zero", "max", "runs"]
    tables = [_random_table(shafa, rng, "empty" if b % 5 == 0 else kinds_t[b % 4]) for b in range(nb)]
    counts = np.stack([_random_counts(rng, kinds_f[b % 4]) for b in range(nb)])
    hdr = [int(rng.integers(0, 2 ** 63)) if b % 3 else b for b in range(nb)]
    d_hdr, d_tab, d_freq = _u64_dev(hdr), _tables_dev(tables), _u64_dev(counts.reshape(-1))
    modes = [b"R" if rng.random() < 0.5 else b"N" for _ in range(nf)]
    cod_txt = [_cod_text(shafa, t) for t in tables]
    freq_txt = [shafa.freq_format(c) for c in counts]
    rng_of = [range(a, a + c) for a, c in zip(first, count)]
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        for framing in (shafa.FRAME_RAW, shafa.FRAME_SHAF):
            r = Regions([shafa.pack_payloads_max([caps[b] for b in rb], framing) for rb in rng_of], rng)
            torch.cuda.synchronize()
            bt.pack_payloads_files(st, first, count, framing, d_src, off, caps, d_n, r.t, r.off, r.caps, r.n)
            bt.finish(st, nb)
            for f, rb in enumerate(rng_of):
                r.check(f, _payload_file(framing, [blocks[b] for b in rb], shafa))
        r = Regions([shafa.pack_cod_max(c) for c in count], rng)
        torch.cuda.synchronize()
        bt.pack_cod_files(st, first, count, modes, d_hdr, d_tab, r.t, r.off, r.caps, r.n)
        bt.finish(st, nb)
        for f, rb in enumerate(rng_of):
            r.check(f, _text_file(modes[f], [hdr[b] for b in rb], [cod_txt[b] for b in rb]))
        r = Regions([shafa.pack_freq_max(c) for c in count], rng)
        torch.cuda.synchronize()
        bt.pack_freq_files(st, first, count, modes, d_hdr, d_freq, r.t, r.off, r.caps, r.n)
        bt.finish(st, nb)
        for f, rb in enumerate(rng_of):
            r.check(f, _text_file(modes[f], [hdr[b] for b in rb], [freq_txt[b] for b in rb]))
    finally:
        bt.close()


def test_pack_files_equal_single_file_packs(shafa):
    """the segmented packs and the single-file packs agree byte for byte on the same blocks"""
    import torch
    rng = np.random.default_rng(77)
    nb = 12
    first, count = [0, 3, 7, 2], [3, 4, 5, 9]
    sizes, caps, off, src = _payload_blocks(rng, nb)
    d_src, d_n = torch.from_numpy(src).to(_dev()), _u64_dev(sizes)
    tables = [_random_table(shafa, rng, "sparse") for _ in range(nb)]
    d_tab = _tables_dev(tables)
    tsz = C.sizeof(shafa.CodeTable)
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        r = Regions([shafa.pack_payloads_max(caps[a:a + c], shafa.FRAME_SHAF) for a, c in zip(first, count)], rng)
        bt.pack_payloads_files(st, first, count, shafa.FRAME_SHAF, d_src, off, caps, d_n, r.t, r.off, r.caps, r.n)
        q = Regions([shafa.pack_cod_max(c) for c in count], rng)
        bt.pack_cod_files(st, first, count, b"NRNR", d_n, d_tab, q.t, q.off, q.caps, q.n)
        bt.finish(st, nb)
        for f, (a, c) in enumerate(zip(first, count)):
            one = torch.zeros(r.caps[f], dtype=torch.uint8, device=_dev())
            n = torch.zeros(1, dtype=torch.int64, device=_dev())
            bt.pack_payloads(st, shafa.FRAME_SHAF, d_src, off[a:a + c], caps[a:a + c], d_n[a:a + c], one, one.numel(), n)
            bt.finish(st, nb)
            r.check(f, one[:int(n.item())].cpu().numpy().tobytes())
            one = torch.zeros(q.caps[f], dtype=torch.uint8, device=_dev())
            bt.pack_cod(st, c, b"NRNR"[f:f + 1], d_n[a:a + c], d_tab[a * tsz:(a + c) * tsz], one, one.numel(), n)
            bt.finish(st, nb)
            q.check(f, one[:int(n.item())].cpu().numpy().tobytes())
    finally:
        bt.close()


# ---------------------------------------------------------------- refusal per file
def test_refused_files_write_nothing_and_the_others_are_exact(shafa):
    import torch
    rng = np.random.default_rng(31)
    nb = 9
    first, count = [0, 2, 5, 7], [2, 3, 2, 2]
    sizes, caps, off, src = _payload_blocks(rng, nb)
    sizes[3] = max(sizes[3], 5)
    blocks = [src[o:o + n].tobytes() for o, n in zip(off, sizes)]
    d_src, d_n = torch.from_numpy(src).to(_dev()), _u64_dev(sizes)
    counts = np.stack([_random_counts(rng, "random") for _ in range(nb)])
    d_freq = _u64_dev(counts.reshape(-1))
    ftxt = [shafa.freq_format(c) for c in counts]
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    rngs = [range(a, a + c) for a, c in zip(first, count)]
    try:
        for framing in (shafa.FRAME_RAW, shafa.FRAME_SHAF):
            want = [_payload_file(framing, [blocks[b] for b in rb], shafa) for rb in rngs]
            # file 1 one byte short of its length
            caps_f = [len(w) + 8 for w in want]
            caps_f[1] = len(want[1]) - 1
            r = Regions(caps_f, rng)
            torch.cuda.synchronize()
            bt.pack_payloads_files(st, first, count, framing, d_src, off, caps, d_n, r.t, r.off, r.caps, r.n)
            rc, errs = bt.finish(st, nb, raise_on_error=False)
            assert rc == shafa.LACK_OF_MEMORY and errs == [0, 0, shafa.LACK_OF_MEMORY] + [0] * 6, (framing, errs)
            assert int(r.n[1].item()) == len(want[1])
            r.untouched(1)
            for f in (0, 2, 3):
                r.check(f, want[f])
            # block 3 (file 1) with a size past its capacity
            bad = list(sizes)
            bad[3] = caps[3] + 1
            r = Regions([len(w) + 64 for w in want], rng)
            torch.cuda.synchronize()
            bt.pack_payloads_files(st, first, count, framing, d_src, off, caps, _u64_dev(bad), r.t, r.off, r.caps, r.n)
            rc, errs = bt.finish(st, nb, raise_on_error=False)
            assert rc == shafa.OUTSIDE_MODULE and errs == [0, 0, 0, shafa.OUTSIDE_MODULE] + [0] * 5, (framing, errs)
            assert int(r.n[1].item()) == 0
            r.untouched(1)
            for f in (0, 2, 3):
                r.check(f, want[f])
        want = [_text_file(b"N", [sizes[b] for b in rb], [ftxt[b] for b in rb]) for rb in rngs]
        caps_f = [len(w) for w in want]
        caps_f[2] -= 1
        r = Regions(caps_f, rng)
        torch.cuda.synchronize()
        bt.pack_freq_files(st, first, count, b"NNNN", d_n, d_freq, r.t, r.off, r.caps, r.n)
        rc, errs = bt.finish(st, nb, raise_on_error=False)
        assert rc == shafa.LACK_OF_MEMORY and errs == [0] * 5 + [shafa.LACK_OF_MEMORY] + [0] * 3, errs
        assert int(r.n[2].item()) == len(want[2])
        r.untouched(2)
        for f in (0, 1, 3):
            r.check(f, want[f])
    finally:
        bt.close()


def test_block_range_past_the_batch_is_refused(shafa):
    import torch
    bt = shafa.Batch(4, 1 << 16)
    d = torch.zeros(4096, dtype=torch.uint8, device=_dev())
    n = torch.zeros(4, dtype=torch.int64, device=_dev())
    try:
        with pytest.raises(shafa.ShafaError) as e:
            bt.pack_payloads_files(None, [0, 2], [2, 3], shafa.FRAME_RAW, d, [0] * 5, [16] * 5, n, d, [0, 100], [100, 100], n)
        assert e.value.code == shafa.OUTSIDE_MODULE
        with pytest.raises(shafa.ShafaError) as e:
            bt.pack_cod_files(None, [4], [1], b"R", n, d, d, [0], [4096], n)
        assert e.value.code == shafa.OUTSIDE_MODULE
    finally:
        bt.close()


# ---------------------------------------------------------------- enqueue only
def test_no_synchronisation_inside_the_segmented_calls(shafa):
    import torch
    rng = np.random.default_rng(41)
    nb = 20
    first, count = [0, 4, 9, 15], [4, 5, 6, 5]
    sizes, caps, off, src = _payload_blocks(rng, nb)
    d_src, d_n = torch.from_numpy(src).to(_dev()), _u64_dev(sizes)
    blocks = [src[o:o + n].tobytes() for o, n in zip(off, sizes)]
    tables = [_random_table(shafa, rng, "random") for _ in range(nb)]
    counts = np.stack([_random_counts(rng, "runs") for _ in range(nb)])
    d_tab, d_freq = _tables_dev(tables), _u64_dev(counts.reshape(-1))
    rngs = [range(a, a + c) for a, c in zip(first, count)]
    shaf = Regions([shafa.pack_payloads_max([caps[b] for b in rb], shafa.FRAME_SHAF) for rb in rngs], rng)
    cod = Regions([shafa.pack_cod_max(c) for c in count], rng)
    freq = Regions([shafa.pack_freq_max(c) for c in count], rng)
    st = torch.cuda.Stream(device=_dev())
    bt = shafa.Batch(nb, 1 << 20)

    def enqueue():
        bt.pack_payloads_files(st, first, count, shafa.FRAME_SHAF, d_src, off, caps, d_n, shaf.t, shaf.off, shaf.caps, shaf.n)
        bt.pack_cod_files(st, first, count, b"RNRN", d_n, d_tab, cod.t, cod.off, cod.caps, cod.n)
        bt.pack_freq_files(st, first, count, b"NRNR", d_n, d_freq, freq.t, freq.off, freq.caps, freq.n)

    try:
        enqueue()                                                          # warm-up: the batch grows here
        bt.finish(st, nb)
        for r in (shaf, cod, freq):
            r.t.fill_(FILL)
            r.n.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)                                 # ~0.1 s of one busy wave
        enqueue()
        busy = not st.query()
        bt.finish(st, nb)
        assert busy, "the stream had drained when the calls returned: something synchronised"
        for f, rb in enumerate(rngs):
            shaf.check(f, _payload_file(shafa.FRAME_SHAF, [blocks[b] for b in rb], shafa))
            cod.check(f, _text_file(b"RNRN"[f:f + 1], [sizes[b] for b in rb], [_cod_text(shafa, tables[b]) for b in rb]))
            freq.check(f, _text_file(b"NRNR"[f:f + 1], [sizes[b] for b in rb], [shafa.freq_format(counts[b]) for b in rb]))
    finally:
        bt.close()


# ---------------------------------------------------------------- scale: the bulk grid in slices
def test_pack_payloads_files_over_100k_blocks(shafa):
    import torch
    rng = np.random.default_rng(51)
    nb = 100_003
    sizes = rng.integers(0, 64, nb)
    sizes[rng.integers(0, nb, 50)] = rng.integers(64, 3000, 50)
    caps = sizes + 16
    off = np.zeros(nb, dtype=np.int64)
    off[1:] = np.cumsum((caps + 15) // 16 * 16)[:-1]
    src = rng.integers(0, 256, int(off[-1] + caps[-1] + 64), dtype=np.uint8)
    counts = []
    left = nb
    while left:
        c = min(left, int(rng.integers(1, 70)))
        counts.append(c)
        left -= c
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    nf = len(counts)
    dcap = [int(sum(sizes[a:a + c])) + 1 + len(str(c)) + sum(2 + len(str(int(s))) for s in sizes[a:a + c])
            for a, c in zip(first, counts)]
    doff = np.concatenate([[0], np.cumsum(dcap)[:-1]]).tolist()
    d_src = torch.from_numpy(src).to(_dev())
    d_n = _u64_dev(sizes)
    d_dst = torch.full((sum(dcap) + 16,), FILL, dtype=torch.uint8, device=_dev())
    d_dst_n = torch.zeros(nf, dtype=torch.int64, device=_dev())
    bt = shafa.Batch(nb, 1 << 16)
    st = torch.cuda.Stream(device=_dev())
    try:
        bt.pack_payloads_files(st, first, counts, shafa.FRAME_SHAF, d_src, off, caps, d_n, d_dst, doff, dcap, d_dst_n)
        bt.finish(st, nb)
        got = d_dst.cpu().numpy().tobytes()
        want = b"".join(_payload_file(shafa.FRAME_SHAF, [src[off[b]:off[b] + sizes[b]].tobytes() for b in range(a, a + c)],
                                      shafa) for a, c in zip(first, counts))
        assert d_dst_n.cpu().tolist() == dcap
        assert got[:len(want)] == want and got[len(want):] == bytes([FILL]) * 16
    finally:
        bt.close()

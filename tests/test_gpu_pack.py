"""The four file formats assembled in device memory (shafa_hipd_pack_payloads / _pack_cod / _pack_freq, csrc/pack.hip) and
shafa.compress_files, which chains F -> T -> C -> the packs.

1. compress_files reproduces every golden session whose first command runs Module F (stored files byte for byte, the
   others by size + SHA-256);
2. each pack equals the C host's formatter (shafa.cod_format / freq_format plus host/modules.c's framing) over random
   shapes, destination misalignments 0..15, extreme tables and counts; nothing past *d_dst_n is written;
3. a file longer than dst_cap, or a size past its capacity, writes nothing and reports the documented codes;
4. the calls only enqueue;
5. what the device wrote decodes with the reference binary and with our CLI."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_fullsize import Session

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GUARD = 4096
FILL = 0xA5
F_KEYS = (".rle", ".rle.freq", ".freq")                  # what `-m f` writes
ALL_KEYS = (".rle", ".rle.freq", ".freq", ".rle.cod", ".rle.shaf", ".cod", ".shaf")
BLOCK = {"K": 655360, "m": 8 << 20, "M": 64 << 20}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _manifest(case):
    with open(os.path.join(GOLD, case, "manifest.json")) as f:
        return json.load(f)


def _first_cmd(case):
    c = _manifest(case)["cmds"][0]
    return c if isinstance(c, dict) else None


def _runs_f(case):
    """the session's first command runs Module F and succeeds: no -m, or -m f alone"""
    c = _first_cmd(case)
    if c is None or c["rc"] != 0:
        return False
    argv = c["argv"]
    mods = [argv[i + 1] for i, a in enumerate(argv) if a == "-m"]
    return mods in ([], ["f"])


F_CASES = sorted(c for c in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, c, "manifest.json")) and _runs_f(c))


def _opt(argv, flag):
    return argv[argv.index(flag) + 1] if flag in argv else None


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _case_input(shafa, case, man, fn):
    """the session's input: stored, or rebuilt the way test_gpu_fullsize.Session rebuilds it"""
    import golden.make_golden as mg
    path = os.path.join(GOLD, case, fn)
    if os.path.exists(path):
        return np.fromfile(path, dtype=np.uint8), None
    argv = man["cmds"][0]["argv"]
    if "generators" in man and _opt(argv, "-b") in ("m", "M"):
        S = Session(shafa, case)
        return S.data, S
    if "generators" in man:
        return mg.make_input(man["generators"][fn]), None
    # the two BASELINE config[0] inputs (their manifests' notes: runs_stream(7, 655360) and uniform gen_bytes(8, 655360))
    zt = mg.zipf_table(1.2)
    return (mg.runs_stream(7, 655360, zt) if case == "cfg0_K_runs" else mg.gen_bytes(8, 655360)), None


@pytest.mark.parametrize("case", F_CASES)
def test_compress_files_reproduce_reference_files(shafa, case):
    import torch
    man = _manifest(case)
    argv = man["cmds"][0]["argv"]
    fn = argv[0]
    data, S = _case_input(shafa, case, man, fn)
    try:
        assert _sha(data.tobytes()) == man["files"][fn]["sha256"]
        c = _opt(argv, "-c")
        bs = BLOCK.get(_opt(argv, "-b"), 65536)
        d_in = torch.from_numpy(data).to(_dev())
        files = shafa.compress_files(d_in, bs, force_rle=c == "r", force_freq=c == "f")
        keys = F_KEYS if _opt(argv, "-m") == "f" else ALL_KEYS
        want = {k for k in keys if fn + k in man["files"]}
        got = {k for k in files if k in keys}
        assert got == want, f"{case}: files {sorted(got)} != the reference's {sorted(want)}"
        for k in sorted(got):
            meta = man["files"][fn + k]
            b = files[k].cpu().numpy().tobytes()
            stored = os.path.join(GOLD, case, fn + k)
            if os.path.exists(stored):
                with open(stored, "rb") as f:
                    assert b == f.read(), f"{case}/{fn + k} differs from the stored file"
            assert len(b) == meta["size"], f"{case}/{fn + k}: {len(b)} bytes, the reference wrote {meta['size']}"
            assert _sha(b) == meta["sha256"], f"{case}/{fn + k} differs from the reference's"
    finally:
        if S is not None:
            S.close()


def test_compress_files_refuses_a_file_under_1_KiB(shafa):
    import torch
    data = np.fromfile(os.path.join(GOLD, "tiny_1023", "a"), dtype=np.uint8)
    with pytest.raises(shafa.ShafaError) as e:
        shafa.compress_files(torch.from_numpy(data).to(_dev()), 65536)
    assert e.value.code == shafa.FILE_TOO_SMALL


# ---------------------------------------------------------------- expected bytes (host formatter + host/modules.c framing)
def _cod_text(shafa, t):
    lens = bytes(t.len)
    if sum(lens) + 255 <= 33151:                          # SHAFA_COD_BLOCK_MAX: what shafa.cod_format's buffer holds
        return shafa.cod_format(t)
    fields = []
    for s in range(256):
        bits = bytes(t.bits[s])
        fields.append("".join("1" if (bits[i >> 3] >> (7 - (i & 7))) & 1 else "0" for i in range(lens[s])).encode())
    return b";".join(fields)


def _text_file(mode, sizes, texts):
    out = b"@" + mode + b"@" + str(len(sizes)).encode()
    for n, t in zip(sizes, texts):
        out += b"@" + str(int(n)).encode() + b"@" + t
    return out + b"@0"


def _payload_file(framing, blocks, shafa):
    if framing == shafa.FRAME_RAW:
        return b"".join(blocks)
    return b"@" + str(len(blocks)).encode() + b"".join(b"@" + str(len(b)).encode() + b"@" + b for b in blocks)


def _tables_dev(tables):
    import torch
    raw = b"".join(bytes(t) for t in tables)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(_dev())


def _u64_dev(vals):
    import torch
    return torch.from_numpy(np.asarray(vals, dtype=np.uint64).view(np.int64).copy()).to(_dev())


class Dst:
    """a destination of cap bytes at misalignment `mis`, with GUARD guard bytes behind it"""

    def __init__(self, cap, mis=0):
        import torch
        self.base = torch.full((cap + GUARD + 16 + 256,), FILL, dtype=torch.uint8, device=_dev())
        k = (-self.base.data_ptr()) % 256 + mis
        self.t = self.base[k:k + cap + GUARD]
        self.cap = cap
        self.n = torch.zeros(1, dtype=torch.int64, device=_dev())

    def reset(self):
        self.t.fill_(FILL)
        self.n.zero_()

    def check(self, want):
        """the file is `want`, and nothing behind it changed"""
        got = self.t.cpu().numpy().tobytes()
        n = int(self.n.item())
        assert n == len(want), f"*d_dst_n = {n}, the file has {len(want)} bytes"
        assert got[:n] == want, "file differs from the host formatter's"
        assert got[n:] == bytes([FILL]) * (len(got) - n), "bytes written past *d_dst_n"

    def untouched(self):
        got = self.t.cpu().numpy()
        assert (got == FILL).all(), "bytes written to d_dst by a refused pack"


# ---------------------------------------------------------------- random shapes
EDGES = [0, 1, 2, 9, 10, 11, 15, 16, 17, 31, 32, 33, 99, 100, 101, 999, 1000, 1001, 4095, 4096, 9999, 10000, 65535, 65536,
         99999, 100000, 100001, 999999, 1000000, 1 << 20]


def _payload_shape(rng, nb):
    sizes = []
    for _ in range(nb):
        r = rng.random()
        sizes.append(EDGES[int(rng.integers(len(EDGES)))] if r < 0.5 else int(rng.integers(0, 4096)) if r < 0.9 else
                     int(rng.integers(0, (1 << 20) + 1)))
    if nb > 64:                                            # keep the big shapes' total moderate
        sizes = [min(s, 70000) for s in sizes]
    caps = [s + int(rng.integers(0, 64)) for s in sizes]
    return sizes, caps


@pytest.mark.parametrize("nb,seed", [(1, 1), (2, 2), (3, 3), (7, 4), (16, 5), (64, 6), (300, 7)])
def test_pack_payloads_equal_host_framing(shafa, nb, seed):
    import torch
    rng = np.random.default_rng(seed)
    sizes, caps = _payload_shape(rng, nb)
    off, pos = [], 0
    for c in caps:
        off.append(pos)
        pos += (c + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
    src = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    src[src == ord("@")] = 0x41                            # ('@' inside payloads is legal; keep it rare, not absent)
    src[::997] = ord("@")
    d_src = torch.from_numpy(src).to(_dev())
    d_n = _u64_dev(sizes)
    blocks = [src[o:o + n].tobytes() for o, n in zip(off, sizes)]
    bt = shafa.Batch(nb, 1 << 20)
    st = torch.cuda.Stream(device=_dev())
    try:
        for framing in (shafa.FRAME_RAW, shafa.FRAME_SHAF):
            want = _payload_file(framing, blocks, shafa)
            cap = shafa.pack_payloads_max(caps, framing)
            assert cap >= len(want)
            for mis in range(16):
                dst = Dst(cap, mis)
                torch.cuda.synchronize()
                bt.pack_payloads(st, framing, d_src, off, caps, d_n, dst.t, cap, dst.n)
                bt.finish(st, nb)
                dst.check(want)
    finally:
        bt.close()


def _random_table(shafa, rng, kind):
    t = shafa.CodeTable()
    raw = rng.integers(0, 256, 256 * 32, dtype=np.uint8)    # bits past a code's length too: the formatter ignores them
    C.memmove(C.addressof(t.bits), raw.ctypes.data, 256 * 32)
    if kind == "empty":
        lens = np.zeros(256, dtype=np.uint8)
    elif kind == "long":
        lens = np.full(256, 255, dtype=np.uint8)
        lens[rng.integers(0, 256, 20)] = rng.integers(0, 255, 20).astype(np.uint8)
    elif kind == "sparse":
        lens = np.where(rng.random(256) < 0.1, rng.integers(1, 40, 256), 0).astype(np.uint8)
    else:
        lens = rng.integers(0, 256, 256).astype(np.uint8)
    C.memmove(C.addressof(t.len), lens.ctypes.data, 256)
    return t


def _random_counts(rng, kind):
    if kind == "zero":
        return np.zeros(256, dtype=np.uint64)
    if kind == "max":
        return np.full(256, 2 ** 64 - 1, dtype=np.uint64)
    if kind == "runs":
        vals = rng.choice(np.array([0, 1, 9, 10, 2 ** 64 - 1, 12345678901234567890], dtype=np.uint64), 256)
        f = np.repeat(vals[:16], 16)
        f[rng.integers(0, 256, 5)] = 2 ** 64 - 1
        return f.astype(np.uint64)
    f = rng.integers(0, 2 ** 63, 256, dtype=np.uint64) >> rng.integers(0, 64, 256).astype(np.uint64)
    f[rng.integers(0, 256, 8)] = 0
    return f


SIZE_EDGES = [0, 1, 9, 10, 99, 100, 65536, 2 ** 32, 2 ** 64 - 1, 10 ** 19 - 1, 10 ** 19]


@pytest.mark.parametrize("nb,seed", [(1, 11), (2, 12), (9, 13), (10, 14), (100, 15), (300, 16)])
def test_pack_cod_and_freq_equal_host_formatter(shafa, nb, seed):
    import torch
    rng = np.random.default_rng(seed)
    kinds_t = ["random", "long", "empty", "sparse"]
    kinds_f = ["random", "zero", "max", "runs"]
    tables = [_random_table(shafa, rng, kinds_t[b % 4] if nb > 1 else "long") for b in range(nb)]
    counts = np.stack([_random_counts(rng, kinds_f[b % 4] if nb > 1 else "runs") for b in range(nb)])
    sizes = [SIZE_EDGES[int(rng.integers(len(SIZE_EDGES)))] if rng.random() < 0.6 else int(rng.integers(0, 2 ** 63)) for _ in range(nb)]
    d_sizes = _u64_dev(sizes)
    d_tab = _tables_dev(tables)
    d_freq = _u64_dev(counts.reshape(-1))
    bt = shafa.Batch(nb, 1 << 16)
    st = torch.cuda.Stream(device=_dev())
    try:
        for mode in (b"R", b"N"):
            want_cod = _text_file(mode, sizes, [_cod_text(shafa, t) for t in tables])
            want_freq = _text_file(mode, sizes, [shafa.freq_format(counts[b]) for b in range(nb)])
            for mis in (0, 1, 7, 15) if mode == b"R" else (3, 8):
                dst = Dst(shafa.pack_cod_max(nb), mis)
                torch.cuda.synchronize()
                bt.pack_cod(st, nb, mode, d_sizes, d_tab, dst.t, dst.cap, dst.n)
                bt.finish(st, nb)
                dst.check(want_cod)
                dst = Dst(shafa.pack_freq_max(nb), mis)
                torch.cuda.synchronize()
                bt.pack_freq(st, nb, mode, d_sizes, d_freq, dst.t, dst.cap, dst.n)
                bt.finish(st, nb)
                dst.check(want_freq)
    finally:
        bt.close()


# ---------------------------------------------------------------- overflow and bad sizes
def test_overflow_and_bad_sizes_write_nothing(shafa):
    import torch
    rng = np.random.default_rng(21)
    nb = 4
    sizes = [1000, 0, 70001, 17]
    caps = [s + 40 for s in sizes]
    off, pos = [], 0
    for c in caps:
        off.append(pos)
        pos += (c + 15) // 16 * 16
    src = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    d_src = torch.from_numpy(src).to(_dev())
    d_n = _u64_dev(sizes)
    blocks = [src[o:o + n].tobytes() for o, n in zip(off, sizes)]
    tables = [_random_table(shafa, rng, "random") for _ in range(nb)]
    counts = np.stack([_random_counts(rng, "random") for _ in range(nb)])
    d_tab, d_freq = _tables_dev(tables), _u64_dev(counts.reshape(-1))
    bt = shafa.Batch(nb, 1 << 17)
    st = torch.cuda.Stream(device=_dev())

    def calls():
        yield "raw", _payload_file(shafa.FRAME_RAW, blocks, shafa), \
            lambda d, cap: bt.pack_payloads(st, shafa.FRAME_RAW, d_src, off, caps, d_n, d.t, cap, d.n)
        yield "shaf", _payload_file(shafa.FRAME_SHAF, blocks, shafa), \
            lambda d, cap: bt.pack_payloads(st, shafa.FRAME_SHAF, d_src, off, caps, d_n, d.t, cap, d.n)
        yield "cod", _text_file(b"N", sizes, [_cod_text(shafa, t) for t in tables]), \
            lambda d, cap: bt.pack_cod(st, nb, b"N", d_n, d_tab, d.t, cap, d.n)
        yield "freq", _text_file(b"R", sizes, [shafa.freq_format(c) for c in counts]), \
            lambda d, cap: bt.pack_freq(st, nb, b"R", d_n, d_freq, d.t, cap, d.n)

    try:
        for name, want, call in calls():
            need = len(want)
            d = Dst(need, 5)
            torch.cuda.synchronize()
            call(d, need)                                                  # exactly the size needed: passes
            bt.finish(st, nb)
            d.check(want)
            for cap in (need - 1, need - 17, 0):
                d.reset()
                torch.cuda.synchronize()
                call(d, cap)
                rc, errs = bt.finish(st, nb, raise_on_error=False)
                assert rc == shafa.LACK_OF_MEMORY and errs[0] == shafa.LACK_OF_MEMORY, (name, cap, rc, errs)
                assert all(e == 0 for e in errs[1:]), (name, cap, errs)
                assert int(d.n.item()) == need, (name, cap)
                d.untouched()
        # a size past its capacity: block 2, nothing written
        bad = list(sizes)
        bad[2] = caps[2] + 1
        d_bad = _u64_dev(bad)
        for framing in (shafa.FRAME_RAW, shafa.FRAME_SHAF):
            d = Dst(shafa.pack_payloads_max(caps, framing) + 64)
            torch.cuda.synchronize()
            bt.pack_payloads(st, framing, d_src, off, caps, d_bad, d.t, d.cap, d.n)
            rc, errs = bt.finish(st, nb, raise_on_error=False)
            assert rc == shafa.OUTSIDE_MODULE and errs == [0, 0, shafa.OUTSIDE_MODULE, 0], (framing, rc, errs)
            d.untouched()
    finally:
        bt.close()


# ---------------------------------------------------------------- enqueue only
def test_no_synchronisation_inside_the_calls(oracle, shafa):
    """With a long piece of GPU work in front of it on the stream, F -> T -> C -> every pack enqueues and returns while the
    stream is still busy; one synchronisation at the end, then the files are checked against the host's."""
    import torch
    dev = _dev()
    zt = shafa.zipf_table(1.2)
    sizes = [1 << 20, (1 << 20) - 5, 333333, 4097]
    blocks = [oracle.gen_bytes(1900 + i, n, zt) for i, n in enumerate(sizes)]
    nb = len(blocks)
    off, pos = [], 0
    for n in sizes:
        off.append(pos)
        pos += (n + 15) // 16 * 16
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, b in zip(off, blocks):
        host[o:o + b.size] = b
    d_in = torch.from_numpy(host).to(dev)
    d_n_in = torch.tensor(sizes, dtype=torch.int64, device=dev)
    tsz = C.sizeof(shafa.CodeTable)
    d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
    d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
    thb = [(shafa.tile_hist_bytes(n) + 15) // 16 * 16 for n in sizes]
    toff = [sum(thb[:b]) for b in range(nb)]
    d_th = torch.zeros(sum(thb) + 16, dtype=torch.uint8, device=dev)
    caps = [n * 2 + 16 for n in sizes]
    ooff = [sum((c + 15) // 16 * 16 for c in caps[:b]) for b in range(nb)]
    d_out = torch.zeros(ooff[-1] + caps[-1] + 16, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(nb, dtype=torch.int64, device=dev)
    shaf, cod, freq = Dst(shafa.pack_payloads_max(caps, shafa.FRAME_SHAF)), Dst(shafa.pack_cod_max(nb)), \
        Dst(shafa.pack_freq_max(nb))
    st = torch.cuda.Stream(device=dev)
    bt = shafa.Batch(nb, max(sizes))

    def enqueue():
        bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
        bt.sf_build_codes(st, nb, d_freq, d_tab)
        bt.sf_encode_dev(st, d_in, off, sizes, d_n_in, d_tab, d_out, ooff, caps, d_n, d_th, toff)
        bt.pack_freq(st, nb, b"N", d_n_in, d_freq, freq.t, freq.cap, freq.n)
        bt.pack_cod(st, nb, b"N", d_n_in, d_tab, cod.t, cod.cap, cod.n)
        bt.pack_payloads(st, shafa.FRAME_SHAF, d_out, ooff, caps, d_n, shaf.t, shaf.cap, shaf.n)

    try:
        enqueue()                                                                          # warm-up: the batch grows here
        bt.finish(st, nb)
        for d in (shaf, cod, freq):
            d.reset()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            torch.cuda._sleep(200_000_000)                                                 # ~0.1 s of one busy wave
        enqueue()
        busy = not st.query()
        bt.finish(st, nb)
        assert busy, "the stream had drained when the calls returned: something synchronised"
        hists = [oracle.hist256(b) for b in blocks]
        tabs = [oracle.sf_build(h) for h in hists]
        encs = []
        for b, t in zip(blocks, tabs):
            rc, e = oracle.sf_encode(b, t)
            assert rc == 0
            encs.append(e.tobytes())
        freq.check(_text_file(b"N", sizes, [shafa.freq_format(h) for h in hists]))
        cod.check(_text_file(b"N", sizes, [shafa.cod_format(shafa.sf_build_codes(h)) for h in hists]))
        shaf.check(_payload_file(shafa.FRAME_SHAF, encs, shafa))
    finally:
        bt.close()


# ---------------------------------------------------------------- interop: the device's files decode
def _decode_with(binary, work, name, want):
    r = subprocess.run([binary, name, "-m", "d"], cwd=work, capture_output=True, timeout=300)
    assert r.returncode == 0, (binary, r.returncode, r.stderr[-2000:])
    stem = name[:-len(".shaf")]
    out = os.path.join(work, stem[:-len(".rle")] if stem.endswith(".rle") else stem)
    with open(out, "rb") as f:
        assert f.read() == want, f"{binary}: decoded {name} differs from the input"
    os.remove(out)


def _device_files(shafa, tmp_path, kind):
    """compress_files of a small random input (plain bytes or runs), its .cod / .shaf written to tmp_path"""
    import torch
    import golden.make_golden as mg
    rng = np.random.default_rng(31 if kind == "plain" else 32)
    n = 65536 * 3 + int(rng.integers(100, 60000))
    data = mg.gen_bytes(4000 + n % 97, n) if kind == "plain" else mg.runs_stream(41, n, mg.zipf_table(1.2))
    files = shafa.compress_files(torch.from_numpy(data).to(_dev()), 65536)
    stem = ".rle" if kind == "rle" else ""
    assert (stem + ".shaf") in files, sorted(files)
    for k in (stem + ".cod", stem + ".shaf"):
        files[k].cpu().numpy().tofile(str(tmp_path / ("x" + k)))
    return "x" + stem + ".shaf", data.tobytes()


@pytest.mark.parametrize("kind", ["plain", "rle"])
def test_device_files_decode_with_our_cli(shafa, tmp_path, kind):
    name, want = _device_files(shafa, tmp_path, kind)
    _decode_with(shafa.CLI_PATH, str(tmp_path), name, want)


@pytest.mark.parametrize("kind", ["plain", "rle"])
def test_device_files_decode_with_reference_binary(shafa, tmp_path, kind):
    import oracle_lib
    if not os.path.exists(oracle_lib.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref/shafa)")
    name, want = _device_files(shafa, tmp_path, kind)
    _decode_with(oracle_lib.REF_BIN, str(tmp_path), name, want)

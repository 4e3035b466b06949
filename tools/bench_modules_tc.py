"""Modules T and C alone on files in device memory (shafa_hipd_unpack_freq, csrc/unpack.hip; shafa.build_cod /
shafa.encode_files) against the host's Module T and against the encode chain with tables already resident.  Standalone; one
MI355X; median, min, max over --reps.

  python tools/bench_modules_tc.py [--reps 7] [--freq-blocks 1,8,128,32768] [--blocks 1,8,128]

Rows:
  unpack_freq[nb]:   Batch.unpack_freq of a .freq of nb blocks of Zipf(1.2) counts (HIP events, ms), the text's bytes;
  build_cod[nb]:     build_cod of that text, resident (wall clock, its two synchronisations included), against the host path on
                     the same text, resident in host memory: the framing in Python, then shafa.freq_parse per block,
                     shafa.sf_build_codes_batch and shafa.cod_format per block through shafa.host(); the two .cod are compared;
  encode_files[nb]:  encode_files(d_in, cod) at nb x 64 MiB Zipf(1.2) (wall clock, its three synchronisations included)
                     against (a) sf_encode_dev + pack_payloads(SHAF) + finish and (b) hist256_tiles + sf_encode_dev with the
                     tile histograms + pack_payloads + finish, both on the same resident blocks with the tables already
                     resident and the regions sized beforehand (wall clock).  encode_files minus (b) is the parse, its
                     synchronisation, the size pass with its synchronisation and the allocations.
Prints one JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(torch, st, fn, reps):
    fn()
    st.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        xs.append((time.perf_counter() - t0) * 1e3)
    return xs


def freq_text(pkg, np, nb, seed):
    """a mode-N .freq of nb blocks: Zipf(1.2) counts of blocks of 48..64 KiB, over a per-block rotation of the symbols"""
    rng = np.random.default_rng(seed)
    w = np.arange(1, 257, dtype=np.float64) ** -1.2
    w /= w.sum()
    parts = [b"@N@%d" % nb]
    for _ in range(nb):
        n = int(rng.integers(48 << 10, (64 << 10) + 1))
        c = np.floor(w * n).astype(np.uint64)
        c[0] += np.uint64(n - int(c.sum()))
        c = np.roll(c, int(rng.integers(256)))
        parts.append(b"@%d@" % n + pkg.freq_format(c))
    return b"".join(parts) + b"@0"


def host_module_t(pkg, np, text):
    """what get_shafa_codes does with the text, through shafa.host(): -> the .cod"""
    parts = text.split(b"@")
    mode, nb = parts[1], int(parts[2])
    freq = np.zeros((nb, 256), dtype=np.uint64)
    for b in range(nb):
        rc, f = pkg.freq_parse(parts[4 + 2 * b])
        assert rc == 0
        freq[b] = f
    tabs = pkg.sf_build_codes_batch(freq)
    out = [b"@" + mode + b"@%d" % nb]
    for b in range(nb):
        out.append(b"@" + parts[3 + 2 * b] + b"@" + pkg.cod_format(tabs[b]))
    return b"".join(out) + b"@0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--freq-blocks", default="1,8,128,32768")
    ap.add_argument("--blocks", default="1,8,128")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    res = {"unpack_freq": {}, "build_cod": {}, "encode_files": {}}
    # ---- Module T
    for nb in [int(x) for x in args.freq_blocks.split(",")]:
        text = freq_text(pkg, np, nb, 77 + nb)
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        mb = pkg.unpack_max_blocks(len(text), "counts")
        bt = pkg.Batch(mb, 1 << 20)
        info = torch.zeros(8, dtype=torch.int64, device=dev)
        sizes = torch.zeros(mb, dtype=torch.int64, device=dev)
        counts = torch.empty(mb * 256, dtype=torch.int64, device=dev)
        ms = timed(torch, st, lambda: bt.unpack_freq(st, mb, d_text, info, sizes, counts), args.reps)
        bt.finish(st, mb)
        bt.close()
        res["unpack_freq"][nb] = {"ms": stats(ms), "text_bytes": len(text), "slots": mb}
        got = []
        dev_ms = wall(torch, lambda: got.append(pkg.build_cod(d_text, stream=st)), args.reps)
        want = []
        t_host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            want.append(host_module_t(pkg, np, text))
            t_host.append((time.perf_counter() - t0) * 1e3)
        same = got[-1].cpu().numpy().tobytes() == want[-1]
        res["build_cod"][nb] = {"build_cod_ms": stats(dev_ms), "host_path_ms": stats(t_host), "identical": same,
                                "cod_bytes": len(want[-1])}
        del d_text, info, sizes, counts, got
    # ---- Module C
    bs = 64 << 20
    tsz = 8448
    d_map = torch.from_numpy(pkg.zipf_table(1.2)).to(dev)
    for nb in sorted({int(x) for x in args.blocks.split(",")}, reverse=True):
        d_in = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            pkg.gen_bytes(st, 4343 + nb, 0, d_in, nb * bs, d_map)
        st.synchronize()
        files = pkg.compress_files(d_in, bs)
        cod, shaf = files[".cod"], files[".shaf"]
        del files
        out = []
        full = wall(torch, lambda: out.append(pkg.encode_files(d_in, cod, stream=st)), args.reps)
        same = torch.equal(out[-1], shaf)
        del out
        # the chain with everything resident: tables and sizes parsed once, the regions sized beforehand
        mb = pkg.unpack_max_blocks(cod.numel(), "cod")
        bt = pkg.Batch(mb, 1 << 20)
        info = torch.zeros(8, dtype=torch.int64, device=dev)
        d_n = torch.zeros(mb, dtype=torch.int64, device=dev)
        tab = torch.empty(mb * tsz, dtype=torch.uint8, device=dev)
        bt.unpack_cod(st, mb, cod, info, d_n, tab)
        bt.finish(st, mb)
        sizes = [bs] * nb
        off = [b * bs for b in range(nb)]
        ocap = [n + n // 2 + 64 for n in sizes]
        ooff = [sum((c + 15) // 16 * 16 for c in ocap[:i]) for i in range(nb)]
        d_enc = torch.empty(ooff[-1] + ocap[-1] + 32, dtype=torch.uint8, device=dev)
        d_enc_n = torch.zeros(nb, dtype=torch.int64, device=dev)
        dst = torch.empty(pkg.pack_payloads_max(ocap, pkg.FRAME_SHAF), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
        thb = [(pkg.tile_hist_bytes(n) + 15) // 16 * 16 for n in sizes]
        toff = [sum(thb[:i]) for i in range(nb)]
        d_th = torch.empty(sum(thb) + 16, dtype=torch.uint8, device=dev)

        def chain(tiles):
            if tiles:
                bt.hist256_tiles(st, d_in, off, sizes, d_freq, d_th, toff)
                bt.sf_encode_dev(st, d_in, off, sizes, d_n[:nb], tab, d_enc, ooff, ocap, d_enc_n, d_th, toff)
            else:
                bt.sf_encode_dev(st, d_in, off, sizes, d_n[:nb], tab, d_enc, ooff, ocap, d_enc_n)
            bt.pack_payloads(st, pkg.FRAME_SHAF, d_enc, ooff, ocap, d_enc_n, dst, dst.numel(), d_len)
            bt.finish(st, nb)

        row = {"encode_files_ms": stats(full), "identical": bool(same)}
        for name, tiles in (("resident_chain_ms", False), ("resident_chain_with_hist_ms", True)):
            row[name] = stats(wall(torch, lambda: chain(tiles), args.reps))
            assert torch.equal(dst[:int(d_len.item())], shaf)
        row["beyond_chain_with_hist_ms"] = round(row["encode_files_ms"]["median"]
                                                 - row["resident_chain_with_hist_ms"]["median"], 3)
        res["encode_files"][nb] = row
        bt.close()
        del d_in, cod, shaf, d_enc, dst, d_th, tab
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

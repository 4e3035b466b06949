"""The file parsers (shafa_hipd_unpack_*, csrc/unpack.hip) and shafa.decompress_files against the decode chain fed host-parsed
tables and sizes.  Standalone; HIP events around each device row (median, min, max over --reps) on one MI355X.

  python tools/bench_unpack_dev.py [--reps 7] [--blocks 1,8,128] [--walk 32,128,4096,32768]

Rows:
  unpack_cod[nb]:     Batch.unpack_cod of the .cod of nb x 64 MiB Zipf(1.2) blocks (ms);
  shaf_walk[nb]:      Batch.unpack_shaf over a synthetic .shaf of nb blocks of 64..4095 bytes: ms and us per block;
  unpack_payloads:    the 128 x 64 MiB .shaf's payloads into aligned regions: ms, GB/s on 2 x payload bytes, fraction of 8 TB/s;
  decompress[nb]:     decompress_files(shaf, cod) end to end (wall clock: its synchronisations included) against
                      sf_decode_dev + pack_payloads on the same payloads already resident in aligned regions with the tables
                      and sizes uploaded from the host (events), at nb x 64 MiB.  The difference is the device parsing.
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
PEAK = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", default="1,8,128")
    ap.add_argument("--walk", default="32,128,4096,32768")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    bs = 64 << 20
    tsz = 8448
    d_map = torch.from_numpy(pkg.zipf_table(1.2)).to(dev)
    res = {"unpack_cod": {}, "shaf_walk": {}, "decompress": {}}
    # ---- the .shaf walk on synthetic files
    rng = np.random.default_rng(5)
    for nb in [int(x) for x in args.walk.split(",")]:
        sizes = rng.integers(64, 4096, nb)
        parts = [b"@%d" % nb]
        for n in sizes:
            parts.append(b"@%d@" % n + bytes(int(n)))
        shaf = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).to(dev)
        bt = pkg.Batch(nb, 1 << 20)
        cnt = torch.tensor([nb], dtype=torch.int64, device=dev)
        off, n = torch.zeros(nb, dtype=torch.int64, device=dev), torch.zeros(nb, dtype=torch.int64, device=dev)
        ms = timed(torch, st, lambda: bt.unpack_shaf(st, nb, shaf, cnt, off, n), args.reps)
        bt.finish(st, nb)
        res["shaf_walk"][nb] = {"ms": stats(ms), "us_per_block": round(statistics.median(ms) * 1000 / nb, 3)}
        bt.close()
    # ---- sessions of nb x 64 MiB Zipf(1.2)
    for nb in sorted({int(x) for x in args.blocks.split(",")}, reverse=True):
        d_in = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            pkg.gen_bytes(st, 4343 + nb, 0, d_in, nb * bs, d_map)
        st.synchronize()
        files = pkg.compress_files(d_in, bs)
        cod, shaf = files[".cod"], files[".shaf"]
        mb = pkg.unpack_max_blocks(cod.numel(), "cod")
        bt = pkg.Batch(mb, 1 << 20)
        info = torch.zeros(8, dtype=torch.int64, device=dev)
        nsym, poff, pn = (torch.zeros(mb, dtype=torch.int64, device=dev) for _ in range(3))
        tab = torch.empty(mb * tsz, dtype=torch.uint8, device=dev)
        ms = timed(torch, st, lambda: bt.unpack_cod(st, mb, cod, info, nsym, tab), args.reps)
        res["unpack_cod"][nb] = {"ms": stats(ms), "cod_bytes": int(cod.numel())}
        bt.unpack_shaf(st, mb, shaf, info[3:4], poff, pn)
        bt.finish(st, mb)
        ps = poff.cpu().tolist()[:nb]
        ns = pn.cpu().tolist()[:nb]
        sy = nsym.cpu().tolist()[:nb]
        al = lambda v: [sum((x + 15) // 16 * 16 for x in v[:i]) for i in range(len(v))]
        ro, so = al(ns), al(sy)
        pay = torch.empty(sum((x + 15) // 16 * 16 for x in ns) + 16, dtype=torch.uint8, device=dev)
        if nb == 128:
            ms = timed(torch, st, lambda: bt.unpack_payloads(st, shaf, poff, pn, pay, ro, ns), args.reps)
            gbs = 2 * sum(ns) / (statistics.median(ms) / 1e3) / 1e9
            res["unpack_payloads"] = {"blocks": nb, "ms": stats(ms), "GB_s": round(gbs, 1),
                                      "peak_frac": round(gbs * 1e9 / PEAK, 3)}
        bt.unpack_payloads(st, shaf, poff, pn, pay, ro, ns)
        bt.finish(st, mb)
        # the reference chain: tables and sizes parsed on the host and uploaded, payloads already resident
        host_cod = cod.cpu().numpy().tobytes()
        texts = host_cod.split(b"@")[4:4 + 2 * nb:2]
        tables = b"".join(bytes(pkg.cod_parse(t)[1]) for t in texts)
        out = torch.empty(sum(sy) + 16, dtype=torch.uint8, device=dev)
        olen = torch.zeros(1, dtype=torch.int64, device=dev)
        sfo = torch.empty(sum((x + 15) // 16 * 16 for x in sy) + 16, dtype=torch.uint8, device=dev)

        def ref():
            d_tab = torch.frombuffer(bytearray(tables), dtype=torch.uint8).to(dev, non_blocking=False)
            d_pn = torch.tensor(ns, dtype=torch.int64, device=dev)
            d_sy = torch.tensor(sy, dtype=torch.int64, device=dev)
            bt.sf_decode_dev(st, pay, ro, ns, d_pn, d_tab, d_sy, sfo, so, sy)
            bt.pack_payloads(st, pkg.FRAME_RAW, sfo, so, sy, d_sy, out, out.numel(), olen)
            bt.finish(st, mb)

        def full():
            pkg.decompress_files(shaf=shaf, cod=cod, decode_rle=False, stream=st)

        row = {}
        for name, fn in (("host_parsed_chain", ref), ("decompress_files", full)):
            fn()
            torch.cuda.synchronize()
            xs = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                xs.append((time.perf_counter() - t0) * 1e3)
            row[name] = stats(xs)
        assert int(olen.item()) == nb * bs and torch.equal(out[:nb * bs], d_in)
        row["parse_cost_ms"] = round(row["decompress_files"]["median"] - row["host_parsed_chain"]["median"], 3)
        res["decompress"][nb] = row
        bt.close()
        del d_in, files, cod, shaf, pay, sfo, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

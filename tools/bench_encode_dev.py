"""Module C from device tables (shafa_hipd_sf_encode_dev) against the host-table entry points, and F -> T -> C with one
synchronisation against today's chain with its round trip.  Standalone; HIP events for the Module C rows, wall clock for the
chains (their host steps are part of what is measured); the compared shapes alternate within one process.

  python tools/bench_encode_dev.py [--reps 7] [--steps 10] [--chain-rounds 15]

Prints one JSON document:
  module_c:  128 x 64 MiB Zipf(1.2), chained form (no tile histograms) and tile-histogram form: ms per call, host entry
             vs sf_encode_dev (median, min, max over the repetitions) and the ratio of the medians; "generic": the same
             launch with block 0's table given one 40-bit code (a rare symbol), so that block takes the generic kernel;
  chain:     1, 2, 8, 32 blocks of 64 MiB Zipf(1.2): rle_encode_tiles -> T -> sf_encode_tiles today (sizes and histograms
             read back; T on the host, or on the device plus a read-back of the tables) and the host-free chain
             (rle_encode_tiles -> sf_build_codes -> sf_encode_dev, one synchronisation): ms per round.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--chain-rounds", type=int, default=15)
    ap.add_argument("--module-c-blocks", type=int, default=128)
    ap.add_argument("--module-c-only", action="store_true", help="skip the F -> T -> C rows")
    ap.add_argument("--zipf-s", type=float, default=1.2, help="Zipf exponent of the Module C rows (1.6: Lmax 15)")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    bs = 64 << 20
    tsz = C.sizeof(pkg.CodeTable)
    d_map = torch.from_numpy(pkg.zipf_table(1.2)).to(dev)
    d_map_c = torch.from_numpy(pkg.zipf_table(args.zipf_s)).to(dev)
    res = {"module_c": {}, "chain": {}}

    # ---- Module C alone: 128 x 64 MiB Zipf(1.2) ---------------------------------------------------------------------
    nb = args.module_c_blocks
    d_in = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(st):
        pkg.gen_bytes(st, 20240601, 0, d_in, nb * bs, d_map_c)
    off, n = [b * bs for b in range(nb)], [bs] * nb
    thb = pkg.tile_hist_bytes(bs)
    thoff = [b * thb for b in range(nb)]
    d_th = torch.zeros(nb * thb, dtype=torch.uint8, device=dev)
    d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
    d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
    bt = pkg.Batch(nb, bs)
    bt.hist256_tiles(st, d_in, off, n, d_freq, d_th, thoff)
    bt.sf_build_codes(st, nb, d_freq, d_tab)
    bt.finish(st, nb)
    raw = d_tab.cpu().numpy().tobytes()
    tabs = (pkg.CodeTable * nb)()
    C.memmove(tabs, raw, nb * tsz)
    lmax = max(max(bytes(t.len)) for t in tabs)
    cap = bs * lmax // 8 + (1 << 20)                  # (1 MiB more: the generic row's 40-bit code of a rare symbol)
    gtabs = (pkg.CodeTable * nb)()
    C.memmove(gtabs, raw, nb * tsz)
    rare = min((s for s in range(256) if gtabs[0].len[s]), key=lambda s: -gtabs[0].len[s])    # block 0's longest code
    gtabs[0].len[rare] = 40
    d_gtab = torch.from_numpy(np.frombuffer(bytes(gtabs), dtype=np.uint8).copy()).to(dev)
    ooff = [b * cap for b in range(nb)]
    d_out = torch.empty(nb * cap, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(nb, dtype=torch.int64, device=dev)
    d_n_in = torch.tensor(n, dtype=torch.int64).to(dev)
    forms = {
        "chained": (lambda: bt.sf_encode(st, d_in, off, n, tabs, d_out, ooff, [cap] * nb, d_n),
                    lambda: bt.sf_encode_dev(st, d_in, off, n, d_n_in, d_tab, d_out, ooff, [cap] * nb, d_n)),
        "tiles": (lambda: bt.sf_encode_tiles(st, d_in, off, n, tabs, d_th, thoff, d_out, ooff, [cap] * nb, d_n),
                  lambda: bt.sf_encode_dev(st, d_in, off, n, d_n_in, d_tab, d_out, ooff, [cap] * nb, d_n, d_th, thoff)),
        "generic": (lambda: bt.sf_encode(st, d_in, off, n, gtabs, d_out, ooff, [cap] * nb, d_n),
                    lambda: bt.sf_encode_dev(st, d_in, off, n, d_n_in, d_gtab, d_out, ooff, [cap] * nb, d_n)),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.steps):
            fn()
        e1.record(st)
        bt.finish(st, nb)
        return e0.elapsed_time(e1) / args.steps

    for name, (host_fn, dev_fn) in forms.items():
        host_fn(); bt.finish(st, nb)
        want = d_out.cpu().numpy().copy(); want_n = d_n.cpu().numpy().copy()
        d_out.zero_()
        dev_fn(); bt.finish(st, nb)
        same = bool((d_n.cpu().numpy() == want_n).all()) and all(
            np.array_equal(d_out[o:o + int(k)].cpu().numpy(), want[o:o + int(k)]) for o, k in zip(ooff, want_n))
        th, td = [], []
        for _ in range(args.reps):                    # alternated: host entry, device entry, host entry, ...
            th.append(timed(host_fn))
            td.append(timed(dev_fn))
        gib = nb * bs / 2 ** 30
        res["module_c"][name] = {"workload": f"{nb} x 64 MiB Zipf({args.zipf_s}), Lmax {lmax}" +
                                 (", block 0 with a 40-bit code" if name == "generic" else ""), "identical": same,
                                 "host_tables_ms": stats(th), "dev_tables_ms": stats(td),
                                 "dev_over_host": round(statistics.median(td) / statistics.median(th), 4),
                                 "host_GiBs": round(gib / (statistics.median(th) * 1e-3), 1),
                                 "dev_GiBs": round(gib / (statistics.median(td) * 1e-3), 1)}
    bt.close()
    del d_in, d_out, d_th
    torch.cuda.empty_cache()

    # ---- F -> T -> C: today's chain and the host-free one -----------------------------------------------------------
    for nb in (() if args.module_c_only else (1, 2, 8, 32)):
        d_in = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            pkg.gen_bytes(st, 777 + nb, 0, d_in, nb * bs, d_map)
        off, n = [b * bs for b in range(nb)], [bs] * nb
        rcap = 2 * bs + 64
        roff = [b * rcap for b in range(nb)]
        thb = pkg.tile_hist_bytes(rcap)
        thoff = [b * thb for b in range(nb)]
        d_rle = torch.empty(nb * rcap, dtype=torch.uint8, device=dev)
        d_rle_n = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
        d_th = torch.zeros(nb * thb, dtype=torch.uint8, device=dev)
        d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
        ocap = rcap * 3 + 16                          # 24 bits per RLE byte: more than Zipf(1.2)'s codes need
        ooff = [b * ocap for b in range(nb)]
        d_out = torch.empty(nb * ocap, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(nb, dtype=torch.int64, device=dev)
        bt = pkg.Batch(nb, rcap)
        h_tabs = (pkg.CodeTable * nb)()

        def today_host_t():
            bt.rle_encode_tiles(st, d_in, off, n, d_rle, roff, [rcap] * nb, d_rle_n, d_freq, d_th, thoff)
            bt.finish(st, nb)
            rn = [int(x) for x in d_rle_n.cpu().numpy()]
            tabs = pkg.sf_build_codes_batch(d_freq.cpu().numpy().astype(np.uint64).reshape(nb, 256))
            bt.sf_encode_tiles(st, d_rle, roff, rn, tabs, d_th, thoff, d_out, ooff, [ocap] * nb, d_n)
            bt.finish(st, nb)

        def today_dev_t():
            bt.rle_encode_tiles(st, d_in, off, n, d_rle, roff, [rcap] * nb, d_rle_n, d_freq, d_th, thoff)
            bt.sf_build_codes(st, nb, d_freq, d_tab)
            bt.finish(st, nb)
            rn = [int(x) for x in d_rle_n.cpu().numpy()]
            C.memmove(h_tabs, d_tab.cpu().numpy().tobytes(), nb * tsz)
            bt.sf_encode_tiles(st, d_rle, roff, rn, h_tabs, d_th, thoff, d_out, ooff, [ocap] * nb, d_n)
            bt.finish(st, nb)

        def host_free():
            bt.rle_encode_tiles(st, d_in, off, n, d_rle, roff, [rcap] * nb, d_rle_n, d_freq, d_th, thoff)
            bt.sf_build_codes(st, nb, d_freq, d_tab)
            bt.sf_encode_dev(st, d_rle, roff, [rcap] * nb, d_rle_n, d_tab, d_out, ooff, [ocap] * nb, d_n, d_th, thoff)
            bt.finish(st, nb)

        variants = {"today_host_T": today_host_t, "today_dev_T_readback": today_dev_t, "host_free": host_free}
        outs = {}
        for name, fn in variants.items():             # warm-up (the batch grows) and the results to compare
            fn()
            outs[name] = (d_n.cpu().numpy().copy(), d_out.cpu().numpy().copy())
        ref_n, ref_out = outs["today_host_T"]
        same = all(np.array_equal(v[0], ref_n) and all(np.array_equal(v[1][o:o + int(k)], ref_out[o:o + int(k)])
                                                       for o, k in zip(ooff, ref_n)) for v in outs.values())
        times = {k: [] for k in variants}
        torch.cuda.synchronize()
        for _ in range(args.chain_rounds):
            for name, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"identical": same}
        row.update({f"{k}_ms": stats(v) for k, v in times.items()})
        row["host_free_over_today_host_T"] = round(statistics.median(times["host_free"]) /
                                                   statistics.median(times["today_host_T"]), 4)
        res["chain"][f"{nb}_blocks"] = row
        bt.close()
        del d_in, d_rle, d_out, d_th
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Module D from device tables (shafa_hipd_sf_decode_dev) against the host-table entry (shafa_hipd_sf_decode), and
F -> T -> C -> D with one synchronisation against the chain that reads tables and sizes back before it decodes.
Standalone; HIP events for the Module D rows, wall clock for the chains; the compared shapes alternate within one process.

  python tools/bench_decode_dev.py [--reps 7] [--legs zipf_128x64M,chain] [--entries host|dev|both]

--legs keeps the named rows (module_d names, or "chain"); --entries times one entry only (for a kernel trace of one side).

Prints one JSON document:
  module_d: ms per call, host entry vs sf_decode_dev (median, min, max) and the ratio of the medians, for
            zipf_128x64M (the headline shape), runs_128x8M (run-heavy data), zipf_{1,2,8}x64M, uniform_8x64M (exact
            kernels, no speculation) and long33_1x64M (one block whose code has more than 32 bits: the byte-map list);
  chain:    1, 2, 8, 32 blocks of 64 MiB Zipf(1.2): hist256_tiles -> sf_build_codes -> sf_encode_dev -> read back tables and
            sizes -> sf_decode, against the same with sf_decode_dev and one synchronisation: ms per round.
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
    ap.add_argument("--chain-rounds", type=int, default=7)
    ap.add_argument("--legs", default="", help="comma-separated rows to run (default: all)")
    ap.add_argument("--entries", default="both", choices=("host", "dev", "both"))
    args = ap.parse_args()
    legs = set(x for x in args.legs.split(",") if x)
    want = lambda name: not legs or name in legs
    import numpy as np
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    tsz = C.sizeof(pkg.CodeTable)
    res = {"module_d": {}, "chain": {}}

    def encode(d_in, nb, bs, tables=None):
        """Encode nb blocks of bs bytes (their own Module T tables unless given) -> (d_e, eoff, en, tables)."""
        off, n = [b * bs for b in range(nb)], [bs] * nb
        bt = pkg.Batch(nb, 3 * bs + 16)
        if tables is None:
            d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
            bt.hist256(st, d_in, off, n, d_freq)
            bt.finish(st, nb)
            freq = d_freq.cpu().numpy().astype(np.uint64).reshape(nb, 256)
            tables = [pkg.sf_build_codes(freq[b]) for b in range(nb)]
        ecap = 3 * bs + 16
        eoff = [b * ecap for b in range(nb)]
        d_e = torch.empty(nb * ecap, dtype=torch.uint8, device=dev)
        d_en = torch.zeros(nb, dtype=torch.int64, device=dev)
        bt.sf_encode(st, d_in, off, n, tables, d_e, eoff, [ecap] * nb, d_en)
        bt.finish(st, nb)
        bt.close()
        return d_e, eoff, [int(x) for x in d_en.cpu().numpy()], tables, ecap

    def module_d(name, d_in, nb, bs, tables=None):
        if not want(name):
            return
        own_tables = tables is None
        d_e, eoff, en, tables, ecap = encode(d_in, nb, bs, tables)
        ooff = [b * bs for b in range(nb)]
        d_o = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        raw = np.frombuffer(b"".join(bytes(t) for t in tables), dtype=np.uint8)
        d_tab = torch.from_numpy(raw.copy()).to(dev)
        d_en = torch.tensor(en, dtype=torch.int64).to(dev)
        d_ns = torch.tensor([bs] * nb, dtype=torch.int64).to(dev)
        bt = pkg.Batch(nb, ecap)
        tarr = bt._tables(tables)
        calls = {
            "host": lambda: bt.sf_decode(st, d_e, eoff, en, tarr, [bs] * nb, d_o, ooff),
            "dev": lambda: bt.sf_decode_dev(st, d_e, eoff, [ecap] * nb, d_en, d_tab, d_ns, d_o, ooff, [bs] * nb),
        }
        if args.entries != "both":
            calls = {args.entries: calls[args.entries]}
        times = {k: [] for k in calls}
        for k in calls:                                   # warm-up (the batch grows here)
            calls[k]()
            bt.finish(st, nb)
        for _ in range(args.reps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                bt.finish(st, nb)
                times[k].append(e0.elapsed_time(e1))
        ok = torch.equal(d_o, d_in[:nb * bs]) if own_tables else None
        bt.close()
        r = {k: stats(v) for k, v in times.items()}
        if len(times) == 2:
            r["dev_over_host"] = round(statistics.median(times["dev"]) / statistics.median(times["host"]), 4)
        r["lmax"] = max(max(bytes(t.len)) for t in tables)
        if ok is not None:
            r["round_trip_ok"] = bool(ok)
        res["module_d"][name] = r
        del d_e, d_o
        torch.cuda.empty_cache()

    bs = 64 << 20
    d_map = torch.from_numpy(pkg.zipf_table(1.2)).to(dev)
    d_in = torch.empty(128 * bs, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(st):
        pkg.gen_bytes(st, 20240601, 0, d_in, 128 * bs, d_map)
    st.synchronize()
    module_d("zipf_128x64M", d_in, 128, bs)
    for nb in (1, 2, 8):
        module_d(f"zipf_{nb}x64M", d_in, nb, bs)
    # F -> T -> C -> D
    for nb in (1, 2, 8, 32) if want("chain") else ():
        off, n = [b * bs for b in range(nb)], [bs] * nb
        ecap = 3 * bs + 16
        eoff = [b * ecap for b in range(nb)]
        d_e = torch.empty(nb * ecap, dtype=torch.uint8, device=dev)
        d_en = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_o = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
        d_tab = torch.zeros(nb * tsz, dtype=torch.uint8, device=dev)
        d_n = torch.tensor(n, dtype=torch.int64).to(dev)
        thb = pkg.tile_hist_bytes(bs)
        thoff = [b * thb for b in range(nb)]
        d_th = torch.zeros(nb * thb, dtype=torch.uint8, device=dev)
        bt = pkg.Batch(nb, ecap)

        def ftc():
            bt.hist256_tiles(st, d_in, off, n, d_freq, d_th, thoff)
            bt.sf_build_codes(st, nb, d_freq, d_tab)
            bt.sf_encode_dev(st, d_in, off, n, d_n, d_tab, d_e, eoff, [ecap] * nb, d_en, d_th, thoff)

        def today():
            ftc()
            bt.finish(st, nb)
            raw = d_tab.cpu().numpy().tobytes()
            tabs = [pkg.CodeTable.from_buffer_copy(raw[b * tsz:(b + 1) * tsz]) for b in range(nb)]
            en = [int(x) for x in d_en.cpu().numpy()]
            bt.sf_decode(st, d_e, eoff, en, tabs, n, d_o, off)
            bt.finish(st, nb)

        def hostfree():
            ftc()
            bt.sf_decode_dev(st, d_e, eoff, [ecap] * nb, d_en, d_tab, d_n, d_o, off, n)
            bt.finish(st, nb)

        times = {"readback": [], "one_sync": []}
        today()
        hostfree()
        for _ in range(args.chain_rounds):
            for k, fn in (("readback", today), ("one_sync", hostfree)):
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        ok = torch.equal(d_o, d_in[:nb * bs])
        bt.close()
        r = {k: stats(v) for k, v in times.items()}
        r["one_sync_over_readback"] = round(statistics.median(times["one_sync"]) / statistics.median(times["readback"]), 4)
        r["round_trip_ok"] = bool(ok)
        res["chain"][f"{nb}x64M"] = r
        del d_e, d_o, d_th
        torch.cuda.empty_cache()
    del d_in
    torch.cuda.empty_cache()

    # uniform bytes: 8/9-bit codes, exact kernels
    d_u = torch.empty(8 * bs, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(st):
        pkg.gen_bytes(st, 77, 0, d_u, 8 * bs, None)
    st.synchronize()
    module_d("uniform_8x64M", d_u, 8, bs)
    # one block whose code has a 33-bit and longer codes: the byte-map list at R = 256
    freq = np.zeros(256, dtype=np.uint64)
    for i in range(40):
        freq[i] = max(1, int(2.0 ** 50 * 0.5 ** i))
    long_tab = pkg.sf_build_codes(freq)
    assert max(bytes(long_tab.len)) > 32
    r = np.frombuffer(d_u[:bs].cpu().numpy().tobytes(), dtype=np.uint8).astype(np.int64)
    d_l = torch.from_numpy(np.minimum((r * r * 40) // (255 * 255 + 1), 39).astype(np.uint8)).to(dev)
    module_d("long33_1x64M", d_l, 1, bs, [long_tab])
    del d_u, d_l
    torch.cuda.empty_cache()
    # run-heavy data, 128 x 8 MiB
    if want("runs_128x8M"):
        bs8 = 8 << 20
        zt = pkg.zipf_table(1.2)
        base = np.concatenate([synth.runs_stream(500 + i, bs8, zt) for i in range(4)])
        d_r = torch.from_numpy(np.tile(base, 32)).to(dev)
        module_d("runs_128x8M", d_r, 128, bs8)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

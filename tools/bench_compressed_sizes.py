"""The size-only chain: the RLE histogram pass (shafa_hipd_rle_encoded_hist_dev, csrc/rle_encode_hist.hip) on resident input
blocks beside its two floors and the only other way to that histogram, and shafa.compressed_sizes against compress_many.
Standalone; HIP events around each kernel row (median, min, max over --reps) on one MI355X.

  python tools/bench_compressed_sizes.py [--reps 7] [--shapes 128x67108864,1000x65536] [--work k64z,k64r,k1mz,k1mr,m8,M128]

Kernel rows, per shape nb x block bytes and content (Zipf(1.2) bytes; run-heavy: synth.runs_stream), ms, GB/s on the input
bytes read and fraction of 8 TB/s:
  hist_pass:   rle_encoded_hist_dev (RLE histogram and size of every block, nothing written but 2 KiB a block);
  size_pass:   rle_encoded_size_dev (the sizes alone);
  hist256:     the plain histogram of the same blocks;
  encode:      rle_encode_tiles of the same blocks into 2 n + 3 regions — the only way to this histogram before the pass.
Driver rows, per workload of tools/bench_compress_many.py: wall clock of compressed_sizes and of compress_many (a
synchronisation per repetition) and each one's peak torch.cuda.max_memory_allocated beyond the input; `same` = every size
equals the length of compress_many's file.  Prints one JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
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


def layout(caps):
    off, pos = [], 0
    for c in caps:
        off.append(pos)
        pos += (c + 15) // 16 * 16
    return off, pos


def rate(nbytes, ms):
    g = nbytes / (statistics.median(ms) / 1e3) / 1e9
    return {"ms": stats(ms), "GB_s": round(g, 1), "peak_frac": round(g * 1e9 / PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="128x67108864,1000x65536")
    ap.add_argument("--work", default="k64z,k64r,k1mz,k1mr,m8,M128")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pkgload
    import bench_compress_many as bcm
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    zt = pkg.zipf_table(1.2)
    d_map = torch.from_numpy(zt).to(dev)
    res = {"kernels": {}, "drivers": {}, "reps": args.reps}

    def content(kind, nb, bs):
        if kind == "zipf":
            d = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
            with torch.cuda.stream(st):
                pkg.gen_bytes(st, 4242, 0, d, nb * bs, d_map)
            st.synchronize()
            return d
        # up to 64 MiB of distinct blocks from the host, repeated on the device (8 GiB: far past every cache)
        uniq = max(1, min(nb, (64 << 20) // bs))
        d_u = torch.from_numpy(synth.runs_stream(99 + nb, uniq * bs, zt)).to(dev).view(uniq, bs)
        return d_u.repeat((nb + uniq - 1) // uniq, 1)[:nb].contiguous().view(-1)

    for shape in [s for s in args.shapes.split(",") if s]:
        nb, bs = (int(x) for x in shape.split("x"))
        for kind in ("zipf", "runs"):
            d_in = content(kind, nb, bs)
            bt = pkg.Batch(nb, 2 * bs + 64)
            ioff, sizes = [b * bs for b in range(nb)], [bs] * nb
            d_n = torch.tensor(sizes, dtype=torch.int64, device=dev)
            row = {"input_bytes": nb * bs}
            d_size = torch.zeros(nb, dtype=torch.int64, device=dev)
            d_hist = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
            ms = timed(torch, st, lambda: bt.rle_encoded_hist_dev(st, d_in, ioff, sizes, d_n, d_size, d_hist), args.reps)
            bt.finish(st, nb)
            row["hist_pass"] = rate(nb * bs, ms)
            d_size2 = torch.zeros(nb, dtype=torch.int64, device=dev)
            ms = timed(torch, st, lambda: bt.rle_encoded_size_dev(st, d_in, ioff, sizes, d_n, d_size2), args.reps)
            bt.finish(st, nb)
            row["size_pass"] = rate(nb * bs, ms)
            d_plain = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
            ms = timed(torch, st, lambda: bt.hist256(st, d_in, ioff, sizes, d_plain), args.reps)
            bt.finish(st, nb)
            row["hist256"] = rate(nb * bs, ms)
            rcap = [2 * bs + 3] * nb
            roff, rtot = layout(rcap)
            d_rle = torch.empty(rtot + 16, dtype=torch.uint8, device=dev)
            d_rn = torch.zeros(nb, dtype=torch.int64, device=dev)
            d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
            thoff, thtot = layout([pkg.tile_hist_bytes(c) for c in rcap])
            d_th = torch.empty(thtot + 16, dtype=torch.uint8, device=dev)
            ms = timed(torch, st, lambda: bt.rle_encode_tiles(st, d_in, ioff, sizes, d_rle, roff, rcap, d_rn, d_freq, d_th, thoff),
                       args.reps)
            bt.finish(st, nb)
            row["encode"] = rate(nb * bs, ms)
            assert torch.equal(d_size, d_rn) and torch.equal(d_size, d_size2), "the passes and the encoder disagree on the sizes"
            assert torch.equal(d_hist, d_freq), "the histogram pass and the encoder disagree"
            row["rle_bytes"] = int(d_rn.sum().item())
            m = lambda k: row[k]["ms"]["median"]                           # noqa: E731
            row["encode_over_hist_pass"] = round(m("encode") / m("hist_pass"), 2)
            row["hist_pass_over_size_pass"] = round(m("hist_pass") / m("size_pass"), 2)
            row["hist_pass_over_hist256"] = round(m("hist_pass") / m("hist256"), 2)
            res["kernels"][f"{shape} {kind}"] = row
            print(shape, kind, json.dumps(row), file=sys.stderr, flush=True)
            bt.close()
            del d_in, d_rle, d_th
            torch.cuda.empty_cache()

    for name in [w for w in args.work.split(",") if w]:
        nf, n, bs, kind = bcm.WORK[name]
        d_in = bcm.make_input(pkg, torch, dev, st, nf * n, kind, 7000 + len(res["drivers"]))
        sizes = [n] * nf
        calls = {"compressed_sizes": lambda: pkg.compressed_sizes(d_in, sizes, bs, stream=st),
                 "compress_many": lambda: pkg.compress_many(d_in, sizes, bs, stream=st)}
        a, b = calls["compressed_sizes"](), calls["compress_many"]()        # warm-up, and the parity check
        same = all(isinstance(x, dict) and x == {k: int(v.numel()) for k, v in y.items()} for x, y in zip(a, b))
        del a, b
        row = {"files": nf, "bytes_per_file": n, "block_size": bs, "content": kind, "same": same}
        for key, fn in calls.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            xs = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                xs.append((time.perf_counter() - t0) * 1e3)
                del out
            peak = torch.cuda.max_memory_allocated() - before
            row[key] = {"ms": stats(xs), "peak_bytes": peak, "peak_over_n": round(peak / (nf * n), 4)}
        row["many_over_sizes"] = round(row["compress_many"]["ms"]["median"] / row["compressed_sizes"]["ms"]["median"], 2)
        res["drivers"][name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
        del d_in
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

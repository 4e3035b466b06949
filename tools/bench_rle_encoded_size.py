"""The RLE encoded-size pass (shafa_hipd_rle_encoded_size_dev, csrc/rle_encode_measure.hip) on resident input blocks, beside
the stage it takes off plain files (rle_encode_tiles into worst-case regions) and the decode-side pass (rle_decoded_size_dev
on the RLE bytes), and the peak device memory of compress_files.  Standalone; HIP events around each device row (median, min,
max over --reps) on one MI355X.

  python tools/bench_rle_encoded_size.py [--reps 7] [--shapes 128x67108864,1000x65536] [--mem-blocks 128] [--tree DIR]

Rows, per shape nb x block bytes and content (Zipf(1.2) bytes; run-heavy: synth.runs_stream):
  size:        the size pass: ms, GB/s on the input bytes read, fraction of 8 TB/s;
  encode:      rle_encode_tiles of the same blocks into 2 n + 3 regions, with its histograms (what compress_files ran before
               it knew the choice);
  decoded:     rle_decoded_size_dev over the RLE bytes of the same blocks (the decode-side size pass).
  memory:      torch.cuda.max_memory_allocated of compress_files beyond its input, on --mem-blocks x 64 MiB at -b M, both
               contents, with the wall clock of the call (median of --reps, a synchronisation each).
--tree: the checkout whose package is loaded (default: this one); a tree without the entry prints the rows it has.
Prints one JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--mem-blocks", type=int, default=128)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "tests"))
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    zt = pkg.zipf_table(1.2)
    d_map = torch.from_numpy(zt).to(dev)
    has = hasattr(pkg.Batch, "rle_encoded_size_dev")
    res = {"tree": os.path.abspath(args.tree), "size_pass": has, "shapes": {}}

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
            rn = d_rn.cpu().tolist()
            row["rle_bytes"] = sum(rn)
            row["encode"] = rate(nb * bs, ms)
            d_size = torch.zeros(nb, dtype=torch.int64, device=dev)
            if has:
                ms = timed(torch, st, lambda: bt.rle_encoded_size_dev(st, d_in, ioff, sizes, d_n, d_size), args.reps)
                bt.finish(st, nb)
                assert d_size.cpu().tolist() == rn, "the size pass and the encoder disagree"
                row["size"] = rate(nb * bs, ms)
                row["encode_over_size"] = round(row["encode"]["ms"]["median"] / row["size"]["ms"]["median"], 2)
            if hasattr(pkg.Batch, "rle_decoded_size_dev"):
                ms = timed(torch, st, lambda: bt.rle_decoded_size_dev(st, d_rle, roff, rn, d_rn, d_size), args.reps)
                bt.finish(st, nb)
                assert d_size.cpu().tolist() == sizes
                row["decoded"] = rate(sum(rn), ms)
            res["shapes"][f"{shape} {kind}"] = row
            bt.close()
            del d_in, d_rle, d_th
            torch.cuda.empty_cache()
    # ---- peak memory and wall clock of compress_files
    if args.mem_blocks > 0:
        res["memory"] = {}
        nb, bs = args.mem_blocks, 64 << 20
        for kind in ("zipf", "runs"):
            d_in = content(kind, nb, bs)
            files = pkg.compress_files(d_in, bs, stream=st)            # warm-up
            key = sorted(files)
            del files
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            xs = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                files = pkg.compress_files(d_in, bs, stream=st)
                torch.cuda.synchronize()
                xs.append((time.perf_counter() - t0) * 1e3)
                del files
            peak = torch.cuda.max_memory_allocated() - before
            res["memory"][kind] = {"input_bytes": nb * bs, "files": key, "peak_bytes": peak, "peak_over_n": round(peak / (nb * bs), 3),
                                   "compress_files_ms": stats(xs)}
            del d_in
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

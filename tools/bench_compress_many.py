"""compress_many (many files in one device batch, shafa-cd_amd/__init__.py) against a loop of compress_files, one call per
file.  Standalone; wall clock with a synchronisation per repetition (both forms synchronise inside anyway); the two forms
alternate within one process, after one warm-up call each.

  python tools/bench_compress_many.py [--reps 7] [--work k64z,k64r,k1mz,k1mr,m8,M128]

Workloads (inputs generated on the device, files back to back in one tensor):
  k64z / k64r:  1 000 x 64 KiB files, Zipf(1.2) / run-heavy, at -b K (one block per file)
  k1mz / k1mr:  1 000 x 1 MiB files, Zipf(1.2) / run-heavy, at -b K (two blocks per file)
  m8:           16 x 8 MiB Zipf(1.2) files at -b m
  M128:         one 8 GiB Zipf(1.2) file at -b M (128 x 64 MiB blocks)
Run-heavy: Zipf(1.2) symbols repeated 1..12 times (RLE is worthwhile).  Per workload: ms per call of both forms (median
[min - max] over the repetitions), the loop's ms per file, the ratio loop / many, and whether every file of compress_many
equals compress_files' byte for byte.  compress_files is compress_many's chain on one file, so that column compares one
file alone (a batch of one, which takes the single-file packs) against the same file among many (the grouping, the
RLE-first order and the segmented packs), not two implementations of the chain; the reference's files anchor both (tests/test_gpu_pack.py, tests/test_gpu_pack_files.py).  Prints one JSON
document.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
K, MB = 655360, 1 << 20

WORK = {                      # name: (files, bytes per file, block size, content)
    "k64z": (1000, 64 << 10, K, "zipf"),
    "k64r": (1000, 64 << 10, K, "runs"),
    "k1mz": (1000, MB, K, "zipf"),
    "k1mr": (1000, MB, K, "runs"),
    "m8": (16, 8 * MB, 8 * MB, "zipf"),
    "M128": (1, 128 * 64 * MB, 64 * MB, "zipf"),
}


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def make_input(pkg, torch, dev, st, total, kind, seed):
    d_map = torch.from_numpy(pkg.zipf_table(1.2)).to(dev)
    if kind == "zipf":
        d = torch.empty(total, dtype=torch.uint8, device=dev)
        pkg.gen_bytes(st, seed, 0, d, total, d_map)
        st.synchronize()
        return d
    sym = torch.empty(total // 4 + 64, dtype=torch.uint8, device=dev)
    rnd = torch.empty(total // 4 + 64, dtype=torch.uint8, device=dev)
    pkg.gen_bytes(st, seed, 0, sym, sym.numel(), d_map)
    pkg.gen_bytes(st, seed + 1, 0, rnd, rnd.numel(), None)
    st.synchronize()
    runs = (rnd.to(torch.int64) % 12) + 1
    d = sym.repeat_interleave(runs)
    while d.numel() < total:
        d = torch.cat([d, d])
    return d[:total].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--work", default=",".join(WORK))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    res = {}
    for name in args.work.split(","):
        nf, n, bs, kind = WORK[name]
        d_in = make_input(pkg, torch, dev, st, nf * n, kind, 7000 + len(res))
        sizes = [n] * nf
        views = [d_in[i * n:(i + 1) * n] for i in range(nf)]

        def many():
            return pkg.compress_many(d_in, sizes, bs, stream=st)

        def loop():
            return [pkg.compress_files(v, bs, stream=st) for v in views]

        a, b = many(), loop()                                           # warm-up, and the parity check
        same = all(isinstance(x, dict) and sorted(x) == sorted(y) and all(torch.equal(x[k], y[k]) for k in y)
                   for x, y in zip(a, b))
        rle = sum(".rle.cod" in y for y in b)
        del a, b
        t_many, t_loop = [], []
        for _ in range(args.reps):
            for fn, acc in ((many, t_many), (loop, t_loop)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
                del out
        res[name] = {"files": nf, "bytes_per_file": n, "block_size": bs, "content": kind, "rle_files": rle,
                     "compress_many_ms": stats(t_many), "compress_files_loop_ms": stats(t_loop),
                     "loop_ms_per_file": round(statistics.median(t_loop) / nf, 4),
                     "loop_over_many": round(statistics.median(t_loop) / statistics.median(t_many), 2),
                     "same_bytes": same}
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
        del d_in, views
        torch.cuda.empty_cache()
    print(json.dumps({"bench_compress_many": res, "reps": args.reps}))


if __name__ == "__main__":
    main()

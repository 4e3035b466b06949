"""decompress_many (many file sets in one device batch, shafa-cd_amd/__init__.py) against a loop of decompress_files, one
call per file set.  Standalone; wall clock with a synchronisation per repetition (both forms synchronise inside anyway); the
two forms alternate within one process, after one warm-up call each.

  python tools/bench_decompress_many.py [--reps 7] [--work k64z,k64r,k1mz,k1mr,m8,M128] [--forms sf,sf_raw,rf]

Workloads (bench_compress_many.py's; the files are made by compress_many):
  k64z / k64r:  1 000 x 64 KiB files, Zipf(1.2) / run-heavy, at -b K (one block per file)
  k1mz / k1mr:  1 000 x 1 MiB files, Zipf(1.2) / run-heavy, at -b K (two blocks per file)
  m8:           16 x 8 MiB Zipf(1.2) files at -b m
  M128:         one 8 GiB Zipf(1.2) file at -b M (128 x 64 MiB blocks)
Forms: sf = shaf + cod, RLE decoded where the file has it (the CLI's `shafa X[.rle].shaf`); sf_raw = shaf + cod without RLE
decoding (`-m d -d s`: the .rle bytes of an RLE file); rf = rle + freq (RLE files only).  Per workload and form: ms per call
of both forms (median [min - max] over the repetitions), the loop's ms per file, the ratio loop / many, and whether every
output of decompress_many equals the loop's byte for byte.  Prints one JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_compress_many import WORK, make_input, stats  # noqa: E402


def entries(sets, form):
    out = []
    for s in sets:
        rle = ".rle.shaf" in s
        k = ".rle" if rle else ""
        if form == "sf":
            out.append(dict(shaf=s[k + ".shaf"], cod=s[k + ".cod"], decode_rle=rle))
        elif form == "sf_raw":
            out.append(dict(shaf=s[k + ".shaf"], cod=s[k + ".cod"], decode_rle=False))
        elif rle:
            out.append(dict(rle=s[".rle"], freq=s[".rle.freq"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--work", default=",".join(WORK))
    ap.add_argument("--forms", default="sf,sf_raw,rf")
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
        sets = pkg.compress_many(d_in, [n] * nf, bs, stream=st)
        del d_in
        assert all(isinstance(s, dict) for s in sets), name
        for form in args.forms.split(","):
            ent = entries(sets, form)
            if not ent:
                continue

            def many():
                return pkg.decompress_many(ent, stream=st)

            def loop():
                return [pkg.decompress_files(**e, stream=st) for e in ent]

            a, b = many(), loop()                                       # warm-up, and the parity check
            same = all(isinstance(x, torch.Tensor) and torch.equal(x, y) for x, y in zip(a, b))
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
            key = f"{name}/{form}"
            res[key] = {"files": len(ent), "bytes_per_file": n, "block_size": bs, "content": kind,
                        "decompress_many_ms": stats(t_many), "decompress_files_loop_ms": stats(t_loop),
                        "loop_ms_per_file": round(statistics.median(t_loop) / len(ent), 4),
                        "loop_over_many": round(statistics.median(t_loop) / statistics.median(t_many), 2),
                        "same_bytes": same}
            print(key, json.dumps(res[key]), file=sys.stderr, flush=True)
        del sets
        torch.cuda.empty_cache()
    print(json.dumps({"bench_decompress_many": res, "reps": args.reps}))


if __name__ == "__main__":
    main()

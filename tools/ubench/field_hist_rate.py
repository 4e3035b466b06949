"""The plane histograms of the quantising split (hist_planes_grid_quant_dev; csrc/planes_lag.hip) on 1 GiB of float32 and of
float64, one block, at the rows of lags (1,), (1, 4096) and (1, 1024, 2^20), each next to the form it replaces, timed
ALTERNATELY with it in one loop.  planes_grid_hist_rate.py's and fields_rate.py's method and field: standalone; one process on one
MI355X; HIP events around one enqueue on a stream (no batch set-up, no synchronisation inside), the median of --reps calls after
--warmup untimed ones.

  python tools/ubench/field_hist_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--sets 1/1,4096/1,1024,1048576]

Legs, per dtype and row of lags:
  hist_quant         two memsets and one launch: the counts from the elements            1 x the tensor's bytes moved
  split_then_hist    split_planes_grid_quant_dev into scratch planes, then hist256 over the planes                        3 x
and one row more, an all-NaN float32 tensor at lags (1,), where EVERY element is an outlier:
  hist_quant         the outliers counted in registers, one atomic a wave at a flush
  split_alone        split_planes_grid_quant_dev alone with a capacity of 0 records: one atomic an element on the block's count
The rate of either leg is the tensor's bytes over the time, so that the forms compare; `ratio` is the other form's median over
the fused median.  No ratio is aimed at: the entry stays for the planes it does not allocate whichever way a row falls.  The
counts of the two forms, and their counts of outliers, are compared before anything is timed.  --lib measures another build of
the library.  One line per pair goes to stderr as it is done.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def hist_legs(torch, pkg, bt, st, args, x, k, lags, abs_error, alone=False):
    dev = x.device
    n = x.numel()
    step, bound = pkg.fields._params("field_hist_rate", abs_error, k)
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    row = (n + 15) // 16 * 16                                              # the planes start at multiples of 16
    planes = torch.empty(k * row, dtype=torch.uint8, device=dev)
    poff = [j * row for j in range(k)]
    fused_f = torch.empty(k * 256, dtype=torch.int64, device=dev)
    two_f = torch.empty(k * 256, dtype=torch.int64, device=dev)
    fused_o = torch.empty(1, dtype=torch.int64, device=dev)
    two_o = torch.empty(1, dtype=torch.int64, device=dev)
    fused = lambda: bt.hist_planes_grid_quant_dev(st, k, [lags], [step], [bound], x, [0], [n], d_n, fused_f, fused_o)
    split = lambda: bt.split_planes_grid_quant_dev(st, k, [lags], [step], [bound], x, [0], [n], d_n, planes, poff, None, [0], [0], two_o)

    def two():
        split()
        bt.hist256(st, planes, poff, [n] * k, two_f)

    fused()
    two()
    bt.finish(st, k)
    if not torch.equal(fused_f, two_f) or not torch.equal(fused_o, two_o) or int(fused_f.sum()) != k * n:
        sys.exit(f"{x.dtype} lags {lags}: the counts of the two forms differ")
    other, name = (split, "split_alone") if alone else (two, "split_then_hist")
    ma, mb = timed_pair(torch, st, fused, other, args.reps, args.warmup)
    legs = {"elements": n, "outliers": int(fused_o[0]), "hist_quant": leg(ma, n * k), name: leg(mb, n * k)}
    legs["hist_quant"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    print(f"{x.dtype} lags {lags}: hist_quant {legs['hist_quant']['ms']['median']} ms, {name} {legs[name]['ms']['median']} ms, "
          f"outliers {legs['outliers']}", file=sys.stderr, flush=True)
    bt.finish(st, k)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--sets", default="1/1,4096/1,1024,1048576")
    ap.add_argument("--abs-error", type=float, default=1e-2)
    args = ap.parse_args()
    sets = [tuple(int(v) for v in s.split(",") if v) for s in args.sets.split("/")]
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    if args.lib:
        pkg.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nbytes = args.mib << 20
    res = {"bytes": nbytes, "reps": args.reps, "warmup": args.warmup, "lib": pkg.LIB_PATH, "run": pkg.PLANES_HIST_RUN,
           "abs_error": args.abs_error, "legs": {}}
    bt = pkg.Batch(8, 1 << 20)
    with torch.cuda.stream(st):
        for name, fty in (("float32", torch.float32), ("float64", torch.float64)):
            k = torch.empty((), dtype=fty).element_size()
            n = nbytes // k
            # fields_rate.py's smooth field of values in +-1000: three waves along the flattened index
            i = torch.arange(n, dtype=torch.float64, device=dev)
            x = (1000 * torch.sin(i / 977) * torch.cos(i / 40961) * torch.sin(i / 1048583 + 0.3)).to(fty)
            del i
            res["legs"][name] = {}
            for lags in sets:
                res["legs"][name][",".join(map(str, lags))] = hist_legs(torch, pkg, bt, st, args, x, k, lags, args.abs_error)
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()
        x = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
        res["legs"]["float32_all_nan"] = {"1": hist_legs(torch, pkg, bt, st, args, x, 4, (1,), args.abs_error, alone=True)}
        del x
    bt.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

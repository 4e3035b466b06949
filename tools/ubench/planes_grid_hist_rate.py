"""The plane histograms of Lorenzo differences (hist_planes_grid_dev; csrc/planes_lag.hip) on 1 GiB of int16 and of int32, one
block, at the rows of lags (), (1,), (1, 4096) and (1, 1024, 2^20), each next to the form it replaces, timed ALTERNATELY with it
in one loop.  planes_grid_rate.py's method: standalone; one process on one MI355X; HIP events around one enqueue on a stream (no
batch set-up, no synchronisation inside), the median of --reps calls after --warmup untimed ones.

  python tools/ubench/planes_grid_hist_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--sets /1/1,4096/1,1024,1048576]

Legs, per dtype and row of lags:
  hist_grid          one memset and one launch: the counts from the elements             1 x the tensor's bytes moved
  split_then_hist    split_planes_grid_dev into scratch planes (split_planes_dev for ()), then hist256 over the planes    3 x
The rate of either leg is the tensor's bytes over the time, so that the forms compare; `ratio` is the two-step median over the
fused median, and the aim is ratio >= 1 in every row (`hist_done` says whether all rows meet it).  The counts of the two forms are
compared with each other, and with torch.bincount over the two-step form's planes, before anything is timed.  --lib measures
another build of the library.  One line per pair goes to stderr as it is done.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def hist_legs(torch, bt, st, args, x, k, lags):
    dev = x.device
    n = x.numel()
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    step = (n + 15) // 16 * 16                                             # the planes start at multiples of 16
    planes = torch.empty(k * step, dtype=torch.uint8, device=dev)
    poff = [j * step for j in range(k)]
    fused_f = torch.empty(k * 256, dtype=torch.int64, device=dev)
    two_f = torch.empty(k * 256, dtype=torch.int64, device=dev)
    fused = lambda: bt.hist_planes_grid_dev(st, k, [lags], x, [0], [n], d_n, fused_f)

    def two():
        if lags:
            bt.split_planes_grid_dev(st, k, [lags], x, [0], [n], d_n, planes, poff)
        else:
            bt.split_planes_dev(st, k, x, [0], [n], d_n, planes, poff)
        bt.hist256(st, planes, poff, [n] * k, two_f)

    fused()
    two()
    bt.finish(st, k)
    want = torch.stack([torch.bincount(planes[poff[j]:poff[j] + n], minlength=256) for j in range(k)]).reshape(-1)
    if not torch.equal(fused_f, two_f) or not torch.equal(two_f, want) or int(fused_f.sum()) != k * n:
        sys.exit(f"lags {lags}: the counts differ")
    ma, mb = timed_pair(torch, st, fused, two, args.reps, args.warmup)
    legs = {"elements": n, "hist_grid": leg(ma, n * k), "split_then_hist": leg(mb, n * k)}
    legs["hist_grid"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    print(f"{x.dtype} lags {lags}: hist_grid {legs['hist_grid']['ms']['median']} ms, split_then_hist "
          f"{legs['split_then_hist']['ms']['median']} ms", file=sys.stderr, flush=True)
    bt.finish(st, k)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--sets", default="/1/1,4096/1,1024,1048576")
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
    res = {"bytes": nbytes, "reps": args.reps, "warmup": args.warmup, "lib": pkg.LIB_PATH, "run": pkg.PLANES_HIST_RUN, "legs": {}}
    bt = pkg.Batch(8, 1 << 20)
    with torch.cuda.stream(st):
        for name, ity in (("int16", torch.int16), ("int32", torch.int32)):
            k = torch.empty((), dtype=ity).element_size()
            # small random values: the high planes of the differences are one byte nearly everywhere, the low ones noise
            x = torch.randint(-300, 301, (nbytes // k,), dtype=ity, device=dev)
            res["legs"][name] = {}
            for lags in sets:
                res["legs"][name][",".join(map(str, lags)) or "plain"] = hist_legs(torch, bt, st, args, x, k, lags)
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()
    bt.close()
    res["hist_done"] = all(r["hist_grid"]["ratio"] >= 1 for d in res["legs"].values() for r in d.values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The byte-plane transposes of lagged differences (split_planes_lag_dev / merge_planes_lag_dev; csrc/planes_lag.hip) on 1 GiB of
int16 and of int32, one block, at lags 3, 64, 4096 and 2^20 (the size rounded down to a multiple of the lag), each next to what
a user has without them, timed ALTERNATELY with it in one loop.  Standalone; one process on one MI355X; HIP events around one
enqueue on a stream (no batch set-up, no synchronisation inside), the median of --reps calls after --warmup untimed ones.

  python tools/ubench/planes_lag_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--lags 3,64,4096,1048576]
                                          [--slow-ms 250] [--slow-reps 3] [--slow-warmup 1]

Legs, per dtype and lag:
  split_lag          one launch: planes of the folded differences at the lag            2 x the tensor's bytes moved
  sub_then_split     out = t.clone(); out[lag:] -= t[:-lag]; then split_planes_dev       6 x
  merge_lag          up to three launches: the column prefix sums of the unfolded planes 3 x (the planes are read twice)
  merge_then_cumsum  merge_planes_dev, then view(R, lag).cumsum(0, dtype=..., out=...)    4 x
torch's side leaves the zigzag fold out, which favours it.  The rate of all four is the fused job's bytes, 3 x the tensor's,
over the time, so that the forms compare; `ratio` is the two-step median over the fused median, and the condition is
ratio >= 1 in every row (`lag_done`).  For the record, lag 1 against the _diff_dev entries, alternately: `vs_diff` is the lag
entry's median over the diff entry's.  Every answer is checked against the torch expression before it is timed.  --lib measures
another build of the library.
A SLOW PAIR: torch's cumsum(0) over a [n / lag, lag] view with few columns takes seconds a call (22 s at lag 3 on 1 GiB of
int16), and 20 + 3 of them would be ten minutes a row.  Each two-step form is therefore timed once while it is checked, and a pair whose
two-step call took more than --slow-ms is measured with --slow-reps after --slow-warmup instead; every pair's `reps` and
`warmup` are in its fused leg, and `slow_pairs` lists those that were cut.  A plain run at the defaults is DESIGN 7.26's table:
there the merge pairs at lags 3 and 64 are medians of 3 after 1, everything else of 20 after 3.  One line per pair goes to stderr
as it is done.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def lag_legs(torch, bt, st, args, x, k, lag):
    """the four legs at one lag on the first multiple-of-lag elements of x"""
    ity = {2: torch.int16, 4: torch.int32}[k]
    dev = x.device
    n = x.numel() // lag * lag
    xi = x[:n]
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    step = (n + 15) // 16 * 16                                             # the planes start at multiples of 16
    planes = torch.empty(k * step, dtype=torch.uint8, device=dev)
    rows = planes.view(k, step)[:, :n]
    back, other = torch.empty_like(xi), torch.empty_like(xi)
    poff = [j * step for j in range(k)]
    split_l = lambda: bt.split_planes_lag_dev(st, k, [lag], xi, [0], [n], d_n, planes, poff)
    merge_l = lambda: bt.merge_planes_lag_dev(st, k, [lag], planes, poff, [n], d_n, back, [0])

    def sub():
        out = xi.clone()
        out[lag:] -= xi[:-lag]
        return out

    def two_split():
        bt.split_planes_dev(st, k, sub(), [0], [n], d_n, planes, poff)

    def two_merge():
        bt.merge_planes_dev(st, k, planes, poff, [n], d_n, back, [0])
        torch.cumsum(back.view(n // lag, lag), 0, dtype=ity, out=other.view(n // lag, lag))

    d = sub()
    want = ((d << 1) ^ (d >> (8 * k - 1))).view(torch.uint8).reshape(-1, k).t().contiguous()
    split_l()
    bt.finish(st, 1)
    ok = torch.equal(rows, want)
    back.zero_()
    merge_l()
    bt.finish(st, 1)
    ok = ok and torch.equal(back, xi)
    del want
    once = {}
    for name, fn in (("sub_then_split", two_split), ("merge_then_cumsum", two_merge)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        bt.finish(st, 1)
        once[name] = a.elapsed_time(b)
        if name == "sub_then_split":
            ok = ok and torch.equal(rows, d.view(torch.uint8).reshape(-1, k).t().contiguous())
    if not ok or not torch.equal(other, xi):
        sys.exit(f"lag {lag}: the legs differ from the torch expression")
    del d
    split_l()                                                              # the fused merge reads the fused split's planes
    legs = {"elements": n}
    for fused, two, fa, fb in (("split_lag", "sub_then_split", split_l, two_split),
                               ("merge_lag", "merge_then_cumsum", merge_l, two_merge)):
        if fused == "merge_lag":
            split_l()
        slow = once[two] > args.slow_ms
        reps, warmup = (args.slow_reps, args.slow_warmup) if slow else (args.reps, args.warmup)
        ma, mb = timed_pair(torch, st, fa, fb, reps, warmup)
        legs[fused], legs[two] = leg(ma, 3 * n * k), leg(mb, 3 * n * k)
        legs[fused]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
        legs[fused].update(reps=reps, warmup=warmup, slow_pair=slow)
        print(f"{xi.dtype} lag {lag}: {fused} {legs[fused]['ms']['median']} ms, {two} {legs[two]['ms']['median']} ms ({reps} after {warmup})",
              file=sys.stderr, flush=True)
    if lag == 1:
        split_d = lambda: bt.split_planes_diff_dev(st, k, xi, [0], [n], d_n, planes, poff)
        merge_d = lambda: bt.merge_planes_diff_dev(st, k, planes, poff, [n], d_n, back, [0])
        for ours, theirs, fa, fb in (("split_lag", "split_diff", split_l, split_d),
                                     ("merge_lag", "merge_diff", merge_l, merge_d)):
            ma, mb = timed_pair(torch, st, fa, fb, args.reps, args.warmup)
            legs[theirs] = leg(mb, 3 * n * k)
            legs[ours]["vs_diff"] = round(statistics.median(ma) / statistics.median(mb), 3)
    bt.finish(st, 1)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--lags", default="3,64,4096,1048576")
    ap.add_argument("--slow-ms", type=float, default=250.0)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--slow-warmup", type=int, default=1)
    args = ap.parse_args()
    lags = [int(v) for v in args.lags.split(",")]
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    if args.lib:
        pkg.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nbytes = args.mib << 20
    res = {"bytes": nbytes, "reps": args.reps, "warmup": args.warmup, "lib": pkg.LIB_PATH, "legs": {}}
    bt = pkg.Batch(1, 1 << 20)
    with torch.cuda.stream(st):
        for name, ity in (("int16", torch.int16), ("int32", torch.int32)):
            k = torch.empty((), dtype=ity).element_size()
            n = nbytes // k
            # small random values: neither side's work depends on them
            x = torch.randint(-300, 301, (n,), dtype=ity, device=dev)
            res["legs"][name] = {}
            for lag in [1] + lags:
                res["legs"][name][str(lag)] = lag_legs(torch, bt, st, args, x, k, lag)
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()
    bt.close()
    res["slow_pairs"] = [f"{d} lag {g} {f}" for d in res["legs"] for g in res["legs"][d] for f in ("split_lag", "merge_lag")
                         if res["legs"][d][g][f]["slow_pair"]]
    res["lag_done"] = all(res["legs"][d][str(g)][f]["ratio"] >= 1 for d in res["legs"] for g in lags for f in ("split_lag", "merge_lag"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

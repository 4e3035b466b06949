"""The byte-plane transposes of Lorenzo differences (split_planes_grid_dev / merge_planes_grid_dev; csrc/planes_lag.hip) on 1 GiB
of int16 and of int32, one block, at the lag sets (1, 4096), (3, 3072) and (1, 1024, 2^20) (the size rounded down to a multiple of
every lag), each next to what a user has without them, timed ALTERNATELY with it in one loop.  planes_lag_rate.py's method:
standalone; one process on one MI355X; HIP events around one enqueue on a stream (no batch set-up, no synchronisation inside), the
median of --reps calls after --warmup untimed ones.

  python tools/ubench/planes_grid_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--sets 1,4096/3,3072/1,1024,1048576]
                                           [--slow-ms 250] [--slow-reps 3] [--slow-warmup 1]

Legs, per dtype and lag set of k lags:
  split_grid         one launch: planes of the folded differences along all lags        2 x the tensor's bytes moved
  sub_then_split     out = t.clone(); out[L:] -= t[:-L]; per further lag torch.sub(out[L:], out[:-L]) into a fresh buffer (the
                     ranges overlap); then split_planes_dev                              2 + 3 k + 2 x
  merge_grid         the first pass from the planes, one pass in place per further lag   3 k x at the most
  merge_then_cumsum  merge_planes_dev, then view(R, L).cumsum(0, dtype=..., out=...) per lag                2 + 2 k x
  one_lag_merges     the existing one-lag merges at each of the set's lags back to back, merge_planes_diff_dev for lag 1 and
                     merge_planes_lag_dev for the others (every one from the planes: the work of k merges, not their result)
torch's side leaves the zigzag fold out, which favours it.  The rate of every leg is the fused split's bytes, 2 x the tensor's,
over the time, so that the forms compare; `ratio` is the two-step median over the fused median, and the aim is ratio >= 1 in
every row; `vs_one_lag` is merge_grid's median over one_lag_merges', and the aim is <= 1.10 (`grid_done` says whether all rows
meet both).  Every answer is checked against the torch expression before it is timed.  --lib measures another build of the library.
A SLOW PAIR is cut as in planes_lag_rate.py: each two-step form is timed once while it is checked, and a pair whose two-step call
took more than --slow-ms is measured with --slow-reps after --slow-warmup instead; `slow_pairs` lists them.  One line per pair
goes to stderr as it is done.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def grid_legs(torch, bt, st, args, x, k, lags):
    """the five legs at one lag set on the first elements of x that are a multiple of every lag"""
    import math
    ity = {2: torch.int16, 4: torch.int32}[k]
    dev = x.device
    unit = math.lcm(*lags)
    n = x.numel() // unit * unit
    xi = x[:n]
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    step = (n + 15) // 16 * 16                                             # the planes start at multiples of 16
    planes = torch.empty(k * step, dtype=torch.uint8, device=dev)
    rows = planes.view(k, step)[:, :n]
    back, other = torch.empty_like(xi), torch.empty_like(xi)
    poff = [j * step for j in range(k)]
    split_g = lambda: bt.split_planes_grid_dev(st, k, [lags], xi, [0], [n], d_n, planes, poff)
    merge_g = lambda: bt.merge_planes_grid_dev(st, k, [lags], planes, poff, [n], d_n, back, [0])

    def sub():
        cur = xi.clone()
        cur[lags[0]:] -= xi[:-lags[0]]
        for lag in lags[1:]:                                               # into another buffer: the two ranges overlap
            nxt = torch.empty_like(cur)
            nxt[:lag] = cur[:lag]
            torch.sub(cur[lag:], cur[:-lag], out=nxt[lag:])
            cur = nxt
        return cur

    def two_split():
        bt.split_planes_dev(st, k, sub(), [0], [n], d_n, planes, poff)

    def two_merge():
        """-> the buffer the result is in"""
        bt.merge_planes_dev(st, k, planes, poff, [n], d_n, back, [0])
        src, dst = back, other
        for lag in lags:
            torch.cumsum(src.view(n // lag, lag), 0, dtype=ity, out=dst.view(n // lag, lag))
            src, dst = dst, src
        return src

    def one_lag():
        for lag in lags:
            if lag == 1:
                bt.merge_planes_diff_dev(st, k, planes, poff, [n], d_n, back, [0])
            else:
                bt.merge_planes_lag_dev(st, k, [lag], planes, poff, [n], d_n, back, [0])

    d = sub()
    want = ((d << 1) ^ (d >> (8 * k - 1))).view(torch.uint8).reshape(-1, k).t().contiguous()
    split_g()
    bt.finish(st, 1)
    ok = torch.equal(rows, want)
    back.zero_()
    merge_g()
    bt.finish(st, 1)
    ok = ok and torch.equal(back, xi)
    del want
    once = {}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    two_split()
    b.record(st)
    bt.finish(st, 1)
    once["sub_then_split"] = a.elapsed_time(b)
    ok = ok and torch.equal(rows, d.view(torch.uint8).reshape(-1, k).t().contiguous())
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    got = two_merge()
    b.record(st)
    bt.finish(st, 1)
    once["merge_then_cumsum"] = a.elapsed_time(b)
    if not ok or not torch.equal(got, xi):
        sys.exit(f"lags {lags}: the legs differ from the torch expression")
    del d
    legs = {"elements": n}
    tag = f"{xi.dtype} lags {lags}"
    for fused, two, fa, fb in (("split_grid", "sub_then_split", split_g, two_split),
                               ("merge_grid", "merge_then_cumsum", merge_g, two_merge)):
        split_g()                                                          # the merges read the fused split's planes
        slow = once[two] > args.slow_ms
        reps, warmup = (args.slow_reps, args.slow_warmup) if slow else (args.reps, args.warmup)
        ma, mb = timed_pair(torch, st, fa, fb, reps, warmup)
        legs[fused], legs[two] = leg(ma, 2 * n * k), leg(mb, 2 * n * k)
        legs[fused]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
        legs[fused].update(reps=reps, warmup=warmup, slow_pair=slow)
        print(f"{tag}: {fused} {legs[fused]['ms']['median']} ms, {two} {legs[two]['ms']['median']} ms ({reps} after {warmup})",
              file=sys.stderr, flush=True)
    split_g()
    ma, mb = timed_pair(torch, st, merge_g, one_lag, args.reps, args.warmup)
    legs["one_lag_merges"] = leg(mb, 2 * n * k)
    legs["merge_grid"]["vs_one_lag"] = round(statistics.median(ma) / statistics.median(mb), 3)
    legs["merge_grid"]["ms_next_to_one_lag"] = round(statistics.median(ma), 4)
    print(f"{tag}: merge_grid {statistics.median(ma):.4f} ms, one_lag_merges {legs['one_lag_merges']['ms']['median']} ms",
          file=sys.stderr, flush=True)
    bt.finish(st, 1)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--sets", default="1,4096/3,3072/1,1024,1048576")
    ap.add_argument("--slow-ms", type=float, default=250.0)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--slow-warmup", type=int, default=1)
    args = ap.parse_args()
    sets = [tuple(int(v) for v in s.split(",")) for s in args.sets.split("/")]
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
            for lags in sets:
                res["legs"][name][",".join(map(str, lags))] = grid_legs(torch, bt, st, args, x, k, lags)
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()
    bt.close()
    rows = [(d, g, res["legs"][d][g]) for d in res["legs"] for g in res["legs"][d]]
    res["slow_pairs"] = [f"{d} lags {g} {f}" for d, g, r in rows for f in ("split_grid", "merge_grid") if r[f]["slow_pair"]]
    res["grid_done"] = all(r["split_grid"]["ratio"] >= 1 and r["merge_grid"]["ratio"] >= 1 and r["merge_grid"]["vs_one_lag"] <= 1.10
                           for _, _, r in rows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

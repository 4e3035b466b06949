"""The rounding entries (split_planes_grid_round_dev / merge_planes_grid_round_dev / hist_planes_grid_round_dev;
csrc/planes_lag.hip) on 1 GiB of bfloat16, of float32 and of float64, one block, at the rows of lags (1,), (1, 4096) and
(1, 1024, 2^20), each next to the form it replaces, timed ALTERNATELY with it in one loop.  fields_rate.py's method and field:
standalone; one process on one MI355X; HIP events around one enqueue on a stream (no batch set-up, no synchronisation inside), the
median of --reps calls after --warmup untimed ones.

  python tools/ubench/rounded_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--sets 1/1,4096/1,1024,1048576]

Legs, per dtype and row of lags:
  split_round          the rounding split: codes in registers, no temporary
  round_then_split     torch integer ops (mask, add, shift, where, negate) that write the codes into a temporary as large as the
                       tensor, then split_planes_grid_dev
  merge_round          the grid merge's chain, the restore pass in place, the patch pass over the tensor's outliers
  merge_then_shift     merge_planes_grid_dev into an integer temporary, then torch integer ops (abs, shift, mask, or) into the result
  hist_round           two memsets and one launch: the counts from the elements
  split_then_hist      split_planes_grid_round_dev into scratch planes, then hist256 over the planes
The rate of every leg is the tensor's bytes over the time, so that the forms compare; `ratio` is the other form's median over the
fused median.  No ratio is aimed at: the fused forms stay for the temporary they save whichever way a row falls.  The planes of
the two split forms, the tensors of the two merge forms (but for the outliers, which come back as the original's bits) and the
counts of the two hist forms are compared before anything is timed.  --lib measures another build of the library.  One line per
row goes to stderr as it is done.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def torch_codes(torch, xi, W, mant, keep, out):
    """the rule of include/shafa_hip.h, "Point-wise relative bounds", in torch integer ops on the elements' bits xi -> out"""
    d = mant - keep
    mag, inf = (1 << (W - 1)) - 1, ((1 << (W - 1 - mant)) - 1) << mant
    m = xi & mag
    rn = (m + ((1 << (d - 1)) - 1) + ((m >> d) & 1)) >> d if d else m
    r = torch.where(m >= inf, m >> d, rn)
    out.copy_(torch.where(xi < 0, -r, r))


def torch_values(torch, codes, W, mant, keep, out):
    """what the merge makes of the codes, in torch integer ops -> out (the result's bits)"""
    d = mant - keep
    mp = (codes.abs() << d) & ((1 << (W - 1)) - 1)
    out.copy_(torch.where(codes < 0, mp | (-1 << (W - 1)), mp))


def rounded_legs(torch, pkg, bt, st, args, x, k, mant, keep, lags):
    dev = x.device
    n, W = x.numel(), 8 * k
    ity = {2: torch.int16, 4: torch.int32, 8: torch.int64}[k]
    xi = x.view(ity)
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    row = (n + 15) // 16 * 16                                              # the planes start at multiples of 16
    planes = torch.empty(k * row, dtype=torch.uint8, device=dev)
    planes2 = torch.empty(k * row, dtype=torch.uint8, device=dev)
    poff = [j * row for j in range(k)]
    cap = pkg.fields.outlier_capacity(n)
    d_outl = torch.empty(2 * cap, dtype=torch.int64, device=dev)
    d_found = torch.zeros(1, dtype=torch.int64, device=dev)
    codes = torch.empty(n, dtype=ity, device=dev)
    back, back2 = torch.empty_like(x), torch.empty_like(x)
    fused = lambda: bt.split_planes_grid_round_dev(st, k, [lags], [mant], [keep], x, [0], [n], d_n, planes, poff, d_outl, [0], [cap],
                                                   d_found)

    def two():
        torch_codes(torch, xi, W, mant, keep, codes)                       # the temporary
        bt.split_planes_grid_dev(st, k, [lags], codes, [0], [n], d_n, planes2, poff)

    fused()
    two()
    bt.finish(st, 1)
    found = int(d_found[0])
    if found > cap or not torch.equal(planes, planes2):
        sys.exit(f"{x.dtype} lags {lags}: the planes of the two forms differ, or the tensor has more outliers than records ({found})")
    ma, mb = timed_pair(torch, st, fused, two, args.reps, args.warmup)
    legs = {"elements": n, "outliers": found, "keep": keep, "split_round": leg(ma, n * k), "round_then_split": leg(mb, n * k)}
    legs["split_round"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    bt.finish(st, 1)
    fused()                                                                # the records of the last split, all of them
    m_fused = lambda: bt.merge_planes_grid_round_dev(st, k, [lags], [mant], [keep], planes, poff, [n], d_n, d_outl, [0], [found],
                                                     back, [0])

    def m_two():
        bt.merge_planes_grid_dev(st, k, [lags], planes, poff, [n], d_n, codes, [0])
        torch_values(torch, codes, W, mant, keep, back2.view(ity))

    m_fused()
    m_two()
    bt.finish(st, 1)
    good = torch.ones(n, dtype=torch.bool, device=dev)
    good[d_outl[0:2 * found:2]] = False                                    # an outlier is the original's bits
    if not torch.equal(back.view(ity)[good], back2.view(ity)[good]) or not torch.equal(back.view(ity)[~good], xi[~good]):
        sys.exit(f"{x.dtype} lags {lags}: the tensors of the two merge forms differ")
    del good
    ma, mb = timed_pair(torch, st, m_fused, m_two, args.reps, args.warmup)
    legs["merge_round"], legs["merge_then_shift"] = leg(ma, n * k), leg(mb, n * k)
    legs["merge_round"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    bt.finish(st, 1)
    del back, back2, codes, planes2
    torch.cuda.empty_cache()
    # the histograms without the planes against the split and hist256 over its planes
    fused_f = torch.empty(k * 256, dtype=torch.int64, device=dev)
    two_f = torch.empty(k * 256, dtype=torch.int64, device=dev)
    fused_o = torch.empty(1, dtype=torch.int64, device=dev)
    two_o = torch.empty(1, dtype=torch.int64, device=dev)
    h_fused = lambda: bt.hist_planes_grid_round_dev(st, k, [lags], [mant], [keep], x, [0], [n], d_n, fused_f, fused_o)

    def h_two():
        bt.split_planes_grid_round_dev(st, k, [lags], [mant], [keep], x, [0], [n], d_n, planes, poff, None, [0], [0], two_o)
        bt.hist256(st, planes, poff, [n] * k, two_f)

    h_fused()
    h_two()
    bt.finish(st, k)
    if not torch.equal(fused_f, two_f) or not torch.equal(fused_o, two_o) or int(fused_f.sum()) != k * n:
        sys.exit(f"{x.dtype} lags {lags}: the counts of the two hist forms differ")
    ma, mb = timed_pair(torch, st, h_fused, h_two, args.reps, args.warmup)
    legs["hist_round"], legs["split_then_hist"] = leg(ma, n * k), leg(mb, n * k)
    legs["hist_round"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    bt.finish(st, k)
    print(f"{x.dtype} keep {keep} lags {lags}: split_round {legs['split_round']['ms']['median']} ms, round_then_split "
          f"{legs['round_then_split']['ms']['median']} ms; merge_round {legs['merge_round']['ms']['median']} ms, merge_then_shift "
          f"{legs['merge_then_shift']['ms']['median']} ms; hist_round {legs['hist_round']['ms']['median']} ms, split_then_hist "
          f"{legs['split_then_hist']['ms']['median']} ms; outliers {found}", file=sys.stderr, flush=True)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--sets", default="1/1,4096/1,1024,1048576")
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
    res = {"bytes": nbytes, "reps": args.reps, "warmup": args.warmup, "lib": pkg.LIB_PATH, "legs": {}}
    bt = pkg.Batch(8, 1 << 20)
    with torch.cuda.stream(st):
        for name, fty, keep in (("bfloat16", torch.bfloat16, 3), ("float32", torch.float32, 10), ("float64", torch.float64, 10)):
            k, mant = torch.empty((), dtype=fty).element_size(), pkg.MANTISSA_BITS[fty]
            n = nbytes // k
            # fields_rate.py's smooth field of values in +-1000: three waves along the flattened index, made in pieces
            x = torch.empty(n, dtype=fty, device=dev)
            piece = 1 << 26
            for lo in range(0, n, piece):
                i = torch.arange(lo, min(n, lo + piece), dtype=torch.float64, device=dev)
                x[lo:lo + piece] = (1000 * torch.sin(i / 977) * torch.cos(i / 40961) * torch.sin(i / 1048583 + 0.3)).to(fty)
                del i
            res["legs"][name] = {}
            for lags in sets:
                res["legs"][name][",".join(map(str, lags))] = rounded_legs(torch, pkg, bt, st, args, x, k, mant, keep, lags)
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()
    bt.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

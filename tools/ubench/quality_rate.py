"""The error entries (error_dev / error_quant_dev / error_round_dev; csrc/planes_lag.hip) on 1 GiB of bfloat16, of
float32 and of float64, one block, each next to the form it replaces, timed ALTERNATELY with it in one loop.  rounded_rate.py's
method and field: standalone; one process on one MI355X; HIP events around one enqueue on a stream (no batch set-up, no
synchronisation inside), the median of --reps calls after --warmup untimed ones.

  python tools/ubench/quality_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH]

Legs, per dtype:
  error_round          the fused entry under the rounding rule: what comes back is made in registers
  round_merge_reduce   split_planes_grid_round_dev into scratch planes, merge_planes_grid_round_dev into a second tensor, then the
                       torch reductions in float64 (sub, square().sum(), abs().max(), min, max, isfinite().sum())
  error_quant          the fused entry under the quantising rule (float32 and float64)
  quant_merge_reduce   the same three steps with the quantising pair
  error_dev            the two-tensor entry over the merge's output and the original
  reduce               those torch reductions alone
  error_*_64           the fused entries and error_dev over the same bytes cut into 64 blocks: 64 workgroups fold the partials, so
                       (one block) - (64 blocks) is what ONE workgroup folding every partial of the tensor costs
The rate of every leg is the tensor's bytes over the time, so that the forms compare; `ratio` is the other form's median over the
entry's median.  No ratio is aimed at: the requirement is only that the entry is not slower.  The records of the fused entry and
of error_dev over the merge's output are compared first (words 0 - 3 and 6 - 11 bit for bit), and torch's numbers against them.
--lib measures another build of the library.  One line per dtype goes to stderr as it is done.  Prints one JSON document."""
import argparse
import json
import math
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def reductions(torch, x, y):
    """what a caller without the entries runs: six reductions with float64 temporaries larger than the tensor"""
    xd = x.double()
    e = xd.sub(y.double())
    return e.square().sum(), e.abs().max(), xd.min(), xd.max(), torch.isfinite(e).sum(), xd.square().sum()


def words(d_stat):
    return [int(v) & ((1 << 64) - 1) for v in d_stat.cpu().view(-1).tolist()]


def dbl(w):
    return struct.unpack("<d", struct.pack("<Q", w))[0]


def legs_of(torch, pkg, bt, st, args, x, k, mant, keep, abs_error):
    dev = x.device
    n = x.numel()
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    row = (n + 15) // 16 * 16
    planes = torch.empty(k * row, dtype=torch.uint8, device=dev)
    poff = [j * row for j in range(k)]
    cap = pkg.fields.outlier_capacity(n)
    d_outl = torch.empty(2 * cap, dtype=torch.int64, device=dev)
    d_found = torch.zeros(1, dtype=torch.int64, device=dev)
    back = torch.empty_like(x)
    stat, stat2 = torch.empty(12, dtype=torch.int64, device=dev), torch.empty(12, dtype=torch.int64, device=dev)
    nb = 64
    cut = n // nb // 16 * 16                                               # 64 blocks at multiples of 16 bytes
    off64, n64 = [b * cut * k for b in range(nb)], [cut] * (nb - 1) + [n - cut * (nb - 1)]
    d_n64 = torch.tensor(n64, dtype=torch.int64, device=dev)
    stat64 = torch.empty(12 * nb, dtype=torch.int64, device=dev)
    lags = (1,)
    out = {"elements": n}
    rules = [("round", dict(keep=keep))]
    if k != 2:
        step, bound = pkg.fields._params("quality_rate", abs_error, k)
        rules.append(("quant", dict(step=step, bound=bound)))
    for rule, p in rules:
        if rule == "round":
            fused = lambda: bt.error_round_dev(st, k, [mant], [keep], x, [0], [n], d_n, stat)
            fused64 = lambda: bt.error_round_dev(st, k, [mant] * nb, [keep] * nb, x, off64, n64, d_n64, stat64)
            split = lambda: bt.split_planes_grid_round_dev(st, k, [lags], [mant], [keep], x, [0], [n], d_n, planes, poff, d_outl, [0],
                                                           [cap], d_found)
            merge = lambda found: bt.merge_planes_grid_round_dev(st, k, [lags], [mant], [keep], planes, poff, [n], d_n, d_outl, [0],
                                                                 [found], back, [0])
        else:
            fused = lambda: bt.error_quant_dev(st, k, [p["step"]], [p["bound"]], x, [0], [n], d_n, stat)
            fused64 = lambda: bt.error_quant_dev(st, k, [p["step"]] * nb, [p["bound"]] * nb, x, off64, n64, d_n64, stat64)
            split = lambda: bt.split_planes_grid_quant_dev(st, k, [lags], [p["step"]], [p["bound"]], x, [0], [n], d_n, planes, poff,
                                                           d_outl, [0], [cap], d_found)
            merge = lambda found: bt.merge_planes_grid_quant_dev(st, k, [lags], [p["step"]], planes, poff, [n], d_n, d_outl, [0],
                                                                 [found], back, [0])
        split()
        bt.finish(st, 1)
        found = int(d_found[0])
        if found > cap:
            sys.exit(f"{x.dtype} {rule}: more outliers than records ({found})")

        def two():
            split()
            merge(found)
            return reductions(torch, x, back)

        pair = lambda: bt.error_dev(st, k, [mant], [math.inf], [0.0], back, [0], [n], d_n, x, [0], stat2)
        pair64 = lambda: bt.error_dev(st, k, [mant] * nb, [math.inf] * nb, [0.0] * nb, back, off64, n64, d_n64, x, off64, stat64)
        fused()
        ref = two()
        pair()
        bt.finish(st, 1)
        a, b = words(stat), words(stat2)
        if any(a[i] != b[i] for i in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11)) or a[4] != found:
            sys.exit(f"{x.dtype} {rule}: the records of the fused entry and of error_dev differ: {a} {b}")
        se2, emax, lo, hi, fin, sx2 = (float(v) for v in ref)
        for got, want in ((dbl(a[6]), se2), (dbl(a[8]), emax), (dbl(a[10]), lo), (dbl(a[11]), hi), (float(a[1]), fin), (dbl(a[7]), sx2)):
            if abs(got - want) > 1e-9 * abs(want):
                sys.exit(f"{x.dtype} {rule}: the record and torch's reductions differ: {got!r} {want!r}")
        s = pkg.ErrorStats(a)
        ma, mb = timed_pair(torch, st, fused, two, args.reps, args.warmup)
        out[f"error_{rule}"], out[f"{rule}_merge_reduce"] = leg(ma, n * k), leg(mb, n * k)
        out[f"error_{rule}"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
        out[f"error_{rule}"].update(psnr=round(s.psnr, 2), snr=round(s.snr, 2), outliers=found)
        mc, _ = timed_pair(torch, st, fused64, fused, args.reps, args.warmup)
        out[f"error_{rule}_64"] = leg(mc, n * k)
        bt.finish(st, nb)
        if rule == "round":                                                # the two-tensor entry against the reductions alone
            ma, mb = timed_pair(torch, st, pair, lambda: reductions(torch, x, back), args.reps, args.warmup)
            out["error_dev"], out["reduce"] = leg(ma, 2 * n * k), leg(mb, 2 * n * k)
            out["error_dev"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
            mc, _ = timed_pair(torch, st, pair64, pair, args.reps, args.warmup)
            out["error_dev_64"] = leg(mc, 2 * n * k)
            bt.finish(st, nb)
        torch.cuda.empty_cache()
    print(f"{x.dtype}: " + "; ".join(f"{name} {v['ms']['median']} ms" + (f" (x{v['ratio']})" if "ratio" in v else "")
                                     for name, v in out.items() if isinstance(v, dict)), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
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
    bt = pkg.Batch(64, 1 << 20)
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
            res["legs"][name] = legs_of(torch, pkg, bt, st, args, x, k, mant, keep, 1e-2)
            del x
            torch.cuda.empty_cache()
    bt.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

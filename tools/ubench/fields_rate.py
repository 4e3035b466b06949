"""The error-bounded field entries (split_planes_grid_quant_dev / merge_planes_grid_quant_dev; csrc/planes_lag.hip) on 1 GiB of
float32 and of float64, one block, at the rows of lags (1,), (1, 4096) and (1, 1024, 2^20), each next to the form it replaces,
timed ALTERNATELY with it in one loop.  planes_grid_hist_rate.py's method: standalone; one process on one MI355X; HIP events
around one enqueue on a stream (no batch set-up, no synchronisation inside), the median of --reps calls after --warmup untimed
ones.

  python tools/ubench/fields_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--sets 1/1,4096/1,1024,1048576]

Legs, per dtype and row of lags:
  split_quant          the quantising split: codes in registers, no temporary
  quant_then_split     torch.round(x * inv) (half to even) cast to the integer type into a temporary as large as the field, then split_planes_grid_dev
  merge_quant          the grid merge's chain, the restore pass in place, the patch pass over the field's few outliers
  merge_then_scale     merge_planes_grid_dev into an integer temporary, then a torch multiply by the step into the result
The rate of every leg is the tensor's bytes over the time, so that the forms compare; `ratio` is the two-step median over the fused
median.  No ratio is aimed at: the fused split quantises up to eight units per unit stored, and it stays for the temporary it
saves whichever way the ratio falls.  The planes of the two split forms and the tensors of the two merge forms (but for the
outliers, which come back as the original's bits) are compared, and the bound is checked, before anything is timed.  --lib measures another build of the library.  One line per pair goes to
stderr as it is done.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from planes_rate import leg, timed_pair  # noqa: E402


def field_legs(torch, pkg, bt, st, args, x, k, lags, abs_error):
    dev = x.device
    n = x.numel()
    ity = torch.int32 if k == 4 else torch.int64
    step, bound = pkg.fields._params("fields_rate", abs_error, k)
    inv = pkg.fields._inverse(step, k)
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
    fused = lambda: bt.split_planes_grid_quant_dev(st, k, [lags], [step], [bound], x, [0], [n], d_n, planes, poff, d_outl, [0], [cap],
                                                   d_found)

    def two():
        codes.copy_(torch.round(x * inv))                                  # the cast into the temporary
        bt.split_planes_grid_dev(st, k, [lags], codes, [0], [n], d_n, planes2, poff)

    fused()
    two()
    bt.finish(st, 1)
    found = int(d_found[0])
    if found > cap or not torch.equal(planes, planes2):
        sys.exit(f"{x.dtype} lags {lags}: the planes of the two forms differ, or the field has more outliers than records ({found})")
    ma, mb = timed_pair(torch, st, fused, two, args.reps, args.warmup)
    legs = {"elements": n, "outliers": found, "split_quant": leg(ma, n * k), "quant_then_split": leg(mb, n * k)}
    legs["split_quant"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    bt.finish(st, 1)
    fused()                                                                # the records of the last split, all of them
    m_fused = lambda: bt.merge_planes_grid_quant_dev(st, k, [lags], [step], planes, poff, [n], d_n, d_outl, [0], [found], back, [0])

    def m_two():
        bt.merge_planes_grid_dev(st, k, [lags], planes, poff, [n], d_n, codes, [0])
        torch.mul(codes.to(x.dtype), step, out=back2)

    m_fused()
    m_two()
    bt.finish(st, 1)
    good = torch.ones(n, dtype=torch.bool, device=dev)
    good[d_outl[0:2 * found:2]] = False                                    # an outlier is the original's bits, not code * step
    if not torch.equal(back[good], back2[good]) or not torch.equal(back[~good], x[~good]) \
            or float((back.double() - x.double()).abs().max()) > bound:
        sys.exit(f"{x.dtype} lags {lags}: the tensors of the two merge forms differ, or miss the bound")
    del good
    ma, mb = timed_pair(torch, st, m_fused, m_two, args.reps, args.warmup)
    legs["merge_quant"], legs["merge_then_scale"] = leg(ma, n * k), leg(mb, n * k)
    legs["merge_quant"]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    bt.finish(st, 1)
    # the restore pass's share: the exact merge alone, alternately with the quantised one
    m_plain = lambda: bt.merge_planes_grid_dev(st, k, [lags], planes, poff, [n], d_n, codes, [0])
    ma, mb = timed_pair(torch, st, m_fused, m_plain, args.reps, args.warmup)
    legs["merge_exact"] = leg(mb, n * k)
    legs["merge_quant"]["restore_share"] = round(1 - statistics.median(mb) / statistics.median(ma), 3)
    bt.finish(st, 1)
    print(f"{x.dtype} lags {lags}: split_quant {legs['split_quant']['ms']['median']} ms, quant_then_split "
          f"{legs['quant_then_split']['ms']['median']} ms; merge_quant {legs['merge_quant']['ms']['median']} ms, merge_then_scale "
          f"{legs['merge_then_scale']['ms']['median']} ms, merge_exact {legs['merge_exact']['ms']['median']} ms", file=sys.stderr,
          flush=True)
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
    res = {"bytes": nbytes, "reps": args.reps, "warmup": args.warmup, "lib": pkg.LIB_PATH, "abs_error": args.abs_error, "legs": {}}
    bt = pkg.Batch(8, 1 << 20)
    with torch.cuda.stream(st):
        for name, fty in (("float32", torch.float32), ("float64", torch.float64)):
            k = torch.empty((), dtype=fty).element_size()
            n = nbytes // k
            # a smooth field of values in +-1000: three waves along the flattened index
            i = torch.arange(n, dtype=torch.float64, device=dev)
            x = (1000 * torch.sin(i / 977) * torch.cos(i / 40961) * torch.sin(i / 1048583 + 0.3)).to(fty)
            del i
            res["legs"][name] = {}
            for lags in sets:
                res["legs"][name][",".join(map(str, lags))] = field_legs(torch, pkg, bt, st, args, x, k, lags, args.abs_error)
                torch.cuda.empty_cache()
            del x
            torch.cuda.empty_cache()
    bt.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The byte-plane transposes (split_planes_dev / merge_planes_dev; csrc/planes.hip) on a 1 GiB bf16 and a 1 GiB fp32 tensor,
next to what a user has without them and next to a plain copy.  Standalone; one process on one MI355X; HIP events around one
enqueue on a stream (no batch set-up, no synchronisation inside), the median of --reps calls after --warmup untimed ones.

  python tools/ubench/planes_rate.py [--reps 20] [--warmup 3] [--mib 1024] [--lib PATH] [--no-mover] [--xor-only] [--diff-only]
                                      [--records-only]

Legs, per dtype; the rate is (bytes read + bytes written) / time = 2 x the tensor's bytes / time:
  split_planes_dev   one block, the whole tensor
  merge_planes_dev   its inverse
  torch_split        x.view(torch.uint8).reshape(-1, k).t().contiguous()      (the generic strided copy)
  torch_merge        planes.t().contiguous().view(dtype)                       (its inverse)
  torch_copy         y.copy_(x): the same bytes moved and nothing else
The transposes against a base (split_planes_xor_dev / merge_planes_xor_dev), per dtype with the base 16-aligned ("aligned") and
one byte behind that ("base+1"), each next to what a user has without them, timed alternately with it in the same loop:
  split_xor          one launch: planes of (x XOR base), base read in place          3 x the tensor's bytes
  xor_then_split     torch.bitwise_xor into a temporary, then split_planes_dev       5 x
  merge_xor          one launch: (planes merged) XOR base                            3 x
  merge_then_xor     merge_planes_dev, then bitwise_xor_ in place                    5 x
The rate of all four is the JOB's bytes, 3 x the tensor's, over the time, so that the two forms compare; `ratio` is the two-step
time over the fused time.  torch XORs integers of the element's width where the base can be viewed as such, and bytes at
base+1, where it cannot.  --xor-only leaves out the plain legs and the mover.
The transposes of differences (split_planes_diff_dev / merge_planes_diff_dev), per dtype on the tensor's bits as int16 / int32,
both sides 16-aligned, each next to what a user has without them, timed alternately with it in the same loop:
  split_diff         one launch: planes of the folded differences                    2 x the tensor's bytes moved
  diff_then_split    torch.diff into a temporary (its first element copied), then split_planes_dev          4 x
  merge_diff         three launches: the prefix sums of the unfolded planes          3 x (the planes are read twice)
  merge_then_cumsum  merge_planes_dev, then torch.cumsum(dtype = the signed dtype of that width)            4 x
torch's side leaves the zigzag fold out, which favours it.  As with the XOR legs the rate of all four is 3 x the tensor's bytes
over the time, and `ratio` the two-step time over the fused time.  `split_plain` / `merge_plain` are the plain entries timed
alternately with the fused ones in a loop of their own, `vs_plain` the fused time over the plain time.  --diff-only leaves out
everything else.
The record transposes (split_records_dev / merge_records_dev; csrc/records.hip) on uint8 buffers of --mib MiB (rounded down to
whole groups of 16 records), both sides 16-aligned, per width:
  3, 12, 16, 32      split_records_dev / merge_records_dev next to torch_split = x.view(n, w).t().contiguous() and torch_merge,
                     its inverse; `records_done`: ours is the faster one in all eight comparisons
  2, 4, 8            next to split_planes_dev / merge_planes_dev, timed alternately in one loop; `vs_planes` is the record
                     entry's time over the plane entry's
The rate is 2 x the buffer's bytes / time.  --records-only leaves out everything else but the mover.
and once: `mover`, the one-shot copy figure of tools/ubench/mover (a fraction of 8 TB/s, as a child process after everything
timed here) when its binary is present.  Every answer is checked against the torch expression before it is timed.  --lib
measures another build of the library (an experiment's).  Prints one JSON document."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, st, fn, reps, warmup):
    for _ in range(warmup):
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


def timed_pair(torch, st, fa, fb, reps, warmup):
    """fa and fb alternately in one loop -> their times"""
    for _ in range(warmup):
        fa()
        fb()
    st.synchronize()
    out = ([], [])
    for _ in range(reps):
        for fn, ms in ((fa, out[0]), (fb, out[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            b.synchronize()
            ms.append(a.elapsed_time(b))
    return out


def leg(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
            "GB_s": round(nbytes / (med / 1e3) / 1e9, 1)}


def xor_legs(torch, pkg, bt, st, args, x, dtype, k, n, d_n, planes, back, poff):
    """the four XOR legs for the base 16-aligned and one byte behind"""
    dev = x.device
    ity = {2: torch.int16, 4: torch.int32}[k]
    store = torch.empty(n * k + 32, dtype=torch.uint8, device=dev)
    res = {}
    for name, shift in (("aligned", 0), ("base+1", 1)):
        o = (-store.data_ptr()) % 16 + shift
        base8 = store[o:o + n * k]
        # a checkpoint's base: the tensor with one element in sixteen redrawn
        base8.copy_(x.view(torch.uint8))
        base8.view(-1, 16 * k)[:, :k] = torch.randint(0, 256, (n // 16, k), dtype=torch.uint8, device=dev)
        if shift == 0:
            bi = base8.view(ity)
            t_xor = lambda: torch.bitwise_xor(x.view(ity), bi)
            t_unxor = lambda: back.view(ity).bitwise_xor_(bi)
        else:
            t_xor = lambda: torch.bitwise_xor(x.view(torch.uint8), base8)
            t_unxor = lambda: back.view(torch.uint8).bitwise_xor_(base8)
        split_x = lambda: bt.split_planes_xor_dev(st, k, x, [0], base8, [0], [n], d_n, planes, poff)
        merge_x = lambda: bt.merge_planes_xor_dev(st, k, planes, poff, base8, [0], [n], d_n, back, [0])

        def two_split():
            tmp = t_xor()
            bt.split_planes_dev(st, k, tmp, [0], [n], d_n, planes, poff)

        def two_merge():
            bt.merge_planes_dev(st, k, planes, poff, [n], d_n, back, [0])
            t_unxor()

        want = t_xor().view(torch.uint8).reshape(-1, k).t().contiguous()
        split_x()
        bt.finish(st, 1)
        ok = torch.equal(planes.view(k, n), want)
        merge_x()
        bt.finish(st, 1)
        ok = ok and torch.equal(back.view(torch.uint8), x.view(torch.uint8))
        two_split()
        bt.finish(st, 1)
        ok = ok and torch.equal(planes.view(k, n), want)
        two_merge()
        bt.finish(st, 1)
        if not ok or not torch.equal(back.view(torch.uint8), x.view(torch.uint8)):
            sys.exit(f"{name}: the XOR legs differ from the torch expression")
        del want
        legs = {}
        for fused, two, fa, fb in (("split_xor", "xor_then_split", split_x, two_split),
                                   ("merge_xor", "merge_then_xor", merge_x, two_merge)):
            ma, mb = timed_pair(torch, st, fa, fb, args.reps, args.warmup)
            legs[fused], legs[two] = leg(ma, 3 * n * k), leg(mb, 3 * n * k)
            legs[fused]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
        bt.finish(st, 1)
        res[name] = legs
    return res


def diff_legs(torch, pkg, bt, st, args, x, k, n, d_n, planes, back, poff):
    """the four legs of the differences and the plain entries next to the fused ones"""
    ity = {2: torch.int16, 4: torch.int32}[k]
    xi, bi = x.view(ity), back.view(ity)
    tmp, other = torch.empty_like(xi), torch.empty_like(xi)
    split_d = lambda: bt.split_planes_diff_dev(st, k, x, [0], [n], d_n, planes, poff)
    merge_d = lambda: bt.merge_planes_diff_dev(st, k, planes, poff, [n], d_n, back, [0])
    split_p = lambda: bt.split_planes_dev(st, k, x, [0], [n], d_n, planes, poff)
    merge_p = lambda: bt.merge_planes_dev(st, k, planes, poff, [n], d_n, back, [0])

    def two_split():
        tmp[:1].copy_(xi[:1])
        torch.diff(xi, out=tmp[1:])
        bt.split_planes_dev(st, k, tmp, [0], [n], d_n, planes, poff)

    def two_merge():
        bt.merge_planes_dev(st, k, planes, poff, [n], d_n, back, [0])
        torch.cumsum(bi, 0, dtype=ity, out=other)

    # the fused answer against torch's integer arithmetic (wrapping, as the signed dtypes do on the device)
    d = torch.empty_like(xi)
    d[:1].copy_(xi[:1])
    torch.diff(xi, out=d[1:])
    want = ((d << 1) ^ (d >> (8 * k - 1))).view(torch.uint8).reshape(-1, k).t().contiguous()
    split_d()
    bt.finish(st, 1)
    ok = torch.equal(planes.view(k, n), want)
    back.view(torch.uint8).zero_()
    merge_d()
    bt.finish(st, 1)
    ok = ok and torch.equal(back.view(torch.uint8), x.view(torch.uint8))
    del want
    two_split()
    bt.finish(st, 1)
    ok = ok and torch.equal(planes.view(k, n), d.view(torch.uint8).reshape(-1, k).t().contiguous())
    two_merge()
    bt.finish(st, 1)
    if not ok or not torch.equal(other.view(torch.uint8), x.view(torch.uint8)):
        sys.exit("the legs of the differences differ from the torch expression")
    del d
    legs = {}
    for fused, two, fa, fb in (("split_diff", "diff_then_split", split_d, two_split),
                               ("merge_diff", "merge_then_cumsum", merge_d, two_merge)):
        ma, mb = timed_pair(torch, st, fa, fb, args.reps, args.warmup)
        legs[fused], legs[two] = leg(ma, 3 * n * k), leg(mb, 3 * n * k)
        legs[fused]["ratio"] = round(statistics.median(mb) / statistics.median(ma), 3)
    for fused, plain, fa, fb in (("split_diff", "split_plain", split_d, split_p), ("merge_diff", "merge_plain", merge_d, merge_p)):
        ma, mb = timed_pair(torch, st, fa, fb, args.reps, args.warmup)
        legs[plain] = leg(mb, 3 * n * k)
        legs[plain]["fused_ms"] = leg(ma, 3 * n * k)["ms"]
        legs[fused]["vs_plain"] = round(statistics.median(ma) / statistics.median(mb), 3)
    bt.finish(st, 1)
    return legs


def record_legs(torch, bt, st, args, dev, nbytes):
    """the record entries at widths 3, 12, 16, 32 next to torch's strided copy, and at 2, 4, 8 next to the plane entries"""
    res = {}
    for w in (3, 12, 16, 32, 2, 4, 8):
        n = nbytes // (16 * w) * 16
        x = torch.randint(0, 256, (n * w,), dtype=torch.uint8, device=dev)
        d_n = torch.tensor([n], dtype=torch.int64, device=dev)
        cols = torch.empty(w * n, dtype=torch.uint8, device=dev)
        back = torch.empty_like(x)
        poff = [j * n for j in range(w)]
        split = lambda: bt.split_records_dev(st, w, x, [0], [n], d_n, cols, poff)
        merge = lambda: bt.merge_records_dev(st, w, cols, poff, [n], d_n, back, [0])
        t_split = lambda: x.view(n, w).t().contiguous()
        want = t_split()
        t_merge = lambda: want.t().contiguous()
        split()
        merge()
        bt.finish(st, 1)
        if not torch.equal(cols.view(w, n), want) or not torch.equal(back, x) or not torch.equal(t_merge().view(-1), x):
            sys.exit(f"width {w}: the columns differ from the torch expression")
        legs = {"records": n}
        if w in (2, 4, 8):
            p_split = lambda: bt.split_planes_dev(st, w, x, [0], [n], d_n, cols, poff)
            p_merge = lambda: bt.merge_planes_dev(st, w, cols, poff, [n], d_n, back, [0])
            for ours, theirs, fa, fb in (("split_records_dev", "split_planes_dev", split, p_split),
                                         ("merge_records_dev", "merge_planes_dev", merge, p_merge)):
                ma, mb = timed_pair(torch, st, fa, fb, args.reps, args.warmup)
                legs[ours], legs[theirs] = leg(ma, 2 * n * w), leg(mb, 2 * n * w)
                legs[ours]["vs_planes"] = round(statistics.median(ma) / statistics.median(mb), 3)
        else:
            for what, fn in (("split_records_dev", split), ("merge_records_dev", merge), ("torch_split", t_split),
                             ("torch_merge", t_merge)):
                legs[what] = leg(timed(torch, st, fn, args.reps, args.warmup), 2 * n * w)
        bt.finish(st, 1)
        res[str(w)] = legs
        del x, cols, back, want
        torch.cuda.empty_cache()
    return res


def mover_one_shot():
    exe = os.path.join(ROOT, "tools", "ubench", "mover")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe, "headline"], capture_output=True, text=True, timeout=120)
    fr = [float(l.rsplit(":", 1)[1].strip(" )")) for l in r.stdout.splitlines() if "of 8 TB/s" in l]
    return fr[0] if fr else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-mover", action="store_true")
    ap.add_argument("--xor-only", action="store_true")
    ap.add_argument("--diff-only", action="store_true")
    ap.add_argument("--records-only", action="store_true")
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
    bt = pkg.Batch(1, 1 << 20)
    with torch.cuda.stream(st):
        for name, dtype in (() if args.records_only else (("bf16", torch.bfloat16), ("fp32", torch.float32))):
            k = torch.empty((), dtype=dtype).element_size()
            n = nbytes // k
            x = torch.empty(n, dtype=torch.float32, device=dev).normal_(0, 0.02).to(dtype)
            d_n = torch.tensor([n], dtype=torch.int64, device=dev)
            planes = torch.empty(k * n, dtype=torch.uint8, device=dev)
            back = torch.empty_like(x)
            poff = [j * n for j in range(k)]
            split = lambda: bt.split_planes_dev(st, k, x, [0], [n], d_n, planes, poff)
            merge = lambda: bt.merge_planes_dev(st, k, planes, poff, [n], d_n, back, [0])
            t_split = lambda: x.view(torch.uint8).reshape(-1, k).t().contiguous()
            want = t_split()
            t_merge = lambda: want.t().contiguous().view(-1).view(dtype)
            other = torch.empty_like(x)
            split()
            merge()
            bt.finish(st, 1)
            if not torch.equal(planes.view(k, n), want) or not torch.equal(back.view(torch.uint8), x.view(torch.uint8)) \
                    or not torch.equal(t_merge().view(torch.uint8), x.view(torch.uint8)):
                sys.exit(f"{name}: the planes differ from the torch expression")
            legs = {}
            for what, fn in (("split_planes_dev", split), ("merge_planes_dev", merge), ("torch_split", t_split),
                             ("torch_merge", t_merge), ("torch_copy", lambda: other.copy_(x))):
                if not args.xor_only and not args.diff_only:
                    legs[what] = leg(timed(torch, st, fn, args.reps, args.warmup), 2 * n * k)
            bt.finish(st, 1)
            del want, other
            torch.cuda.empty_cache()
            if not args.diff_only:
                legs["xor"] = xor_legs(torch, pkg, bt, st, args, x, dtype, k, n, d_n, planes, back, poff)
            torch.cuda.empty_cache()
            if not args.xor_only:
                legs["diff"] = diff_legs(torch, pkg, bt, st, args, x, k, n, d_n, planes, back, poff)
            res["legs"][name] = legs
            del x, planes, back
            torch.cuda.empty_cache()
        if args.records_only or not (args.xor_only or args.diff_only):
            res["records"] = record_legs(torch, bt, st, args, dev, nbytes)
            res["records_done"] = all(res["records"][w][ours]["GB_s"] > res["records"][w][theirs]["GB_s"] for w in ("3", "12", "16", "32")
                                      for ours, theirs in (("split_records_dev", "torch_split"), ("merge_records_dev", "torch_merge")))
    bt.close()
    res["diff_done"] = not args.xor_only and not args.records_only and all(res["legs"][d]["diff"][f]["ratio"] > 1 for d in res["legs"]
                                                 for f in ("split_diff", "merge_diff"))
    res["done"] = not args.xor_only and not args.diff_only and not args.records_only and all(res["legs"][d][ours]["GB_s"] >= res["legs"][d][theirs]["GB_s"] for d in res["legs"]
                      for ours, theirs in (("split_planes_dev", "torch_split"), ("merge_planes_dev", "torch_merge")))
    if not args.no_mover and not args.xor_only and not args.diff_only:
        torch.cuda.synchronize()
        fr = mover_one_shot()
        if fr is not None:
            res["mover"] = {"one_shot_frac_of_8TBs": fr, "GB_s": round(fr * 8000, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

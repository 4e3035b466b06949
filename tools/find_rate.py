"""The pattern search (shafa.find, shafa.find_files; csrc/find.hip) on 2 x 64 MiB of synth Zipf(1.2) bytes, next to code the
search does not touch: shafa.crc32 on the same tensor (both are one-read tile passes at any alignment) and checksum_files on
the same file sets.  Standalone; one MI355X; wall clock around whole calls, their synchronisations included; the median of
--reps calls after one untimed call, and min / max.

  python tools/find_rate.py [--reps 5] [--blocks 2] [--event-blocks 16] [--max-bytes N]

Legs:
  crc32            shafa.crc32 of the tensor                                       (yardstick for find)
  absent16_count   find, a 16-byte pattern that does not occur, max_hits = 0      (no emit launch)
  absent16         the same with the default max_hits                             (an emit launch that reads no tile again)
  planted1000      a 16-byte pattern written at 1000 places
  dense1           the 1-byte pattern of the commonest symbol                     (every candidate a match; max_hits entries stored)
  checksum_files   on the mode-N set and on the mode-R set of the tensor          (yardstick for find_files)
  find_files       the planted pattern in both sets
  events           the entries alone, by HIP events around one enqueue (no batch set-up, no synchronisation, no read-back), on
                   --event-blocks regions of 64 MiB (the tensor repeated): crc32_dev, find_dev with the absent pattern
                   (max_hits 0 and 65536), the planted and the dense one
Every answer is checked against numpy on the host before it is timed.  Prints one JSON document.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_verify import BS, stats, timed  # noqa: E402


def wall(torch, fn, reps):
    fn()                                                                 # untimed: code objects, workspace growth
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def positions(data, pat):
    """every start of pat in data (numpy, host)"""
    hit = np.flatnonzero(data[:len(data) - len(pat) + 1] == pat[0])
    for i in range(1, len(pat)):
        hit = hit[data[hit + i] == pat[i]]
    return hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--event-blocks", type=int, default=16)
    ap.add_argument("--max-bytes", type=int, default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    n = args.blocks * BS
    host = synth.gen_bytes(2025, n, synth.zipf_table(1.2)).copy()
    rng = np.random.default_rng(7)
    absent = rng.integers(0, 256, 16, dtype=np.uint8)
    planted = rng.integers(0, 256, 16, dtype=np.uint8)
    for s in np.sort(rng.choice(n // 64 - 1, 1000, replace=False)) * 64 + 13:
        host[s:s + 16] = planted
    common = np.array([np.bincount(host, minlength=256).argmax()], dtype=np.uint8)
    d_in = torch.from_numpy(host).to(dev)
    gib = lambda ms: round(n / (sorted(ms)[len(ms) // 2] / 1e3) / 2**30, 1)
    res = {"bytes": n, "reps": args.reps, "legs": {}}

    def leg(name, fn, check):
        check(fn())
        ms = wall(torch, fn, args.reps)
        res["legs"][name] = {"ms": stats(ms), "GiB_s": gib(ms)}

    import zlib
    digest = zlib.crc32(host)
    leg("crc32", lambda: pkg.crc32(d_in, stream=st), lambda c: c == digest or sys.exit("crc32 differs"))

    def same(pat, max_hits=65536):
        want = positions(host, pat)

        def check(got):
            if got.count != want.size or got.size != n or not np.array_equal(got.positions, want[:max_hits]):
                sys.exit(f"find differs: {got.count} {want.size}")
        return check

    leg("absent16_count", lambda: pkg.find(d_in, absent.tobytes(), max_hits=0, stream=st), same(absent, 0))
    leg("absent16", lambda: pkg.find(d_in, absent.tobytes(), stream=st), same(absent))
    leg("planted1000", lambda: pkg.find(d_in, planted.tobytes(), stream=st), same(planted))
    leg("dense1", lambda: pkg.find(d_in, common.tobytes(), stream=st), same(common))
    res["legs"]["planted1000"]["count"] = int(positions(host, planted).size)
    res["legs"]["dense1"]["count"] = int(positions(host, common).size)
    for name, force in (("N", False), ("R", True)):
        files = pkg.compress_files(d_in, BS, force_rle=force)
        kw = dict(shaf=files[".rle.shaf" if force else ".shaf"].clone(), cod=files[".rle.cod" if force else ".cod"].clone(),
                  decode_rle=force)
        del files
        torch.cuda.empty_cache()
        leg(f"checksum_files_{name}", lambda: pkg.checksum_files(stream=st, max_bytes=args.max_bytes, **kw),
            lambda c: c == pkg.Checksum(digest, n) or sys.exit("checksum_files differs"))
        leg(f"find_files_{name}", lambda: pkg.find_files(planted.tobytes(), stream=st, max_bytes=args.max_bytes, **kw),
            same(planted))
        del kw
        torch.cuda.empty_cache()
    # ---- the entries alone
    nb = args.event_blocks // args.blocks * args.blocks
    if nb:
        d_big = d_in.repeat(nb // args.blocks)
        off, cap = [b * BS for b in range(nb)], [BS] * nb
        d_n = torch.tensor(cap, dtype=torch.int64, device=dev)
        d_crc = torch.zeros(nb, dtype=torch.int32, device=dev)
        d_count = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        d_hits = torch.zeros(65536, dtype=torch.int64, device=dev)
        bt = pkg.Batch(nb, BS)
        ev = {"bytes": nb * BS}
        big = lambda ms: round(nb * BS / (sorted(ms)[len(ms) // 2] / 1e3) / 2**30, 1)
        ms = timed(torch, st, lambda: bt.crc32_dev(st, d_big, off, cap, d_n, d_crc), args.reps)
        bt.finish(st, nb)
        ev["crc32_dev"] = {"ms": stats(ms), "GiB_s": big(ms)}
        for name, pat, mh in (("find_dev_absent16_count", absent, 0), ("find_dev_absent16", absent, 65536),
                              ("find_dev_planted", planted, 65536), ("find_dev_dense1", common, 65536)):
            def one():
                with torch.cuda.stream(st):
                    d_total.zero_()                                          # every call stores its first max_hits matches
                bt.find_dev(st, d_big, off, cap, d_n, None, off, pat.tobytes(), mh, d_hits if mh else None, d_count, d_total)
            ms = timed(torch, st, one, args.reps)
            bt.finish(st, nb)
            want = sum(int(positions(host[b * BS:(b + 1) * BS], pat).size) for b in range(args.blocks)) * (nb // args.blocks)
            if int(d_count.sum().cpu()) != want or int(d_total.cpu()[0]) != want:
                sys.exit(f"{name} differs")
            ev[name] = {"ms": stats(ms), "GiB_s": big(ms), "count": want}
        bt.close()
        res["events"] = ev
    print(json.dumps(res))


if __name__ == "__main__":
    main()

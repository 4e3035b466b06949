"""The seek index against the block-granular reader.  Standalone; one MI355X; wall clock, synchronisations included; median,
min, max over --reps after one untimed call.

  python tools/seek_rate.py [--reps 5] [--blocks 2] [--span 1024] [--ranges 1024] [--step-seconds 120]

On one set of --blocks blocks of 64 MiB (a mode-N .shaf + .cod of Zipf(1.2) bytes) and its mode-R twin (run-heavy bytes,
force_rle), per set:
  build:   build_index against decoded_sizes on the same files, and the index's bytes as a share of the files';
  one:     one 4 KiB read_range against decompress_range of the same bytes;
  many:    --ranges random 4 KiB ranges in ONE read_ranges against the same ranges through decompress_range, one call each.
The yardstick is decompress_range, which this feature leaves untouched.  Every result is compared with the yardstick's bytes.
A step that passes --step-seconds ends the run (SIGALRM); the yardstick's loop of the last step stops at half that budget and
says how many of the ranges it timed (the per-range mean is what `many` is then compared with).  Prints one JSON document.
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_verify import BS, stats  # noqa: E402


def wall(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        xs.append((time.perf_counter() - t0) * 1e3)
    return xs


class Step:
    def __init__(self, seconds, name):
        self.seconds, self.name = seconds, name

    def __enter__(self):
        def late(*_):
            raise SystemExit(f"seek_rate: step {self.name!r} passed {self.seconds} s")
        signal.signal(signal.SIGALRM, late)
        signal.alarm(self.seconds)

    def __exit__(self, *_):
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--span", type=int, default=1024)
    ap.add_argument("--ranges", type=int, default=1024)
    ap.add_argument("--step-seconds", type=int, default=120)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    zt = pkg.zipf_table(1.2)
    n = args.blocks * BS
    res = {"blocks": args.blocks, "span": args.span, "ranges": args.ranges}
    for name in ("N", "R"):
        with Step(args.step_seconds, name + " files"):
            if name == "N":
                d_in = torch.empty(n, dtype=torch.uint8, device=dev)
                pkg.gen_bytes(st, 4343, 0, d_in, n, torch.from_numpy(zt).to(dev))
                st.synchronize()
                files = pkg.compress_files(d_in, BS)
                assert ".shaf" in files
                kw = dict(shaf=files[".shaf"].clone(), cod=files[".cod"].clone())
            else:
                d_in = torch.from_numpy(synth.runs_stream(4711, BS, zt)).to(dev).repeat(args.blocks)
                files = pkg.compress_files(d_in, BS, force_rle=True)
                kw = dict(shaf=files[".rle.shaf"].clone(), cod=files[".rle.cod"].clone())
            del files
            torch.cuda.empty_cache()
        row = {"file_bytes": sum(int(t.numel()) for t in kw.values())}
        with Step(args.step_seconds, name + " build"):
            idx = pkg.build_index(span=args.span, stream=st, **kw)
            assert idx.decoded_size == n and all(b.indexed for b in idx.blocks)
            row["build_index_ms"] = stats(wall(torch, lambda: pkg.build_index(span=args.span, stream=st, **kw), args.reps))
            row["decoded_sizes_ms"] = stats(wall(torch, lambda: pkg.decoded_sizes(stream=st, **kw), args.reps))
            row["index_bytes"] = idx.nbytes
            row["index_share_of_files"] = round(idx.nbytes / row["file_bytes"], 5)
        rng = np.random.default_rng(12)
        ranges = [(int(o), 4096) for o in rng.integers(0, n - 4096, args.ranges)]
        with Step(args.step_seconds, name + " one"):
            o = ranges[0][0]
            assert torch.equal(pkg.read_range(idx, o, 4096, stream=st, **kw), d_in[o:o + 4096])
            row["read_range_ms"] = stats(wall(torch, lambda: pkg.read_range(idx, o, 4096, stream=st, **kw), args.reps))
            row["decompress_range_ms"] = stats(wall(torch, lambda: pkg.decompress_range(o, 4096, stream=st, **kw), args.reps))
        with Step(args.step_seconds, name + " many"):
            out, offs = pkg.read_ranges(idx, ranges, stream=st, **kw)
            for i in range(0, len(ranges), 97):
                assert torch.equal(out[offs[i]:offs[i + 1]], d_in[ranges[i][0]:ranges[i][0] + 4096]), i
            row["read_ranges_ms"] = stats(wall(torch, lambda: pkg.read_ranges(idx, ranges, stream=st, **kw), args.reps))
            pkg.decompress_range(*ranges[0], stream=st, **kw)
            torch.cuda.synchronize()
            t0, done = time.perf_counter(), 0
            for o, k in ranges:
                pkg.decompress_range(o, k, stream=st, **kw)
                done += 1
                if time.perf_counter() - t0 > args.step_seconds / 2:
                    break
            torch.cuda.synchronize()
            per = (time.perf_counter() - t0) * 1e3 / done
            row["decompress_range_calls_timed"] = done
            row["decompress_range_all_ranges_ms"] = round(per * len(ranges), 2)
        row["ratio_one"] = round(row["decompress_range_ms"]["median"] / row["read_range_ms"]["median"], 2)
        row["ratio_many"] = round(row["decompress_range_all_ranges_ms"] / row["read_ranges_ms"]["median"], 2)
        res[name] = row
        del idx, kw, d_in
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

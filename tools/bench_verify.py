"""The compare pass (shafa_hipd_compare_dev, csrc/compare.hip) and shafa.verify_files against decompress_files + torch.equal.
Standalone; one MI355X; median, min, max over --reps.

  python tools/bench_verify.py [--reps 7] [--blocks 1,8,128] [--verify-blocks 1,8,128] [--max-bytes N]

Rows, per nb blocks of 64 MiB (synth.runs_stream bytes, one distinct block repeated on the device):
  compare[nb]:   Batch.compare_dev of nb exact regions against a copy at ref alignment 0 and 1 (HIP events, ms; GB/s over the
                 2 x nb x 64 MiB both operands hold), next to rle_decoded_size_dev over the RLE bytes of the same blocks in the
                 same run (GB/s over the RLE bytes): a read-only pass of the same skeleton over one operand;
  verify[nb]:    verify_files (wall clock, its synchronisations included) against decompress_files + torch.equal on the same
                 sets — a mode-N .shaf + .cod of Zipf(1.2) bytes and the .rle + .freq of the run-heavy bytes — and
                 torch.cuda.max_memory_allocated of both beyond what was resident before the call.
Prints one JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BS = 64 << 20


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(torch, st, fn, reps):
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


def wall_and_peak(torch, fn, reps):
    """-> (ms per call, peak bytes allocated during a call beyond what was allocated before it)"""
    fn()
    torch.cuda.synchronize()
    xs, peak = [], 0
    for _ in range(reps):
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        xs.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - before)
    return xs, peak


def gbs(nbytes, ms):
    return round(nbytes / (statistics.median(ms) / 1e3) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", default="1,8,128")
    ap.add_argument("--verify-blocks", default="1,8,128")
    ap.add_argument("--max-bytes", type=int, default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    zt = pkg.zipf_table(1.2)
    d_block = torch.from_numpy(synth.runs_stream(4711, BS, zt)).to(dev)
    res = {"compare": {}, "verify": {}}
    # ---- the pass alone
    for nb in sorted({int(x) for x in args.blocks.split(",") if x}, reverse=True):
        d_a = d_block.repeat(nb)
        d_r = torch.empty(nb * BS + 16, dtype=torch.uint8, device=dev)
        off, n = [b * BS for b in range(nb)], [BS] * nb
        d_n = torch.tensor(n, dtype=torch.int64, device=dev)
        d_first = torch.zeros(nb, dtype=torch.int64, device=dev)
        bt = pkg.Batch(nb, 2 * BS + 64)
        row = {}
        for al in (0, 1):
            d_ref = d_r[al:al + nb * BS]
            d_ref.copy_(d_a)
            ms = timed(torch, st, lambda: bt.compare_dev(st, d_a, off, n, d_n, d_ref, off, n, d_first), args.reps)
            bt.finish(st, nb)
            assert d_first.cpu().tolist() == n
            row[f"align{al}"] = {"ms": stats(ms), "GB_s": gbs(2 * nb * BS, ms)}
        del d_r, d_ref
        rcap = [2 * BS + 16] * nb
        roff = [b * (2 * BS + 16) for b in range(nb)]
        d_rle = torch.empty(nb * (2 * BS + 16) + 16, dtype=torch.uint8, device=dev)
        d_rn = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
        bt.rle_encode(st, d_a, off, n, d_rle, roff, rcap, d_rn, d_freq)
        bt.finish(st, nb)
        rn = d_rn.cpu().tolist()
        d_size = torch.zeros(nb, dtype=torch.int64, device=dev)
        ms = timed(torch, st, lambda: bt.rle_decoded_size_dev(st, d_rle, roff, rn, d_rn, d_size), args.reps)
        bt.finish(st, nb)
        assert d_size.cpu().tolist() == n
        row["rle_decoded_size"] = {"ms": stats(ms), "rle_bytes": sum(rn), "GB_s": gbs(sum(rn), ms)}
        res["compare"][nb] = row
        bt.close()
        del d_a, d_rle
        torch.cuda.empty_cache()
    # ---- the driver against decoding the file and comparing it
    d_map = torch.from_numpy(zt).to(dev)
    for nb in sorted({int(x) for x in args.verify_blocks.split(",") if x}, reverse=True):
        row = {}
        for name in ("N", "rle+freq"):
            if name == "N":
                d_in = torch.empty(nb * BS, dtype=torch.uint8, device=dev)
                with torch.cuda.stream(st):
                    pkg.gen_bytes(st, 4343 + nb, 0, d_in, nb * BS, d_map)
                st.synchronize()
                files = pkg.compress_files(d_in, BS)
                assert ".shaf" in files
                kw = dict(shaf=files[".shaf"].clone(), cod=files[".cod"].clone(), decode_rle=False)
            else:
                d_in = d_block.repeat(nb)
                files = pkg.compress_files(d_in, BS, force_rle=True)
                kw = dict(rle=files[".rle"].clone(), freq=files[".rle.freq"].clone())
            del files
            torch.cuda.empty_cache()
            got = []
            v_ms, v_peak = wall_and_peak(torch, lambda: got.append(pkg.verify_files(d_in, stream=st, max_bytes=args.max_bytes, **kw)),
                                         args.reps)
            assert all(g == pkg.Verify(True, None, nb * BS) for g in got), got[-1]
            same = []

            def decode_and_compare():
                out = pkg.decompress_files(stream=st, max_bytes=args.max_bytes, **kw)
                same.append(torch.equal(out, d_in))

            d_ms, d_peak = wall_and_peak(torch, decode_and_compare, args.reps)
            assert all(same)
            row[name] = {"verify_files_ms": stats(v_ms), "decompress_and_equal_ms": stats(d_ms),
                         "verify_peak_bytes": v_peak, "decompress_peak_bytes": d_peak, "decoded_bytes": nb * BS,
                         "file_bytes": sum(int(t.numel()) for t in kw.values() if hasattr(t, "numel"))}
            del d_in, kw
            torch.cuda.empty_cache()
        res["verify"][nb] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

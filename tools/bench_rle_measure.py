"""The RLE size pass (shafa_hipd_rle_decoded_size_dev, csrc/rle_measure.hip) against rle_decode_dev — until now the only way to
learn the decoded sizes — on the same resident RLE blocks, and decompress_range against decompress_files.  Standalone; HIP
events around each device row (median, min, max over --reps) on one MI355X.

  python tools/bench_rle_measure.py [--reps 7] [--shapes 128x67108864,1000x65536] [--range-blocks 128]

Rows, per shape nb x block bytes (synth.runs_stream blocks, RLE-encoded on the device by Batch.rle_encode):
  measure:    the size pass: ms, GB/s on the RLE bytes read, fraction of 8 TB/s;
  decode:     rle_decode_dev into regions of exactly the decoded sizes: ms, GB/s on the same RLE bytes (it also writes the
              output: out_GB_s counts read + written);
  range:      decompress_range of 1 MiB from the middle of a mode-N set of --range-blocks x 64 MiB Zipf(1.2) blocks against
              decompress_files of the whole set (wall clock, synchronisations included).
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
PEAK = 8e12


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


def layout(caps):
    off, pos = [], 0
    for c in caps:
        off.append(pos)
        pos += (c + 15) // 16 * 16
    return off, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="128x67108864,1000x65536")
    ap.add_argument("--range-blocks", type=int, default=128)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    synth = pkgload.load_submodule("synth")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    zt = pkg.zipf_table(1.2)
    res = {"shapes": {}}
    for shape in args.shapes.split(","):
        nb, bs = (int(x) for x in shape.split("x"))
        # up to 64 MiB of distinct blocks from the host, repeated on the device to nb blocks (8 GiB: far past every cache)
        uniq = max(1, min(nb, (64 << 20) // bs))
        d_u = torch.from_numpy(synth.runs_stream(99 + nb, uniq * bs, zt)).to(dev).view(uniq, bs)
        d_in = d_u.repeat((nb + uniq - 1) // uniq, 1)[:nb].contiguous().view(-1)
        del d_u
        bt = pkg.Batch(nb, 2 * bs + 64)
        ioff = [b * bs for b in range(nb)]
        rcap = [2 * bs + 16] * nb
        roff, rtot = layout(rcap)
        d_rle = torch.empty(rtot + 16, dtype=torch.uint8, device=dev)
        d_rn = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
        bt.rle_encode(st, d_in, ioff, [bs] * nb, d_rle, roff, rcap, d_rn, d_freq)
        bt.finish(st, nb)
        rn = d_rn.cpu().tolist()
        d_size = torch.zeros(nb, dtype=torch.int64, device=dev)
        ms_m = timed(torch, st, lambda: bt.rle_decoded_size_dev(st, d_rle, roff, rn, d_rn, d_size), args.reps)
        bt.finish(st, nb)
        sizes = d_size.cpu().tolist()
        assert sizes == [bs] * nb, sizes[:4]
        ooff, otot = layout(sizes)
        d_out = torch.empty(otot + 16, dtype=torch.uint8, device=dev)
        d_on = torch.zeros(nb, dtype=torch.int64, device=dev)
        ms_d = timed(torch, st, lambda: bt.rle_decode_dev(st, d_rle, roff, rn, d_rn, d_out, ooff, sizes, d_on), args.reps)
        bt.finish(st, nb)
        assert d_on.cpu().tolist() == sizes and torch.equal(d_out[:nb * bs], d_in)
        rb = sum(rn)
        gm = rb / (statistics.median(ms_m) / 1e3) / 1e9
        gd = rb / (statistics.median(ms_d) / 1e3) / 1e9
        res["shapes"][shape] = {
            "rle_bytes": rb, "decoded_bytes": nb * bs,
            "measure": {"ms": stats(ms_m), "GB_s": round(gm, 1), "peak_frac": round(gm * 1e9 / PEAK, 4)},
            "decode": {"ms": stats(ms_d), "GB_s": round(gd, 1),
                       "out_GB_s": round((rb + nb * bs) / (statistics.median(ms_d) / 1e3) / 1e9, 1)},
            "decode_over_measure": round(statistics.median(ms_d) / statistics.median(ms_m), 2)}
        bt.close()
        del d_in, d_rle, d_out
        torch.cuda.empty_cache()
    # ---- 1 MiB from the middle of a mode-N set against the whole set
    nb, bs = args.range_blocks, 64 << 20
    if nb > 0:
        d_map = torch.from_numpy(zt).to(dev)
        d_in = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            pkg.gen_bytes(st, 777, 0, d_in, nb * bs, d_map)
        st.synchronize()
        files = pkg.compress_files(d_in, bs)
        assert ".shaf" in files
        mid = nb * bs // 2 - (1 << 19)
        shaf, cod = files[".shaf"], files[".cod"]
        row = {}
        for name, fn in (("decompress_range_1MiB", lambda: pkg.decompress_range(mid, 1 << 20, shaf=shaf, cod=cod, stream=st)),
                         ("decompress_files", lambda: pkg.decompress_files(shaf=shaf, cod=cod, decode_rle=False, stream=st))):
            out = fn()
            torch.cuda.synchronize()
            xs = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                xs.append((time.perf_counter() - t0) * 1e3)
            row[name] = stats(xs)
            assert torch.equal(out, d_in[mid:mid + (1 << 20)] if "range" in name else d_in), name
            del out
        res["range"] = {"blocks": nb, "ms": row}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

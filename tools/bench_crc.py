"""The CRC-32 pass (shafa_hipd_crc32_dev, csrc/crc32.hip) and shafa.checksum_files against decompress_files + zlib.crc32 on the
host.  Standalone; one MI355X; median, min, max over --reps.

  python tools/bench_crc.py [--reps 7] [--blocks 1,8,128] [--checksum-blocks 1,8] [--max-bytes N]

Rows, per nb blocks of 64 MiB (synth.runs_stream bytes, one distinct block repeated on the device):
  crc32[nb]:     Batch.crc32_dev of the nb blocks at address alignment 0 and 1 (HIP events, ms; GB/s over the nb x 64 MiB
                 read), checked against zlib.crc32, next to Batch.compare_dev on the same blocks against a copy at the same
                 alignments in the same run (GB/s over the 2 x nb x 64 MiB both operands hold);
  checksum[nb]:  checksum_files (wall clock, its synchronisations included) against decompress_files + a copy to the host +
                 zlib.crc32 there, on a mode-N .shaf + .cod of Zipf(1.2) bytes and the .rle + .freq of the run-heavy bytes,
                 and torch.cuda.max_memory_allocated of both beyond what was resident before the call.
Prints one JSON document.
"""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_verify import BS, gbs, stats, timed, wall_and_peak  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", default="1,8,128")
    ap.add_argument("--checksum-blocks", default="1,8")
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
    block = synth.runs_stream(4711, BS, zt)
    want = zlib.crc32(block.tobytes())
    d_block = torch.from_numpy(block).to(dev)
    res = {"crc32": {}, "checksum": {}}
    # ---- the pass alone, next to the compare pass
    for nb in sorted({int(x) for x in args.blocks.split(",") if x}, reverse=True):
        d_a = d_block.repeat(nb)
        d_r = torch.empty(nb * BS + 16, dtype=torch.uint8, device=dev)
        off, n = [b * BS for b in range(nb)], [BS] * nb
        d_n = torch.tensor(n, dtype=torch.int64, device=dev)
        d_crc = torch.zeros(nb, dtype=torch.int32, device=dev)
        d_first = torch.zeros(nb, dtype=torch.int64, device=dev)
        bt = pkg.Batch(nb, 2 * BS + 64)
        row = {}
        for al in (0, 1):
            d_ref = d_r[al:al + nb * BS]
            d_ref.copy_(d_a)
            ms = timed(torch, st, lambda: bt.crc32_dev(st, d_ref, off, n, d_n, d_crc), args.reps)
            bt.finish(st, nb)
            assert [c & 0xFFFFFFFF for c in d_crc.cpu().tolist()] == [want] * nb
            row[f"crc32_align{al}"] = {"ms": stats(ms), "GB_s": gbs(nb * BS, ms)}
            ms = timed(torch, st, lambda: bt.compare_dev(st, d_a, off, n, d_n, d_ref, off, n, d_first), args.reps)
            bt.finish(st, nb)
            assert d_first.cpu().tolist() == n
            row[f"compare_align{al}"] = {"ms": stats(ms), "GB_s": gbs(2 * nb * BS, ms)}
        res["crc32"][nb] = row
        bt.close()
        del d_a, d_r, d_ref
        torch.cuda.empty_cache()
    # ---- the driver against decoding the file and digesting it on the host
    d_map = torch.from_numpy(zt).to(dev)
    for nb in sorted({int(x) for x in args.checksum_blocks.split(",") if x}, reverse=True):
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
            digest = pkg.crc32(d_in, stream=st)
            del files, d_in
            torch.cuda.empty_cache()
            got = []
            c_ms, c_peak = wall_and_peak(torch, lambda: got.append(pkg.checksum_files(stream=st, max_bytes=args.max_bytes, **kw)),
                                         args.reps)
            assert all(g == pkg.Checksum(digest, nb * BS) for g in got), got[-1]
            host = []

            def decode_and_digest():
                out = pkg.decompress_files(stream=st, max_bytes=args.max_bytes, **kw)
                host.append(zlib.crc32(out.cpu().numpy()))

            d_ms, d_peak = wall_and_peak(torch, decode_and_digest, args.reps)
            assert all(h == digest for h in host)
            row[name] = {"checksum_files_ms": stats(c_ms), "decompress_and_zlib_ms": stats(d_ms),
                         "checksum_peak_bytes": c_peak, "decompress_peak_bytes": d_peak, "decoded_bytes": nb * BS,
                         "file_bytes": sum(int(t.numel()) for t in kw.values() if hasattr(t, "numel"))}
            del kw
            torch.cuda.empty_cache()
        res["checksum"][nb] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The payload pack (shafa_hipd_pack_payloads, csrc/pack.hip) against the two ways a caller assembles a .shaf / .rle today.
Standalone; HIP events for the device rows, wall clock for the host assembly (its copies and the join are what it costs);
the compared forms alternate within one process.

  python tools/bench_pack_dev.py [--reps 7] [--steps 5] [--host-reps 3] [--blocks 128,8,1]

Workload: nb x 64 MiB Zipf(1.2) blocks, encoded by hist256_tiles -> sf_build_codes -> sf_encode_dev; the payloads lie at the
start of their worst-case regions with their sizes on the device, as that chain leaves them.  Rows per nb:
  pack_shaf / pack_raw:  Batch.pack_payloads(FRAME_SHAF / FRAME_RAW): ms per call (median, min, max over the repetitions);
  torch_copy_loop:       one torch slice copy_ per block into the same unaligned destinations as the .shaf (payload bytes
                         only, sizes known on the host);
  host_assembly:         what tests/test_gpu_fullsize.py does: a device-to-host copy per block, then b"".join with the headers.
GB/s counts 2 x payload bytes (read + write); peak_frac is that over 8 TB/s.  Prints one JSON document.
"""
import argparse
import hashlib
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--blocks", default="128,8,1")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pkgload
    pkg = pkgload.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    bs = 64 << 20
    d_map = torch.from_numpy(pkg.zipf_table(1.2)).to(dev)
    res = {}
    for nb in [int(x) for x in args.blocks.split(",")]:
        d_in = torch.empty(nb * bs, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            pkg.gen_bytes(st, 4242 + nb, 0, d_in, nb * bs, d_map)
        off, n = [b * bs for b in range(nb)], [bs] * nb
        thb = pkg.tile_hist_bytes(bs)
        d_th = torch.empty(nb * thb, dtype=torch.uint8, device=dev)
        d_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
        d_tab = torch.empty(nb * 8448, dtype=torch.uint8, device=dev)
        d_n_in = torch.tensor(n, dtype=torch.int64, device=dev)
        ocap = bs * 9 // 8 + 64                       # Zipf(1.2) codes average ~5.3 bits
        ooff = [b * ocap for b in range(nb)]
        d_enc = torch.empty(nb * ocap, dtype=torch.uint8, device=dev)
        d_enc_n = torch.zeros(nb, dtype=torch.int64, device=dev)
        bt = pkg.Batch(nb, bs)
        bt.hist256_tiles(st, d_in, off, n, d_freq, d_th, [b * thb for b in range(nb)])
        bt.sf_build_codes(st, nb, d_freq, d_tab)
        bt.sf_encode_dev(st, d_in, off, n, d_n_in, d_tab, d_enc, ooff, [ocap] * nb, d_enc_n,
                         d_th, [b * thb for b in range(nb)])
        bt.finish(st, nb)
        del d_in, d_th
        torch.cuda.empty_cache()
        sizes = [int(x) for x in d_enc_n.cpu().tolist()]
        payload = sum(sizes)
        caps = [ocap] * nb
        cap_shaf, cap_raw = pkg.pack_payloads_max(caps, pkg.FRAME_SHAF), pkg.pack_payloads_max(caps, pkg.FRAME_RAW)
        d_dst = torch.empty(cap_shaf, dtype=torch.uint8, device=dev)
        d_dst_n = torch.zeros(1, dtype=torch.int64, device=dev)
        # the .shaf's payload destinations (host-known here, for the torch loop)
        head = b"@" + str(nb).encode()
        doff, pos = [], len(head)
        for k in sizes:
            pos += 2 + len(str(k))
            doff.append(pos)
            pos += k
        shaf_len = pos

        def pack_shaf():
            bt.pack_payloads(st, pkg.FRAME_SHAF, d_enc, ooff, caps, d_enc_n, d_dst, cap_shaf, d_dst_n)

        def pack_raw():
            bt.pack_payloads(st, pkg.FRAME_RAW, d_enc, ooff, caps, d_enc_n, d_dst, cap_raw, d_dst_n)

        def torch_loop():
            with torch.cuda.stream(st):
                for b in range(nb):
                    d_dst[doff[b]:doff[b] + sizes[b]].copy_(d_enc[ooff[b]:ooff[b] + sizes[b]])

        def host_assembly():
            out = head
            for b in range(nb):
                out += b"@" + str(sizes[b]).encode() + b"@" + d_enc[ooff[b]:ooff[b] + sizes[b]].cpu().numpy().tobytes()
            return out

        # results: the pack's .shaf equals the host assembly, its .rle the payloads back to back
        t0 = time.perf_counter()
        want = host_assembly()
        host_first_ms = (time.perf_counter() - t0) * 1e3
        want_sha = hashlib.sha256(want).hexdigest()
        del want
        pack_shaf()
        bt.finish(st, nb)
        ok_shaf = int(d_dst_n.item()) == shaf_len and \
            hashlib.sha256(d_dst[:shaf_len].cpu().numpy().tobytes()).hexdigest() == want_sha
        pack_raw()
        bt.finish(st, nb)
        raw_sha = hashlib.sha256()
        for b in range(nb):
            raw_sha.update(d_enc[ooff[b]:ooff[b] + sizes[b]].cpu().numpy().tobytes())
        ok_raw = int(d_dst_n.item()) == payload and \
            hashlib.sha256(d_dst[:payload].cpu().numpy().tobytes()).hexdigest() == raw_sha.hexdigest()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.steps):
                fn()
            e1.record(st)
            bt.finish(st, nb)
            return e0.elapsed_time(e1) / args.steps

        forms = {"pack_shaf": pack_shaf, "pack_raw": pack_raw, "torch_copy_loop": torch_loop}
        for fn in forms.values():
            timed(fn)                                 # warm-up
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():               # alternated
                times[k].append(timed(fn))
        host_ms = [host_first_ms]
        for _ in range(max(args.host_reps - 1, 0)):
            t0 = time.perf_counter()
            host_assembly()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        row = {"workload": f"{nb} x 64 MiB Zipf(1.2) after sf_encode_dev", "payload_bytes": payload, "shaf_bytes": shaf_len,
               "identical": {"shaf_vs_host_assembly": ok_shaf, "raw_vs_payloads": ok_raw}}
        for k, v in list(times.items()) + [("host_assembly", host_ms)]:
            med = statistics.median(v)
            row[k] = {"ms": stats(v), "GBs": round(2 * payload / (med * 1e-3) / 1e9, 1),
                      "peak_frac": round(2 * payload / (med * 1e-3) / PEAK, 3)}
        row["pack_shaf_over_torch_copy_loop"] = round(statistics.median(times["pack_shaf"]) /
                                                      statistics.median(times["torch_copy_loop"]), 4)
        res[f"{nb}_blocks"] = row
        bt.close()
        del d_enc, d_dst
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of the fused decode-and-measure kernels (include/cvtt_mi355x.h, cvttmi_measure_error_device) on one GPU.

    python tools/measure_bench.py [--sizes 4096,16384] [--reps 10] [--formats bc1,bc7,...] [--out file.json]

Per format and image size (S x S texels = (S/4)^2 blocks): seeded random packed blocks and source blocks in HBM, the
device-pointer measure timed with HIP events (median of --reps calls; a call = the measure kernel and its one-workgroup
total), algorithmic bytes = packed + source, and the share of 8 TB/s.  BC7 at the first size also times the route of
Context.psnr_bc7 (decode to HBM, then torch arithmetic and .item()).  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats`.  Prints one JSON line per case and writes them all to --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
FORMATS = ["bc1", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s", "etc1", "etc2", "etc2rgba", "etc2punchthrough", "eac", "r11u",
           "r11s", "bc7", "bc6hu", "bc6hs"]


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--formats", default=",".join(FORMATS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    ctx = api.Context(0)
    lib = ctx._lib
    tot = torch.zeros(80, dtype=torch.uint8, device="cuda")
    results = []
    for size in [int(s) for s in args.sizes.split(",")]:
        n = (size // 4) ** 2
        g = torch.Generator(device="cuda")
        for fmt in args.formats.split(","):
            fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
            g.manual_seed(fid)
            packed = torch.randint(0, 256, (n, bpb), dtype=torch.uint8, device="cuda", generator=g)
            if fmt in ("bc6hu", "bc6hs"):
                src = (torch.rand((n, 16, 4), device="cuda", generator=g) * 4).half().view(torch.int16)
            elif fmt in ("r11u", "r11s"):
                src = torch.randint(-1023, 2047, (n, 16), dtype=torch.int16, device="cuda", generator=g)
            else:
                src = torch.randint(0, 256, (n, 16, 4), dtype=torch.uint8, device="cuda", generator=g)
            stream = torch.cuda.current_stream().cuda_stream

            def run():
                rc = lib.cvttmi_measure_error_device(ctx._h, fid, packed.data_ptr(), src.data_ptr(), n, None, tot.data_ptr(), stream)
                assert rc == 0, rc

            med, best = timed(torch, run, args.reps)
            nbytes = n * (bpb + tex)
            rec = {"format": fmt, "size": size, "blocks": n, "us_median": round(med, 2), "us_best": round(best, 2),
                   "bytes": nbytes, "GBps": round(nbytes / med / 1e3, 1), "share_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
            if fmt == "bc7" and size == int(args.sizes.split(",")[0]):
                # the route of Context.psnr_bc7: decode to HBM, torch arithmetic, .item()
                r_med, r_best = timed(torch, lambda: ctx.psnr_bc7(src, packed), args.reps)
                rec["psnr_bc7_route_us_median"] = round(r_med, 2)
                rec["fused_speedup_vs_psnr_bc7"] = round(r_med / med, 2)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del packed, src
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"library_source_sha256": api.library_source_sha256(), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()

"""Timing of the mip chain (include/cvtt_mi355x.h "mip chains", Context.build_mips / encode_mips) on one GPU.

    python tools/mips_bench.py [--reps 30] [--chain-reps 10] [--chain-size 4096] [--small] [--out profiles/mips/mips_bench.json]

1. The level-1 launch (cvttmi_build_mips_device with two levels) at 16384^2 RGBA8 and 8192^2 RGBA16F, timed with device events.
   Bytes moved = the image read + the level written.  The yardstick is a device-to-device hipMemcpyAsync that moves the same
   total (it copies half of it: a copy reads and writes every byte), timed in the same process, the two sides alternating.
2. The whole chain at --chain-size^2 for BC7 (default plan) and BC1: Context.encode_mips (the downsample launches, one tiling
   launch per level, ONE encode call, one compaction per level) against a loop of Context.encode_image over the same,
   prebuilt level images -- the only way to a chain before encode_mips existed.  The two sides alternate; both end in a
   device synchronise inside the events.  The outputs of the two sides are compared as well.
Every figure is the median of the repetitions with the minimum and the 10th / 90th percentile beside it.  --small shrinks
every size (a rehearsal of the script, not a measurement).  Prints one JSON line per case and writes them all to --out with
the library's source SHA-256."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(us):
    us = np.asarray(us, np.float64)
    return {"us_median": round(float(np.median(us)), 2), "us_min": round(float(us.min()), 2),
            "us_p10": round(float(np.percentile(us, 10)), 2), "us_p90": round(float(np.percentile(us, 90)), 2), "reps": int(us.size)}


def alternate(torch, sides, reps, warmup=3):
    """sides: {name: fn}; every repetition runs each side once, in turn, between its own pair of events -> {name: [us]}"""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    return times


def level1_case(torch, api, ctx, hip, size, kind, reps):
    lib = ctx._lib
    texel = 8 if kind == api.PIXELS_RGBA16F else 4
    g = torch.Generator(device="cuda")
    g.manual_seed(size + kind)
    if kind == api.PIXELS_RGBA16F:
        image = (torch.rand((size, size, 4), device="cuda", generator=g) * 4).half().view(torch.int16)
    else:
        image = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
    layout = api.mip_layout(size, size, texel, 16, 2)
    pyramid = torch.empty(layout.pyramid_bytes, dtype=torch.uint8, device="cuda")
    moved = size * size * texel + layout.pyramid_bytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        rc = lib.cvttmi_build_mips_device(ctx._h, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), size, size,
                                          size * texel, kind, 2, stream)
        assert rc == 0, rc

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), moved // 2, 3, stream)
        assert rc == 0, rc  # 3 = hipMemcpyDeviceToDevice

    t = alternate(torch, {"kernel": kernel, "copy": copy}, reps)
    rec = {"case": "level1", "pixels": "rgba16f" if kind == api.PIXELS_RGBA16F else "rgba8", "size": size, "bytes_moved": moved,
           "kernel": stats(t["kernel"]), "copy_same_bytes": stats(t["copy"])}
    rec["kernel_GBps"] = round(moved / rec["kernel"]["us_median"] / 1e3, 1)
    rec["copy_GBps"] = round(moved / rec["copy_same_bytes"]["us_median"] / 1e3, 1)
    rec["kernel_over_copy_rate"] = round(rec["kernel_GBps"] / rec["copy_GBps"], 3)
    return rec


def chain_case(torch, api, ctx, fmt, size, reps):
    g = torch.Generator(device="cuda")
    g.manual_seed(size)
    image = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
    images = ctx.build_mips(image)
    torch.cuda.synchronize()
    keep = {}

    def one_call():
        keep["mips"] = ctx.encode_mips(fmt, image)

    def loop():
        keep["loop"] = [ctx.encode_image(fmt, level) for level in images]

    def build_only():
        ctx.build_mips(image)

    t = alternate(torch, {"encode_mips": one_call, "encode_image_loop": loop, "build_mips": build_only}, reps)
    same = all(bool((a == b).all().item()) for a, b in zip(keep["mips"], keep["loop"]))
    rec = {"case": "chain", "format": fmt, "size": size, "levels": len(images), "outputs_identical": same,
           "encode_mips": stats(t["encode_mips"]), "encode_image_loop": stats(t["encode_image_loop"]), "build_mips": stats(t["build_mips"])}
    rec["encode_mips_over_loop"] = round(rec["encode_mips"]["us_median"] / rec["encode_image_loop"]["us_median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--chain-reps", type=int, default=10)
    ap.add_argument("--chain-size", type=int, default=4096)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "mips", "mips_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("mips_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    # the HIP runtime this process already has mapped (one runtime per process: api.load_library)
    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    results = []
    for size, kind in ((16384, api.PIXELS_RGBA8), (8192, api.PIXELS_RGBA16F)):
        rec = level1_case(torch, api, ctx, hip, size // 16 if args.small else size, kind, args.reps)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        torch.cuda.empty_cache()
    for fmt in ("bc7", "bc1"):
        rec = chain_case(torch, api, ctx, fmt, args.chain_size // 16 if args.small else args.chain_size, args.chain_reps)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0),
                   "small": bool(args.small), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()

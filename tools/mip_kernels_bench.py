"""Timing of the mip kernels wider than 2x2 (include/cvtt_mi355x.h "mip chains", CVTTMI_MIP_KERNEL_*) on one GPU.

    python tools/mip_kernels_bench.py [--reps 30] [--size 16384] [--small] [--floor-tbps 6.29] [--out profiles/mips/mip_kernels_bench.json]

The level-1 launch (cvttmi_build_mips_filtered_device with two levels) of a --size^2 RGBA8 image of random bytes under every
kernel with the plain rule and with SRGB, and under the 2x2 filters of tools/mip_filters_bench.py (box, srgb, normal, box+alpha,
srgb+alpha, and the box a second time: "box_again", the noise every ratio is read against), all in ONE run, timed with device
events as tools/mips_bench.py does: every repetition runs each side once, in turn.  Every figure is the median of the
repetitions with the minimum and the 10th / 90th percentile beside it; "over_box" is the median over the median of "box" in the
same run, "over_floor" the median over the time the bytes moved (the level read once, level 1 written once) take at 6.29 TB/s,
the rate a float4 copy reaches on this part (--floor-tbps).  --small shrinks the image (a rehearsal of the
script, not a measurement).  Prints one JSON line per side and writes them all to --out with the library's source SHA-256."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mips_bench import alternate, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--floor-tbps", type=float, default=6.29)
    ap.add_argument("--out", default=os.path.join("profiles", "mips", "mip_kernels_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("mip_kernels_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    lib = ctx._lib
    size = args.size // 16 if args.small else args.size
    g = torch.Generator(device="cuda")
    g.manual_seed(size)
    image = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
    layout = api.mip_layout(size, size, 4, 16, 2)
    pyramid = torch.empty(layout.pyramid_bytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def side(word):
        def run():
            rc = lib.cvttmi_build_mips_filtered_device(ctx._h, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), size, size,
                                                       size * 4, api.PIXELS_RGBA8, 2, word, stream)
            assert rc == 0, rc
        return run

    sides = {name: side(value) for name, value in api.MIP_FILTERS.items()}
    sides["box_again"] = side(api.MIP_FILTER_BOX)
    for kernel, code in api.MIP_KERNELS.items():
        sides[kernel] = side(code | api.MIP_FILTER_BOX)
        sides[kernel + "+srgb"] = side(code | api.MIP_FILTER_SRGB)
    sides["lanczos3+repeat"] = side(api.MIP_KERNELS["lanczos3"] | api.MIP_WRAPS["repeat"])
    times = alternate(torch, sides, args.reps)
    box = stats(times["box"])["us_median"]
    moved = size * size * 4 + layout.pyramid_bytes
    floor_us = moved / (args.floor_tbps * 1e6)
    results = []
    for name in sides:
        rec = {"case": "level1", "filter": name, "pixels": "rgba8", "size": size, "bytes_moved": moved, "kernel": stats(times[name])}
        rec["GBps"] = round(moved / rec["kernel"]["us_median"] / 1e3, 1)
        rec["over_box"] = round(rec["kernel"]["us_median"] / box, 4)
        rec["over_floor"] = round(rec["kernel"]["us_median"] / floor_us, 4)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    doc = {"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0), "small": bool(args.small),
           "floor_tbps": args.floor_tbps, "floor_us": round(floor_us, 2), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

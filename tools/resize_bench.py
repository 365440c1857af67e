"""Timing of the resize (include/cvtt_mi355x.h "resize") on one GPU.

    python tools/resize_bench.py [--reps 20] [--small] [--out profiles/resize/resize_bench.json]

Everything in ONE run, timed with device events as tools/mips_bench.py does (every repetition runs each side of a group once, in
turn; the median of the repetitions with the minimum and the 10th / 90th percentile beside it).  A resize call is timed whole:
the copy of its tables into the work space and its one or two launches.
  half      16384^2 -> 8192^2 under each mip kernel and the plain rule, against level 1 of cvttmi_build_mips_filtered_device with
            the same kernel -- the 2:1 kernel with its one table in scalar registers, where the general one reads a weight row per
            column and per row from memory; "over_mips" is the ratio of the medians.  The box is timed beside them, without a ratio.
  sizes     4096^2 -> 1000^2, 4000x3000 -> 4096x4096 and 16384^2 -> 512^2 under Lanczos3: absolute times and the launches each took
  layers    6 x 1024^2 -> 6 x 512^2 in one call against six calls
--small divides every size by 16 (a rehearsal of the script, not a measurement).  Prints one JSON line per side and writes them all
to --out with the library's source SHA-256."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "resize", "resize_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("resize_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    lib = ctx._lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    shrink = 16 if args.small else 1
    g = torch.Generator(device="cuda")
    g.manual_seed(1)

    def random_images(layers, h, w):
        return torch.randint(0, 256, (layers, h, w, 4), dtype=torch.uint8, device="cuda", generator=g)

    def resize_side(images, dw, dh, kernel, each_layer=False):
        """the C call on preallocated buffers (the work space included: nothing is allocated inside the timed region)"""
        n, h, w = images.shape[:3]
        word = api.resize_filter_word(kernel)
        count = 1 if each_layer else n
        need = ctypes.c_size_t(0)
        assert lib.cvttmi_resize_work_bytes(w, h, dw, dh, api.PIXELS_RGBA8, word, count, ctypes.byref(need)) == 0
        out = torch.empty((n, dh, dw, 4), dtype=torch.uint8, device="cuda")
        work = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")

        def run():
            for l in range(0, n, count):
                rc = lib.cvttmi_resize_image_device(ctx._h, out[l].data_ptr(), dw, dh, dw * 4, dw * dh * 4, images[l].data_ptr(), w, h, w * 4,
                                                    w * h * 4, api.PIXELS_RGBA8, count, word, work.data_ptr(), need.value, stream)
                assert rc == 0, rc
        return run, need.value

    def record(case, name, times, **more):
        rec = dict({"case": case, "side": name, "kernel": stats(times)}, **more)
        print(json.dumps(rec), flush=True)
        return rec

    results = []
    # ---- exactly half against the mip kernels ----
    size = 16384 // shrink
    image = random_images(1, size, size)
    layout = api.mip_layout(size, size, 4, 16, 2)
    pyramid = torch.empty(layout.pyramid_bytes, dtype=torch.uint8, device="cuda")

    def mips_side(word):
        def run():
            rc = lib.cvttmi_build_mips_filtered_device(ctx._h, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), size, size, size * 4,
                                                       api.PIXELS_RGBA8, 2, word, stream)
            assert rc == 0, rc
        return run
    sides, work_bytes = {}, {}
    for kernel, code in api.MIP_KERNELS.items():
        sides["mips " + kernel] = mips_side(code)
        sides["resize " + kernel], work_bytes[kernel] = resize_side(image, size // 2, size // 2, kernel)
    sides["resize box"], work_bytes["box"] = resize_side(image, size // 2, size // 2, "box")
    times = alternate(torch, sides, args.reps)
    for kernel in list(api.MIP_KERNELS) + ["box"]:
        launches = api.resize_launches(size, size, size // 2, size // 2, kernel)
        more = dict(source=[size, size], destination=[size // 2, size // 2], launches=launches, work_bytes=work_bytes[kernel])
        if kernel != "box":
            results.append(record("half", "mips " + kernel, times["mips " + kernel], source=[size, size]))
            more["over_mips"] = round(stats(times["resize " + kernel])["us_median"] / stats(times["mips " + kernel])["us_median"], 4)
        results.append(record("half", "resize " + kernel, times["resize " + kernel], **more))
    del sides, pyramid

    # ---- other ratios: absolute times and the path each took ----
    for (w, h), (dw, dh) in (((4096, 4096), (1000, 1000)), ((4000, 3000), (4096, 4096)), ((16384, 16384), (512, 512))):
        w, h, dw, dh = (max(1, v // shrink) for v in (w, h, dw, dh))
        source = image if (w, h) == (size, size) else random_images(1, h, w)
        run, need = resize_side(source, dw, dh, "lanczos3")
        times = alternate(torch, {"resize": run}, args.reps)
        results.append(record("sizes", "resize lanczos3", times["resize"], source=[w, h], destination=[dw, dh],
                              launches=api.resize_launches(w, h, dw, dh, "lanczos3"), work_bytes=need))
        del run, source
    del image

    # ---- layers: one call against one call per layer ----
    side = 1024 // shrink
    faces = random_images(6, side, side)
    sides = {"one call": resize_side(faces, side // 2, side // 2, "lanczos3")[0],
             "six calls": resize_side(faces, side // 2, side // 2, "lanczos3", each_layer=True)[0]}
    times = alternate(torch, sides, args.reps)
    for name in sides:
        results.append(record("layers", name, times[name], source=[side, side], destination=[side // 2, side // 2], layers=6))

    doc = {"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0), "small": bool(args.small),
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

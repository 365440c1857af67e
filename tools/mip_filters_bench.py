"""Timing of the mip filters (include/cvtt_mi355x.h "mip chains", CVTTMI_MIP_FILTER_*) on one GPU.

    python tools/mip_filters_bench.py [--reps 30] [--size 16384] [--parent-lib path/to/libcvtt_mi355x.so] [--small]
                                      [--out profiles/mips/mip_filters_bench.json] [--parent-out profiles/mips/one_path_bench.json]

The level-1 launch (cvttmi_build_mips_filtered_device with two levels) of a --size^2 RGBA8 image of random bytes under every
filter, timed with device events as tools/mips_bench.py does: every repetition runs each side once, in turn.  The sides are
the five filters, the box filter a second time ("box_again": the spread between two timings of the same launch in the same run
is the noise every ratio is read against) and, with --parent-lib, cvttmi_build_mips_device of a library built from the parent
commit, loaded beside this one in the same process ("box_parent").  "normal" is also timed for RGBA8_SNORM.
Every figure is the median of the repetitions with the minimum and the 10th / 90th percentile beside it; the ratios are medians
over the median of "box".  --small shrinks the image (a rehearsal of the script, not a measurement).  Prints one JSON line per
side and writes them all to --out with the library's source SHA-256.
With --parent-lib a second part times this library against the parent's through the one C entry both have
(cvttmi_build_mips_filtered_device), pair by pair, each pair with a repeat of this library's side beside it ("_again"): level 1 of
the --size^2 RGBA8 image under box, srgb+alpha and lanczos3, level 1 of a (--size / 2)^2 RGBA16F image under box, and the whole box
chain of a (--size / 4)^2 RGBA8 image.  A case is "within_noise" when this library's median lies at or below the parent's 90th
percentile.  Written to --parent-out with both source SHA-256."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mips_bench import alternate, stats  # noqa: E402


def parent_box(path, device):
    """(library, context handle) of another build of the library: only the entry points the parent commit already had"""
    lib = ctypes.CDLL(path)
    lib.cvttmi_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    lib.cvttmi_destroy.argtypes = [ctypes.c_void_p]
    lib.cvttmi_build_mips_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_build_mips_filtered_device.argtypes = lib.cvttmi_build_mips_device.argtypes[:-1] + [ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_source_sha256.restype = ctypes.c_char_p
    h = ctypes.c_void_p()
    rc = lib.cvttmi_create(ctypes.byref(h), device)
    if rc != 0:
        sys.exit("cvttmi_create of %s failed (%d)" % (path, rc))
    return lib, h


def against_parent(torch, api, ctx, parent, size, reps, stream):
    """[record] of the five cases of the docstring: this library and the parent's through cvttmi_build_mips_filtered_device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(size + 1)
    cases = [("level1", "box", api.PIXELS_RGBA8, size, 2), ("level1", "srgb+alpha", api.PIXELS_RGBA8, size, 2),
             ("level1", "lanczos3", api.PIXELS_RGBA8, size, 2), ("level1", "box", api.PIXELS_RGBA16F, size // 2, 2),
             ("chain", "box", api.PIXELS_RGBA8, size // 4, None)]
    results = []
    for case, name, kind, n, levels in cases:
        texel = 8 if kind == api.PIXELS_RGBA16F else 4
        if kind == api.PIXELS_RGBA16F:
            image = (torch.rand((n, n, 4), device="cuda", generator=g) * 4).half().view(torch.int16)
        else:
            image = torch.randint(0, 256, (n, n, 4), dtype=torch.uint8, device="cuda", generator=g)
        layout = api.mip_layout(n, n, texel, 16, levels)
        word = api.mip_filter_word("box", name) if name in api.MIP_KERNELS else api.MIP_FILTERS[name]
        pyramids = {}

        def side(lib, handle, key):
            pyramid = pyramids[key] = torch.zeros(layout.pyramid_bytes, dtype=torch.uint8, device="cuda")

            def run():
                rc = lib.cvttmi_build_mips_filtered_device(handle, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), n, n, n * texel,
                                                           kind, len(layout), word, stream)
                assert rc == 0, rc
            return run

        times = alternate(torch, {"this": side(ctx._lib, ctx._h, "this"), "parent": side(parent[0], parent[1], "parent"),
                                  "this_again": side(ctx._lib, ctx._h, "again")}, reps)
        this, old, again = stats(times["this"]), stats(times["parent"]), stats(times["this_again"])
        rec = {"case": case, "filter": name, "pixels": "rgba16f" if kind == api.PIXELS_RGBA16F else "rgba8", "size": n, "launches": len(layout) - 1,
               "outputs_identical": bool((pyramids["this"] == pyramids["parent"]).all().item()), "this": this, "parent": old,
               "this_again": again, "this_over_parent": round(this["us_median"] / old["us_median"], 4),
               "again_over_this": round(again["us_median"] / this["us_median"], 4), "within_noise": this["us_median"] <= old["us_p90"]}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del image, pyramids
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "mips", "mip_filters_bench.json"))
    ap.add_argument("--parent-out", default=os.path.join("profiles", "mips", "one_path_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("mip_filters_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    lib = ctx._lib
    size = args.size // 16 if args.small else args.size
    g = torch.Generator(device="cuda")
    g.manual_seed(size)
    image = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
    layout = api.mip_layout(size, size, 4, 16, 2)
    pyramid = torch.empty(layout.pyramid_bytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def side(filt, kind=api.PIXELS_RGBA8):
        def run():
            rc = lib.cvttmi_build_mips_filtered_device(ctx._h, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), size, size,
                                                       size * 4, kind, 2, filt, stream)
            assert rc == 0, rc
        return run

    sides = {name: side(value) for name, value in api.MIP_FILTERS.items()}
    sides["normal_snorm"] = side(api.MIP_FILTER_NORMAL, api.PIXELS_RGBA8_SNORM)
    sides["box_again"] = side(api.MIP_FILTER_BOX)
    parent = None
    if args.parent_lib:
        plib, ph = parent = parent_box(args.parent_lib, 0)

        def box_parent():
            rc = plib.cvttmi_build_mips_device(ph, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), size, size, size * 4,
                                               api.PIXELS_RGBA8, 2, stream)
            assert rc == 0, rc
        sides["box_parent"] = box_parent
    times = alternate(torch, sides, args.reps)
    box = stats(times["box"])["us_median"]
    results = []
    for name in sides:
        rec = {"case": "level1", "filter": name, "pixels": "rgba8_snorm" if name == "normal_snorm" else "rgba8", "size": size,
               "bytes_moved": size * size * 4 + layout.pyramid_bytes, "kernel": stats(times[name])}
        rec["GBps"] = round(rec["bytes_moved"] / rec["kernel"]["us_median"] / 1e3, 1)
        rec["over_box"] = round(rec["kernel"]["us_median"] / box, 4)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    doc = {"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0), "small": bool(args.small),
           "results": results}
    if parent:
        doc["parent_library_source_sha256"] = (parent[0].cvttmi_source_sha256() or b"").decode()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    if parent:
        del image, pyramid
        torch.cuda.empty_cache()
        doc["results"] = against_parent(torch, api, ctx, parent, size, args.reps, stream)
        parent[0].cvttmi_destroy(parent[1])
        os.makedirs(os.path.dirname(os.path.abspath(args.parent_out)), exist_ok=True)
        with open(args.parent_out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

"""Timing of RGBA16F under the mip kernels and in a resize (include/cvtt_mi355x.h, "RGBA16F under a kernel") on one GPU.

    python tools/hdr_resample_bench.py [--reps 30] [--small] [--parent-lib PATH] [--out profiles/hdr/hdr_resample_bench.json]

Everything in ONE run, timed with device events as tools/mips_bench.py does: every repetition runs each side once, in turn; every
figure is the median of the repetitions with the minimum and the 10th / 90th percentile beside it.
  level1    the level-1 launch (cvttmi_build_mips_filtered_device with two levels) of an 8192^2 RGBA16F image under each kernel
            (NONNEGATIVE; Lanczos3 under SIGNED as well), beside (a) the RGBA16F 2x2 box of the same image ("box", and "box_again",
            the noise every ratio is read against) and (b) the RGBA8 plain rule of the same kernel at 16384^2 -- the same bytes read
            (and half the bytes written).  "over_box" and "over_rgba8" are ratios of medians; "rate_over_box" is this side's bytes
            moved / time over the box's: the box is pure HBM traffic, so a side near its rate is bound by HBM and one far below it
            by VALU issue ("bound", the line drawn at 0.8).
  resize    8192^2 -> 4096^2 and 4096^2 -> 1000^2 under Lanczos3, a call timed whole (the copy of its tables and its launches)
  scratch   the private segment of every RGBA16F resample kernel in the library's code object (must be 0), with its registers
--parent-lib: a build of the parent commit's library.  The RGBA8 legs of tools/mip_kernels_bench.py and tools/resize_bench.py are
then run in child processes with that library and with this one, alternating (parent, this, parent, this), and the medians of both
are written side by side: the integer kernels are meant to time as they did.
--small divides every size by 16 (a rehearsal of the script, not a measurement)."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from mips_bench import alternate, stats  # noqa: E402


def kernel_resources(lib_path, llvm="/opt/rocm/llvm/bin"):
    """{kernel name: {scratch, vgprs, sgprs, lds}} of the RGBA16F resample kernels, from the metadata of the library's gfx950 code
    object; {} where the tools to read it are missing"""
    try:
        with tempfile.TemporaryDirectory() as d:
            fat, one, co = os.path.join(d, "fat.bin"), os.path.join(d, "one.bin"), os.path.join(d, "dev.co")
            subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, fat])
            raw, magic, notes = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", ""
            starts = [m.start() for m in re.finditer(magic, raw)]  # one bundle per translation unit
            for a, b in zip(starts, starts[1:] + [len(raw)]):
                open(one, "wb").write(raw[a:b])
                subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                       "--input=" + one, "--output=" + co, "--unbundle"])
                notes += subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co]).decode()
    except (OSError, subprocess.CalledProcessError):
        return {}
    found, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(name|private_segment_fixed_size|vgpr_count|sgpr_count|group_segment_fixed_size):\s+(\S+)", line)
        if m:
            cur[m.group(1)] = m.group(2)
        if line.strip().startswith(".wavefront_size:"):
            if "_half_" in cur.get("name", ""):
                short = re.search(r"cvttmi_\w+?_half_\w*?kernel(ILi\d+E)?", cur["name"])
                found[short.group(0) if short else cur["name"]] = {
                    "scratch_bytes": int(cur.get("private_segment_fixed_size", -1)), "vgprs": int(cur.get("vgpr_count", -1)),
                    "sgprs": int(cur.get("sgpr_count", -1)), "static_lds_bytes": int(cur.get("group_segment_fixed_size", -1))}
            cur = {}
    return found


def rgba8_legs(parent_lib, reps, small):
    """medians of the RGBA8 sides of the two older tools under the parent's library and this one, runs alternating"""
    runs = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as d:
        for turn in range(2):
            for who in ("parent", "this"):
                env = dict(os.environ)
                env.pop("CVTTMI_LIB", None)
                if who == "parent":
                    env["CVTTMI_LIB"] = parent_lib
                got = {}
                for tool, key in (("mip_kernels_bench.py", "filter"), ("resize_bench.py", "side")):
                    out = os.path.join(d, "%s_%d_%s.json" % (who, turn, tool))
                    cmd = [sys.executable, os.path.join(HERE, tool), "--reps", str(reps), "--out", out] + (["--small"] if small else [])
                    subprocess.check_call(cmd, env=env, stdout=subprocess.DEVNULL)
                    doc = json.load(open(out))
                    for rec in doc["results"]:
                        name = "%s: %s %s" % (tool[:-3], rec["case"], rec[key])
                        if "source" in rec and rec["case"] == "sizes":
                            name += " %dx%d" % tuple(rec["source"])
                        got[name] = rec["kernel"]["us_median"]
                    got["library_source_sha256"] = doc["library_source_sha256"]
                runs[who].append(got)
    sides = [k for k in runs["this"][0] if k != "library_source_sha256"]
    table = {k: {"parent_us": [r[k] for r in runs["parent"]], "this_us": [r[k] for r in runs["this"]]} for k in sides}
    for rec in table.values():
        rec["this_over_parent"] = round(sum(rec["this_us"]) / sum(rec["parent_us"]), 4)
    return {"order": "parent, this, parent, this; medians of %d repetitions each, microseconds" % reps,
            "parent_library_source_sha256": runs["parent"][0]["library_source_sha256"], "sides": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "hdr", "hdr_resample_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("hdr_resample_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    lib = ctx._lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    shrink = 16 if args.small else 1
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    HALF, RGBA8 = api.PIXELS_RGBA16F, api.PIXELS_RGBA8

    def radiance(h, w):
        """log-normal HDR values, finite halfs"""
        return torch.exp(torch.randn((h, w, 4), device="cuda", generator=g) * 2.0).clamp_(max=65504.0).half()

    def mips_side(image, kind, word):
        h, w = image.shape[:2]
        texel = 8 if kind == HALF else 4
        layout = api.mip_layout(w, h, texel, 16, 2)
        pyramid = torch.empty(layout.pyramid_bytes, dtype=torch.uint8, device="cuda")

        def run():
            rc = lib.cvttmi_build_mips_filtered_device(ctx._h, pyramid.data_ptr(), layout.pyramid_bytes, image.data_ptr(), w, h, w * texel, kind, 2,
                                                       word, stream)
            assert rc == 0, rc
        return run, w * h * texel + layout.pyramid_bytes

    results = []
    # ---- level 1 ----
    size = 8192 // shrink
    half_image = radiance(size, size)
    byte_image = torch.randint(0, 256, (2 * size, 2 * size, 4), dtype=torch.uint8, device="cuda", generator=g)
    sides, moved = {}, {}
    NONNEG, SIGNED = api.MIP_HDR["nonnegative"], api.MIP_HDR["signed"]
    sides["f16 box"], moved["f16 box"] = mips_side(half_image, HALF, api.MIP_FILTER_BOX)
    sides["f16 box_again"], moved["f16 box_again"] = mips_side(half_image, HALF, api.MIP_FILTER_BOX)
    for kernel, code in api.MIP_KERNELS.items():
        sides["f16 " + kernel], moved["f16 " + kernel] = mips_side(half_image, HALF, code | NONNEG)
        sides["rgba8 " + kernel], moved["rgba8 " + kernel] = mips_side(byte_image, RGBA8, code)
    sides["f16 lanczos3 signed"], moved["f16 lanczos3 signed"] = mips_side(half_image, HALF, api.MIP_KERNELS["lanczos3"] | SIGNED)
    times = alternate(torch, sides, args.reps)
    box_us = stats(times["f16 box"])["us_median"]
    box_rate = moved["f16 box"] / box_us
    for name in sides:
        rec = {"case": "level1", "side": name, "size": 2 * size if name.startswith("rgba8") else size, "bytes_moved": moved[name],
               "kernel": stats(times[name])}
        us = rec["kernel"]["us_median"]
        rec["GBps"] = round(moved[name] / us / 1e3, 1)
        rec["over_box"] = round(us / box_us, 4)
        if name.startswith("f16 ") and name.split()[1] in api.MIP_KERNELS:
            rec["over_rgba8"] = round(us / stats(times["rgba8 " + name.split()[1]])["us_median"], 4)
            rec["rate_over_box"] = round(moved[name] / us / box_rate, 4)
            rec["bound"] = "HBM" if rec["rate_over_box"] >= 0.8 else "VALU issue"
        print(json.dumps(rec), flush=True)
        results.append(rec)
    del sides, byte_image

    # ---- resize ----
    for (w, h), (dw, dh) in (((8192, 8192), (4096, 4096)), ((4096, 4096), (1000, 1000))):
        w, h, dw, dh = (max(1, v // shrink) for v in (w, h, dw, dh))
        source = half_image if (w, h) == (size, size) else radiance(h, w)
        word = api.resize_filter_word("lanczos3", hdr="nonnegative")
        need = ctypes.c_size_t(0)
        assert lib.cvttmi_resize_work_bytes(w, h, dw, dh, HALF, word, 1, ctypes.byref(need)) == 0
        out = torch.empty((dh, dw, 4), dtype=torch.float16, device="cuda")
        work = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")

        def run():
            rc = lib.cvttmi_resize_image_device(ctx._h, out.data_ptr(), dw, dh, dw * 8, dw * dh * 8, source.data_ptr(), w, h, w * 8, w * h * 8,
                                                HALF, 1, word, work.data_ptr(), need.value, stream)
            assert rc == 0, rc
        t = alternate(torch, {"resize": run}, args.reps)
        launches = api.resize_launches(w, h, dw, dh, "lanczos3", hdr="nonnegative")
        bytes_moved = w * h * 8 + dw * dh * 8 + (0 if launches == 1 else 2 * h * dw * 16)
        rec = {"case": "resize", "side": "f16 lanczos3", "source": [w, h], "destination": [dw, dh], "launches": launches, "work_bytes": need.value,
               "bytes_moved": bytes_moved, "kernel": stats(t["resize"])}
        rec["GBps"] = round(bytes_moved / rec["kernel"]["us_median"] / 1e3, 1)
        rec["rate_over_box"] = round(bytes_moved / rec["kernel"]["us_median"] / box_rate, 4)
        rec["bound"] = "HBM" if rec["rate_over_box"] >= 0.8 else "VALU issue"
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del run, source, out, work
    del half_image
    torch.cuda.empty_cache()

    lib_path = os.environ.get("CVTTMI_LIB", api._LIB_PATH)
    resources = kernel_resources(lib_path)
    doc = {"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0), "small": bool(args.small),
           "results": results, "kernel_resources": resources if resources else "not measured",
           "scratch_bytes_max": max(r["scratch_bytes"] for r in resources.values()) if resources else "not measured"}
    if args.parent_lib:
        doc["rgba8_legs_against_parent"] = rgba8_legs(os.path.abspath(args.parent_lib), max(5, args.reps // 2), args.small)
    else:
        doc["rgba8_legs_against_parent"] = "not measured (no --parent-lib)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: doc[k] for k in ("scratch_bytes_max", "rgba8_legs_against_parent")}), flush=True)


if __name__ == "__main__":
    main()

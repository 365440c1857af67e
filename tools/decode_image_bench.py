"""Timing of decoding into images (include/cvtt_mi355x.h "decoding into images", Context.decode_image / decode_mips) on one GPU.

    python tools/decode_image_bench.py [--reps 30] [--small] [--out profiles/decode_image/decode_image_bench.json]

1. cvttmi_decode_image_device at 4096^2 and 16384^2 for bc1, bc7, etc2rgba (RGBA8 images) and bc6hu (RGBA16F), timed with
   device events, against two yardsticks taken in the same run, the three sides alternating:
     copy    a device-to-device hipMemcpyAsync of as many bytes as the image has (what merely writing the output costs, with
             a read of the same size on top: the decoder reads 1/8 or 1/4 of that)
     parent  the only route to the image before this call: pad the blocks to a multiple of eight, Context.decode into
             PixelBlocks, untile with a torch permute, crop, make contiguous
   The packed blocks are real: a 4096^2 noise image encoded by Context.encode_image (16384^2: those blocks repeated 4 x 4).
   The outputs of the new call and of the parent's route are compared as well.
2. A 13-level 4096^2 chain for bc1 and bc7 (Context.encode_mips of the noise image): cvttmi_decode_mips_device, one launch,
   against one cvttmi_decode_image_device per level into the same buffers.
3. --block-decode: nothing of the above, only cvttmi_decode_device (the decode inside "parent", without the untiling) on 2^20
   random blocks of bc7, bc6hu and bc6hs, every sample kept: one process measures one build of the library (CVTTMI_LIB), so an
   A/B of two builds alternates processes (profiles/decode/one_kernel_bench.json).
Every figure is the median of the repetitions with the minimum and the 10th / 90th percentile beside it.  --small shrinks
every size by 16 (a rehearsal of the script, not a measurement).  Prints one JSON line per case and writes them all to --out
with the library's source SHA-256."""
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


def source_image(torch, fmt, size):
    g = torch.Generator(device="cuda")
    g.manual_seed(size)
    if fmt == "bc6hu":
        return (torch.rand((size, size, 4), device="cuda", generator=g) * 4).half()
    return torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)


def image_case(torch, api, ctx, hip, fmt, base, packed_base, size, reps):
    """packed_base: the blocks of a base^2 image; size: a multiple of base"""
    lib = ctx._lib
    fid, bpb = api.TEXTURE_FORMATS[fmt][:2]
    hdr = fmt == "bc6hu"
    texel, dtype = (8, torch.float16) if hdr else (4, torch.uint8)
    k, bw = size // base, size // 4
    packed = packed_base.view(base // 4, base // 4, bpb).repeat(k, k, 1).reshape(-1, bpb).contiguous()
    n = bw * bw
    out = torch.empty((size, size, 4), dtype=dtype, device="cuda")
    src = torch.empty_like(out)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = {}

    def new():
        rc = lib.cvttmi_decode_image_device(ctx._h, fid, out.data_ptr(), size * texel, 1 if hdr else 0, packed.data_ptr(), size, size, stream)
        assert rc == 0, rc

    def copy():
        rc = hip.hipMemcpyAsync(out.data_ptr(), src.data_ptr(), size * size * texel, 3, stream)  # 3 = hipMemcpyDeviceToDevice
        assert rc == 0, rc

    def parent():
        pad = (-n) % 8
        p = torch.cat([packed, packed.new_zeros((pad, bpb))]) if pad else packed
        blocks = ctx.decode(fmt, p)[:n]
        keep["parent"] = blocks.view(bw, bw, 4, 4, 4).permute(0, 2, 1, 3, 4).reshape(bw * 4, bw * 4, 4)[:size, :size].contiguous()

    t = alternate(torch, {"decode_image": new, "copy": copy, "parent_route": parent}, reps)
    new()
    torch.cuda.synchronize()
    same = bool(torch.equal(out.view(torch.int16) if hdr else out, keep["parent"]))
    rec = {"case": "image", "format": fmt, "size": size, "image_bytes": size * size * texel, "packed_bytes": n * bpb,
           "outputs_identical": same, "decode_image": stats(t["decode_image"]), "copy_same_bytes": stats(t["copy"]),
           "parent_route": stats(t["parent_route"])}
    rec["decode_image_GBps_written"] = round(rec["image_bytes"] / rec["decode_image"]["us_median"] / 1e3, 1)
    rec["decode_image_over_copy_time"] = round(rec["decode_image"]["us_median"] / rec["copy_same_bytes"]["us_median"], 3)
    rec["parent_over_decode_image_time"] = round(rec["parent_route"]["us_median"] / rec["decode_image"]["us_median"], 2)
    return rec


def chain_case(torch, api, ctx, fmt, size, reps):
    lib = ctx._lib
    fid, bpb = api.TEXTURE_FORMATS[fmt][:2]
    levels = ctx.encode_mips(fmt, source_image(torch, fmt, size))
    layout = api.mip_layout(size, size, 4, bpb)
    assert levels[0].data_ptr() + layout[-1].packedByteOffset == levels[-1].data_ptr()  # consecutive, as encode_mips returns them
    image = torch.empty((size, size, 4), dtype=torch.uint8, device="cuda")
    pyramids = {name: torch.zeros(layout.pyramid_bytes, dtype=torch.uint8, device="cuda") for name in ("decode_mips", "per_level")}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def one_launch():
        rc = lib.cvttmi_decode_mips_device(ctx._h, fid, image.data_ptr(), size * 4, pyramids["decode_mips"].data_ptr(), layout.pyramid_bytes, 0,
                                           levels[0].data_ptr(), size, size, len(layout), stream)
        assert rc == 0, rc

    def per_level():
        for L, blocks in zip(layout, levels):
            dst = image.data_ptr() if L is layout[0] else pyramids["per_level"].data_ptr() + L.byteOffset
            rc = lib.cvttmi_decode_image_device(ctx._h, fid, dst, L.width * 4, 0, blocks.data_ptr(), L.width, L.height, stream)
            assert rc == 0, rc

    t = alternate(torch, {"decode_mips": one_launch, "per_level": per_level}, reps)
    rec = {"case": "chain", "format": fmt, "size": size, "levels": len(layout),
           "outputs_identical": bool(torch.equal(pyramids["decode_mips"], pyramids["per_level"])),
           "decode_mips": stats(t["decode_mips"]), "decode_image_per_level": stats(t["per_level"])}
    rec["decode_mips_over_per_level_time"] = round(rec["decode_mips"]["us_median"] / rec["decode_image_per_level"]["us_median"], 3)
    return rec


def block_decode_case(torch, api, ctx, fmt, n, reps, warmup=5):
    """cvttmi_decode_device alone (what Context.decode calls, the "parent_route" above without its untiling): n random blocks
    -> decoded blocks, device events around each call; every sample is kept"""
    fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
    g = torch.Generator(device="cuda")
    g.manual_seed(fid)
    packed = torch.randint(0, 256, (n, bpb), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty(n * tex, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def decode():
        rc = ctx._lib.cvttmi_decode_device(ctx._h, fid, out.data_ptr(), packed.data_ptr(), n, stream)
        assert rc == 0, rc

    us = alternate(torch, {"decode": decode}, reps, warmup)["decode"]
    rec = {"case": "block_decode", "format": fmt, "blocks": n, "samples_us": [round(t, 2) for t in us]}
    rec.update(stats(us))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--block-decode", action="store_true",
                    help="only the block decode of bc7 / bc6hu / bc6hs at 2^20 blocks (the library: CVTTMI_LIB, for an A/B of two builds)")
    ap.add_argument("--out", default=os.path.join("profiles", "decode_image", "decode_image_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("decode_image_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    if args.block_decode:
        results = [block_decode_case(torch, api, ctx, fmt, (1 << 20) // (256 if args.small else 1), args.reps) for fmt in ("bc7", "bc6hu", "bc6hs")]
        for rec in results:
            print(json.dumps({k: v for k, v in rec.items() if k != "samples_us"}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0),
                       "small": bool(args.small), "results": results}, f, indent=1)
        return
    # the HIP runtime this process already has mapped (one runtime per process: api.load_library)
    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    shrink = 16 if args.small else 1
    base = 4096 // shrink
    results = []
    for fmt in ("bc1", "bc7", "etc2rgba", "bc6hu"):
        packed = ctx.encode_image(fmt, source_image(torch, fmt, base))
        torch.cuda.synchronize()
        for size in (4096 // shrink, 16384 // shrink):
            rec = image_case(torch, api, ctx, hip, fmt, base, packed, size, args.reps)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            torch.cuda.empty_cache()
    for fmt in ("bc1", "bc7"):
        rec = chain_case(torch, api, ctx, fmt, base, args.reps)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0),
                   "small": bool(args.small), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()

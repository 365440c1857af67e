"""Timing of texture arrays and cube maps (include/cvtt_mi355x.h "texture arrays and cube maps") on one GPU.

    python tools/texture_array_bench.py [--reps 30] [--small] [--out profiles/texture_array/texture_array_bench.json]

Two sides per shape, timed with device events as tools/mips_bench.py does (every repetition runs each side once, in turn):
  "texture"    Context.encode_texture: one C call for all layers and levels
  "per_layer"  the route there was before it: Context.encode_mips per layer, then one torch.cat into container order
Before anything is timed the two sides' outputs are compared byte for byte.  Shapes:
  (a) a cube, 6 x 1024^2, BC7, full chain, level-major (KTX order)
  (b) 256 x 64^2, BC1, full chain, layer-major (DDS order)
  (c) 1 x 4096^2, BC1 and BC7, full chain
  (d) Context.build_mips_array alone against Context.build_mips per layer, for the images of (a) and (b)
Every figure is the median of the repetitions with the minimum and the 10th / 90th percentile beside it.  "faster": the new
side's median lies below the old side's 10th percentile -- asked of (a), (b), (d); "not_slower": that, or each median inside the
other side's 10th-90th range -- asked of (c).  --small shrinks the shapes (a rehearsal of the script, not a measurement).  Prints
one JSON line per case and writes them all to --out with the library's source SHA-256."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mips_bench import alternate, stats  # noqa: E402


def verdicts(new, old):
    faster = new["us_median"] < old["us_p10"]
    inside = old["us_p10"] <= new["us_median"] <= old["us_p90"] and new["us_p10"] <= old["us_median"] <= new["us_p90"]
    return {"faster": bool(faster), "not_slower": bool(faster or inside or new["us_median"] <= old["us_median"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "texture_array", "texture_array_bench.json"))
    args = ap.parse_args()
    import torch
    from convectionkernels_amd import api
    if not torch.cuda.is_available():
        sys.exit("texture_array_bench needs an MI355X: nothing is measured without one")
    ctx = api.Context(0)
    shrink = 8 if args.small else 1
    g = torch.Generator(device="cuda")
    g.manual_seed(20)

    def images(layers, size):
        # random RGBA bytes, the content of tools/mips_bench.py's chain case (the 0.66 / 4.21 ms figures of a 4096^2 chain)
        return torch.randint(0, 256, (layers, size, size, 4), dtype=torch.uint8, device="cuda", generator=g)

    def encode_case(name, fmt, layers, size, order, want):
        size = max(4, size // shrink)
        imgs = images(layers, size)

        def texture():
            return ctx.encode_texture(fmt, imgs, order=order)

        def per_layer():
            chains = [ctx.encode_mips(fmt, imgs[l]) for l in range(layers)]
            if order == "layer":
                return torch.cat([t for chain in chains for t in chain])
            return torch.cat([chain[L] for L in range(len(chains[0])) for chain in chains])

        a, b = texture().base, per_layer()
        torch.cuda.synchronize()
        if not (a.shape == b.shape and bool((a == b).all())):
            sys.exit("%s: encode_texture and the per-layer route disagree" % name)
        t = alternate(torch, {"texture": texture, "per_layer": per_layer}, args.reps)
        rec = {"case": name, "format": fmt, "layers": layers, "size": size, "order": order, "levels": api.mip_level_count(size, size),
               "blocks": int(a.shape[0]), "texture": stats(t["texture"]), "per_layer": stats(t["per_layer"]), "asked": want}
        return finish(rec, "texture", "per_layer")

    def mips_case(name, layers, size, want):
        size = max(4, size // shrink)
        imgs = images(layers, size)

        def array():
            return ctx.build_mips_array(imgs)

        def per_layer():
            return [ctx.build_mips(imgs[l]) for l in range(layers)]

        a, b = array(), per_layer()
        torch.cuda.synchronize()
        if not all(bool((x == y).all()) for ca, cb in zip(a, b) for x, y in zip(ca, cb)):
            sys.exit("%s: build_mips_array and the per-layer route disagree" % name)
        t = alternate(torch, {"array": array, "per_layer": per_layer}, args.reps)
        rec = {"case": name, "layers": layers, "size": size, "levels": api.mip_level_count(size, size), "array": stats(t["array"]),
               "per_layer": stats(t["per_layer"]), "asked": want}
        return finish(rec, "array", "per_layer")

    def finish(rec, new, old):
        rec.update(verdicts(rec[new], rec[old]))
        rec["ratio"] = round(rec[new]["us_median"] / rec[old]["us_median"], 4)
        rec["met"] = rec[rec["asked"]]
        print(json.dumps(rec), flush=True)
        return rec

    results = [
        encode_case("a_cube_6x1024_bc7", "bc7", 6, 1024, "level", "faster"),
        encode_case("b_array_256x64_bc1", "bc1", 256, 64, "layer", "faster"),
        encode_case("c_single_4096_bc1", "bc1", 1, 4096, "layer", "not_slower"),
        encode_case("c_single_4096_bc7", "bc7", 1, 4096, "layer", "not_slower"),
        mips_case("d_mips_6x1024", 6, 1024, "faster"),
        mips_case("d_mips_256x64", 256, 64, "faster"),
    ]
    doc = {"library_source_sha256": api.library_source_sha256(), "device": torch.cuda.get_device_name(0), "small": bool(args.small),
           "reps": args.reps, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

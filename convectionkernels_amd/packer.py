"""Image -> compressed texture file on the MI355X: the caller side of the hot path.

    python -m convectionkernels_amd.packer [-format F] [-uniform] [-fakebt709] [-quality Q] [-dds] [-mips] [-mipfilter box|srgb|normal] [-mipkernel triangle|mitchell|lanczos3|kaiser] [-wrap clamp|repeat|mirror] [-alphaweight] [-srgb] [-metrics] [-array | -cube] [-resize WxH | -maxsize N | -pow2 nearest|up|down] [-resizekernel box|triangle|mitchell|lanczos3|kaiser] [-resizerule box|srgb|normal] [-resizewrap clamp|repeat|mirror] input [input ...] output

The command line follows the reference's example packer (etc2packer.cpp:44-105: `-format etc1|etc2rgb|etc2rgba|etc2punchthrough|r11u|r11s`,
`-fakebt709`, `-uniform` (which overrides it), input, output; default etc2rgb, KTX output) and adds the BC formats (bc1..bc5, bc7; `-dds` for a DX10 DDS
file, `-quality 1..100` for a BC7 plan).  The image is uploaded once; tiling into groups of eight 4x4 blocks with
edge clamping (etc2packer.cpp:215-248), encoding and the removal of padding blocks all run on the device, and the
packed blocks are already in container order.  The input is anything PIL opens, or a .npy of shape (H, W, 4) uint8.
-format bc6hu|bc6hs: the input is a .npy of shape (H, W, 4) -- (L, H, W, 4) with -array / -cube --, float16, or float32, which is
clamped to +-65504 and rounded to nearest even; non-finite values and every other input are refused.  Under -mipkernel and the
resize flags such an image is filtered in float32 and the results are clamped to the format's range (Context.build_mips's hdr):
bc6hu "nonnegative" [+0, 65504], bc6hs "signed" [-65504, 65504].  With -metrics BC6H prints the MSE; it has no PSNR (nan).
-metrics: after the file is written, print the encoding error to stdout, measured on the device against the input image
(Context.measure_image: one line per measured channel with its MSE and PSNR, then the PSNR over all of them; R11 has no
image form and is measured over the written blocks against their tiles, the clamped texels of the edge blocks included).
-mips: the file holds the full mip chain down to 1x1 (Context.encode_mips: 2x2 box filter on the device, floor convention, every
level from the rounded one before it, all levels searched by one encode call).  With -metrics the lines of level 0 come first,
unchanged, then one line per further level: its PSNR over the format's channels against that level's own image.  Not for
R11, which has no image form.
-mipfilter box|srgb|normal, -alphaweight: the filter of the chain (Context.build_mips: "srgb" averages colour in linear light,
"normal" renormalises a normal map, -alphaweight weights colour by alpha -- with box or srgb); either implies -mips.
-mipkernel triangle|mitchell|lanczos3|kaiser: every level is filtered with that kernel (4, 8 or 12 taps per direction) instead of the
2x2 rule, under -mipfilter box (the default), srgb or normal; implies -mips.  Not with -alphaweight; bc6h: box only.  -wrap
clamp|repeat|mirror: how the kernel's taps leave the image (repeat: a tiling texture); only with -mipkernel.
-srgb: the file carries the sRGB code of its format (container.SRGB_FORMATS).  Only a mark: level 0 and the encode are unchanged.
-array: every input is one layer of a texture array (N inputs, then the output); -cube: the inputs are the faces of a cube in the
order +X -X +Y -Y +Z -Z, or of a cube array (6 n inputs).  Either also takes a single .npy of shape (L, H, W, 4).  All layers
must be of one size, a cube's faces square.  The layers go through one call (Context.encode_texture) and into one KTX (level-major)
or, with -dds, DDS (layer-major) file that a loader binds as an array or a cube; combines with -mips, -mipfilter, -alphaweight,
-srgb and -quality.  With -metrics the lines above are printed for every layer under a `layer N` heading.  Not for R11.
-resize WxH, -maxsize N, -pow2 nearest|up|down (one of them): the image -- every layer of -array / -cube in one call -- is resized on
the device (Context.resize) before anything else; -mips, -metrics and the container header see the new size.  -maxsize: the larger
side becomes at most N, the aspect kept, each side max(1, floor(side * N / larger + 0.5)); never enlarges.  -pow2: each side on its own
to the next power of two up, down, or the nearer of the two (the larger one from the middle on).  -resizekernel (default lanczos3; box is
an area average), -resizerule box|srgb|normal (default box: the plain rule) and -resizewrap (default clamp) say how, and go only with
one of the three.  Sizes are 1 .. 65535.  bc6hu / bc6hs: -resizerule box only.  -mipfilter srgb|normal and -alphaweight are not for
bc6hu / bc6hs either."""
import re
import sys

import numpy as np

from . import api, container

USAGE = __doc__.split("\n\n")[1]


def load_rgba8(path):
    if path.endswith(".npy"):
        img = np.load(path)
    else:
        from PIL import Image  # only needed for image files
        img = np.array(Image.open(path).convert("RGBA"))
    if img.ndim != 3 or img.shape[2] != 4 or img.dtype != np.uint8:
        raise ValueError("expected an (H, W, 4) uint8 image, got %s %s" % (img.shape, img.dtype))
    return np.ascontiguousarray(img)


HALF_FORMATS = {"bc6hu": "nonnegative", "bc6hs": "signed"}  # the formats encoded from RGBA16F images, and their range (api.MIP_HDR)


def load_rgba16f(path, fmt, ndim=3):
    """the image of a half-float format: a .npy of `ndim` dimensions, float16 or float32 -> float16; anything else is a ValueError that
    names the format"""
    shape = "(H, W, 4)" if ndim == 3 else "(L, H, W, 4)"
    if not path.endswith(".npy"):
        raise ValueError("%s is encoded from a float16 or float32 .npy of shape %s, got %s" % (fmt, shape, path))
    img = np.load(path)
    if img.ndim != ndim or img.shape[-1] != 4 or 0 in img.shape or img.dtype not in (np.float16, np.float32):
        raise ValueError("%s is encoded from a float16 or float32 .npy of shape %s, got %s %s" % (fmt, shape, img.shape, img.dtype))
    if not np.isfinite(img).all():
        raise ValueError("%s: the image holds non-finite values (NaN or infinity)" % fmt)
    if img.dtype == np.float32:
        img = np.clip(img, np.float32(-65504.0), np.float32(65504.0)).astype(np.float16)  # (astype rounds to nearest even)
    return np.ascontiguousarray(img)


def r11_blocks(img, signed):
    """PixelBlockScalarS16 tiles of the RGB average exactly as etc2packer.cpp:236-241 computes them (including its
    use of the *unsigned* normalised value, scaled by 1023, for the signed format), groups of 8 blocks, edges clamped."""
    h, w = img.shape[:2]
    bw, bh = (w + 3) // 4, (h + 3) // 4
    gw = (bw + 7) // 8 * 8
    ys = np.minimum(np.arange(bh * 4), h - 1)
    xs = np.minimum(np.arange(gw * 4), w - 1)
    total = img[ys][:, xs, :3].astype(np.float64).sum(axis=2)
    normalized = total / (255.0 * 3.0)
    values = np.floor(normalized * (1023.0 if signed else 2047.0) + 0.5).astype(np.int16)
    return values.reshape(bh, 4, gw, 4).transpose(0, 2, 1, 3).reshape(bh * gw, 16), bw, bh, gw


def encode_file(image, fmt, options=None, plan=None, ctx=None):
    """(H, W, 4) uint8 numpy image -> packed blocks (ceil(H/4) * ceil(W/4), bytesPerBlock) uint8, container order."""
    import torch
    ctx = ctx or api.default_context()
    fmt = container.canonical(fmt)
    h, w = image.shape[:2]
    if fmt in ("r11u", "r11s"):
        blocks, bw, bh, gw = r11_blocks(image, fmt == "r11s")
        packed = ctx.encode_etc2_alpha11(blocks, signed=(fmt == "r11s"), options=options)
        return np.asarray(packed).reshape(bh, gw, 8)[:, :bw].reshape(-1, 8)
    dev = torch.from_numpy(image).cuda(ctx.device)
    packed = ctx.encode_image(fmt, dev, options, plan)
    torch.cuda.synchronize(ctx.device)
    return packed.cpu().numpy()


def encode_file_mips(image, fmt, options=None, plan=None, ctx=None, mip_filter="box", kernel=None, wrap="clamp", hdr=None):
    """(H, W, 4) uint8 (BC6H: float16) numpy image -> [packed blocks of level L], the full chain, container order (not R11)"""
    import torch
    ctx = ctx or api.default_context()
    levels = ctx.encode_mips(container.canonical(fmt), torch.from_numpy(image).cuda(ctx.device), options, plan, mip_filter=mip_filter,
                             kernel=kernel, wrap=wrap, hdr=hdr)
    torch.cuda.synchronize(ctx.device)
    return [level.cpu().numpy() for level in levels]


def measure_file_mips(image, fmt, levels, ctx=None, mip_filter="box", kernel=None, wrap="clamp", hdr=None):
    """[ErrorReport of level L against its own image] for the levels encode_file_mips returned, level 0 left out"""
    import torch
    ctx = ctx or api.default_context()
    fmt = container.canonical(fmt)
    images = ctx.build_mips(torch.from_numpy(np.ascontiguousarray(image)).cuda(ctx.device), len(levels), signed=fmt in ("bc4s", "bc5s"),
                            filter=mip_filter, kernel=kernel, wrap=wrap, hdr=hdr)
    return [ctx.measure_image(fmt, img, torch.from_numpy(np.ascontiguousarray(packed)).cuda(ctx.device))
            for img, packed in zip(images[1:], levels[1:])]


def measure_file(image, fmt, packed, options=None, ctx=None):
    """ErrorReport of the packed blocks encode_file returned for `image`"""
    import torch
    ctx = ctx or api.default_context()
    fmt = container.canonical(fmt)
    if fmt in ("r11u", "r11s"):
        # the written blocks (ceil(W/4) of each group-padded row) against their tiles; the packed count need not be a
        # multiple of 8, so the measure runs over whole groups and only the written blocks' values are added up
        tiles, bw, bh, gw = r11_blocks(image, fmt == "r11s")
        tiles = tiles.reshape(bh, gw, 16)[:, :bw].reshape(-1, 16)
        n = len(tiles)
        pad = (-n) % api.NumParallelBlocks
        src = np.concatenate([tiles, np.repeat(tiles[-1:], pad, axis=0)])
        bc = np.concatenate([np.asarray(packed, np.uint8).reshape(-1, 8), np.repeat(np.asarray(packed, np.uint8).reshape(-1, 8)[-1:], pad, axis=0)])
        rep = ctx.measure_error(fmt, src, bc, per_block=True)
        totals = api.ErrorTotals()
        totals.format, totals.channelMask, totals.texels = rep.totals.format, rep.totals.channelMask, 16 * n
        totals.sse[0] = int(rep.per_block[:n].astype(np.uint64).sum())
        return api.ErrorReport(fmt, totals, rep.per_block[:n])
    dev = torch.from_numpy(np.ascontiguousarray(image)).cuda(ctx.device)
    return ctx.measure_image(fmt, dev, torch.from_numpy(np.ascontiguousarray(packed)).cuda(ctx.device))


def load_layers(paths, fmt=None):
    """the inputs of -array / -cube -> (L, H, W, 4) uint8 (a format of HALF_FORMATS: float16): one image per path, or a single .npy of
    that shape"""
    if fmt in HALF_FORMATS:
        if len(paths) == 1 and paths[0].endswith(".npy") and np.load(paths[0], mmap_mode="r").ndim == 4:
            return load_rgba16f(paths[0], fmt, 4)
        images = [load_rgba16f(p, fmt) for p in paths]
    elif len(paths) == 1 and paths[0].endswith(".npy"):
        stack = np.load(paths[0])
        if stack.ndim == 4:
            if stack.shape[0] < 1 or stack.shape[3] != 4 or stack.dtype != np.uint8:
                raise ValueError("expected an (L, H, W, 4) uint8 array, got %s %s" % (stack.shape, stack.dtype))
            return np.ascontiguousarray(stack)
        images = [load_rgba8(p) for p in paths]
    else:
        images = [load_rgba8(p) for p in paths]
    for p, img in zip(paths, images):
        if img.shape != images[0].shape:
            raise ValueError("all layers must be of one size: %s is %dx%d, %s is %dx%d"
                             % (paths[0], images[0].shape[1], images[0].shape[0], p, img.shape[1], img.shape[0]))
    return np.stack(images)


def encode_file_texture(images, fmt, options=None, plan=None, ctx=None, mips=False, mip_filter="box", order="level", kernel=None,
                        wrap="clamp", hdr=None):
    """(L, H, W, 4) uint8 (BC6H: float16) numpy layers -> [layer][level] packed blocks (numpy), one level or the full chain (not R11)"""
    import torch
    ctx = ctx or api.default_context()
    blocks = ctx.encode_texture(container.canonical(fmt), torch.from_numpy(images).cuda(ctx.device), options, plan,
                                levels=None if mips else 1, order=order, mip_filter=mip_filter, kernel=kernel, wrap=wrap, hdr=hdr)
    torch.cuda.synchronize(ctx.device)
    host, start = blocks.base.cpu().numpy(), blocks.base.data_ptr()
    per = host.shape[1]
    return [[host[(t.data_ptr() - start) // per: (t.data_ptr() - start) // per + t.shape[0]] for t in levels] for levels in blocks]


def resized_size(w, h, resize=None, maxsize=None, pow2=None):
    """the size -resize (w, h) / -maxsize N / -pow2 nearest|up|down gives a w x h image"""
    if resize is not None:
        w, h = resize
    elif maxsize is not None:
        if maxsize < 1:
            raise ValueError("-maxsize: sizes are 1 .. 65535")
        larger = max(w, h)
        if larger > maxsize:
            w, h = (max(1, (side * maxsize * 2 + larger) // (2 * larger)) for side in (w, h))
    elif pow2 is not None:
        def power(side):
            below = 1 << (side.bit_length() - 1)
            if below == side or pow2 == "down":
                return below
            return 2 * below if pow2 == "up" or side - below >= 2 * below - side else below
        w, h = power(w), power(h)
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError("resize to %dx%d: sizes are 1 .. 65535" % (w, h))
    return w, h


def resize_file(images, width, height, kernel="lanczos3", rule="box", wrap="clamp", signed=False, ctx=None, hdr=None):
    """(H, W, 4) or (L, H, W, 4) uint8 numpy image(s) -> the same resized to width x height on the device (all layers in one call);
    float16 images with hdr, their range (api.MIP_HDR)"""
    import torch
    ctx = ctx or api.default_context()
    out = ctx.resize(torch.from_numpy(np.ascontiguousarray(images)).cuda(ctx.device), width, height, kernel=kernel, filter=rule, wrap=wrap,
                     signed=signed, hdr=hdr)
    torch.cuda.synchronize(ctx.device)
    return out.cpu().numpy()


def print_metrics(report, out=None):
    out = out or sys.stdout
    for c, name in enumerate("RGBA"):
        if (report.channel_mask >> c) & 1:
            out.write("%s mse %.6f psnr %.4f dB\n" % (name, report.mse[c], report.psnr(name)))
    out.write("psnr %.4f dB (%s, %d texels)\n" % (report.psnr(), report.channels.upper(), report.texels))


def print_mip_metrics(reports, w, h, out=None):
    """one line per level 1 .. of a w x h image: the reports measure_file_mips returned"""
    out = out or sys.stdout
    for l, report in enumerate(reports, 1):
        out.write("mip %d %dx%d psnr %.4f dB (%s, %d texels)\n" % (l, max(1, w >> l), max(1, h >> l), report.psnr(),
                                                                  report.channels.upper(), report.texels))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    fmt, uniform, fake, quality, dds, metrics, mips, paths = "etc2rgb", False, False, None, False, False, False, []
    mip_filter, alpha_weight, srgb, array, cube = None, False, False, False, False
    mip_kernel, wrap = None, None
    resize, maxsize, pow2, size_flags, resize_kernel, resize_rule, resize_wrap = None, None, None, 0, None, None, None
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "-format" and i + 1 < len(argv):
            fmt = argv[i + 1]
            i += 1
        elif a == "-quality" and i + 1 < len(argv):
            quality = int(argv[i + 1])
            i += 1
        elif a == "-uniform":
            uniform = True
        elif a == "-dds":
            dds = True
        elif a == "-metrics":
            metrics = True
        elif a == "-mips":
            mips = True
        elif a == "-mipfilter" and i + 1 < len(argv) and argv[i + 1] in ("box", "srgb", "normal"):
            mip_filter = argv[i + 1]
            i += 1
        elif a == "-mipkernel" and i + 1 < len(argv) and argv[i + 1] in api.MIP_KERNELS:
            mip_kernel = argv[i + 1]
            i += 1
        elif a == "-wrap" and i + 1 < len(argv) and argv[i + 1] in api.MIP_WRAPS:
            wrap = argv[i + 1]
            i += 1
        elif a == "-resize" and i + 1 < len(argv) and re.match(r"^[0-9]+x[0-9]+$", argv[i + 1]):
            resize = tuple(int(v) for v in argv[i + 1].split("x"))
            size_flags += 1
            i += 1
        elif a == "-maxsize" and i + 1 < len(argv) and argv[i + 1].isdigit():
            maxsize = int(argv[i + 1])
            size_flags += 1
            i += 1
        elif a == "-pow2" and i + 1 < len(argv) and argv[i + 1] in ("nearest", "up", "down"):
            pow2 = argv[i + 1]
            size_flags += 1
            i += 1
        elif a == "-resizekernel" and i + 1 < len(argv) and argv[i + 1] in api.RESIZE_KERNELS:
            resize_kernel = argv[i + 1]
            i += 1
        elif a == "-resizerule" and i + 1 < len(argv) and argv[i + 1] in api.RESIZE_RULES:
            resize_rule = argv[i + 1]
            i += 1
        elif a == "-resizewrap" and i + 1 < len(argv) and argv[i + 1] in api.MIP_WRAPS:
            resize_wrap = argv[i + 1]
            i += 1
        elif a == "-alphaweight":
            alpha_weight = True
        elif a == "-srgb":
            srgb = True
        elif a == "-fakebt709":
            fake = True
        elif a == "-array":
            array = True
        elif a == "-cube":
            cube = True
        elif a.startswith("-"):
            sys.stderr.write(USAGE + "\n")
            return 2
        else:
            paths.append(a)
        i += 1
    if (array and cube) or len(paths) < 2 or (len(paths) != 2 and not (array or cube)):
        sys.stderr.write(USAGE + "\n")
        return 2
    mips = mips or mip_filter is not None or alpha_weight or mip_kernel is not None
    mip_filter = (mip_filter or "box") + ("+alpha" if alpha_weight else "")
    try:
        fmt = container.canonical(fmt)
        if mip_filter not in api.MIP_FILTERS:
            raise ValueError("-alphaweight goes with -mipfilter box or srgb")
        if mip_kernel is not None and alpha_weight:
            raise ValueError("-mipkernel does not go with -alphaweight")
        if fmt in HALF_FORMATS and (mip_filter != "box" or resize_rule not in (None, "box")):
            raise ValueError("%s is encoded from half-float images, which take the box rule only (no -mipfilter srgb|normal, -alphaweight, "
                             "-resizerule srgb|normal)" % fmt)
        if wrap is not None and mip_kernel is None:
            raise ValueError("-wrap goes with -mipkernel")
        if fmt in ("bc4s", "bc5s") and mip_filter not in ("box", "normal"):
            raise ValueError("-mipfilter %s: %s averages the image as int8, which takes box or normal" % (mip_filter, fmt))
        if srgb and fmt not in container.SRGB_FORMATS:
            raise ValueError("-srgb: %s has no sRGB format code" % fmt)
        if mips and fmt in ("r11u", "r11s"):
            raise ValueError("-mips: %s has no image form, so no mip chain" % fmt)
        if (array or cube) and fmt in ("r11u", "r11s"):
            raise ValueError("-%s: %s has no image form" % ("cube" if cube else "array", fmt))
        if dds and (array or cube) and container.FORMATS[fmt][3] is None:
            raise ValueError("%s has no DXGI format; use KTX" % fmt)
        if size_flags > 1:
            raise ValueError("-resize, -maxsize, -pow2: one of them")
        for flag, value in (("-resizekernel", resize_kernel), ("-resizerule", resize_rule), ("-resizewrap", resize_wrap)):
            if value is not None and not size_flags:
                raise ValueError("%s goes with -resize, -maxsize or -pow2" % flag)
        if resize_rule == "srgb" and fmt in ("bc4s", "bc5s"):
            raise ValueError("-resizerule srgb: %s reads the image as int8, which takes box or normal" % fmt)
        if cube and len(paths) > 2 and (len(paths) - 1) % 6 != 0:
            raise ValueError("-cube takes the 6 faces of a cube (+X -X +Y -Y +Z -Z) or 6 n of a cube array, got %d inputs" % (len(paths) - 1))
        if array or cube:
            layers = load_layers(paths[:-1], fmt)
            if cube and (layers.shape[0] % 6 != 0 or layers.shape[1] != layers.shape[2]):
                raise ValueError("-cube needs 6 n square faces, got %d of %dx%d" % (layers.shape[0], layers.shape[2], layers.shape[1]))
        else:
            image = load_rgba16f(paths[0], fmt) if fmt in HALF_FORMATS else load_rgba8(paths[0])
        if size_flags:
            loaded = layers if (array or cube) else image
            target = resized_size(loaded.shape[-2], loaded.shape[-3], resize, maxsize, pow2)
            if cube and target[0] != target[1]:
                raise ValueError("-cube: resizing to %dx%d leaves no square faces" % target)
    except (ValueError, OSError) as e:
        sys.stderr.write("%s\n" % e)
        return 1
    if size_flags and target != (loaded.shape[-2], loaded.shape[-3]):
        loaded = resize_file(loaded, target[0], target[1], resize_kernel or "lanczos3", resize_rule or "box", resize_wrap or "clamp",
                             signed=fmt in ("bc4s", "bc5s"), hdr=HALF_FORMATS.get(fmt))
        if array or cube:
            layers = loaded
        else:
            image = loaded
    how = dict(mip_filter=mip_filter, kernel=mip_kernel, wrap=wrap or "clamp", hdr=HALF_FORMATS.get(fmt) if mip_kernel is not None else None)
    options = api.Options()
    if uniform:  # etc2packer.cpp:202-205
        options.flags |= api.Flags.Uniform
    elif fake:
        options.flags |= api.Flags.ETC_UseFakeBT709
    plan = None
    if quality is not None:
        plan = api.BC7EncodingPlan()
        api.ConfigureBC7EncodingPlanFromQuality(plan, quality)
    if array or cube:
        h, w = layers.shape[1:3]
        texture = encode_file_texture(layers, fmt, options, plan, mips=mips, order="layer" if dds else "level", **how)
        (container.write_dds_texture if dds else container.write_ktx_texture)(paths[-1], fmt, w, h, texture, cube, srgb)
        for n, (image, levels) in enumerate(zip(layers, texture) if metrics else ()):
            sys.stdout.write("layer %d\n" % n)
            print_metrics(measure_file(image, fmt, levels[0], options))
            if mips:
                print_mip_metrics(measure_file_mips(image, fmt, levels, **how), w, h)
        return 0
    h, w = image.shape[:2]
    if mips:
        levels = encode_file_mips(image, fmt, options, plan, **how)
        packed = levels[0]
        (container.write_dds_mips if dds else container.write_ktx_mips)(paths[1], fmt, w, h, levels, srgb)
    else:
        packed = encode_file(image, fmt, options, plan)
        (container.write_dds if dds else container.write_ktx)(paths[1], fmt, w, h, packed, srgb)
    if metrics:
        print_metrics(measure_file(image, fmt, packed, options))
        if mips:
            print_mip_metrics(measure_file_mips(image, fmt, levels, **how), w, h)
    return 0


if __name__ == "__main__":
    sys.exit(main())

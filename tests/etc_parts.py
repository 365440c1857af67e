"""The ETC part sweeps from Python: the table of sweeps, the tables of inputs their domains read (oracle/etc_parts.h turns an
input number into arguments; the values it picks from are built here), the host side (the restatement's parts, the
reference's own functions where oracle/_ref was built) and the device side (tests/device/lanetest_etc.hip in the lane-test
library).  Nothing here is part of the product."""
import ctypes
import os

import numpy as np

from oracle import pyref

CHUNK = pyref.ETC_PARTS_CHUNK


def host_threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


# ---- weight sets of the weighted metric: the default, the goldens', the corners of tests/fuzz_options.py -------------------
DEFAULT_WEIGHTS = (float(np.float32(0.2125) / np.float32(0.7154)), 1.0, float(np.float32(0.0721) / np.float32(0.7154)))
WEIGHT_SETS = {
    "default": DEFAULT_WEIGHTS,
    "goldens": (0.1, 1.0, 0.8),
    "zero red": (0.0, 1.0, 1.0),
    "negative red": (-1.0, 1.0, 3.0),
    "100, 1e-3, 0.1": (100.0, 1e-3, 0.1),
    "all 1e-3": (1e-3, 1e-3, 1e-3),
}


# ---- the tables ------------------------------------------------------------------------------------------------------------
def th_table():
    """[16][128] targets of resolveTHFake per granularity g: every cell boundary k 34 g - 1, k 34 g, k 34 g + 1 (k = 0 ... 15),
    the cell midpoints (510 g = 15 * 34 g is the largest sum of a channel), the largest target the T-mode line modifiers reach
    (510 g + 128 g: numLine * 2 * thDistance[7], etc2_kernel.hip) with the value below it, and seeded values up to there:
    128 different values"""
    rng = np.random.Generator(np.random.PCG64(20261021))
    table = np.zeros((16, 128), np.int32)
    for g in range(1, 17):
        cell, top = 34 * g, 638 * g
        vals = set()
        for k in range(16):
            vals |= {max(k * cell - 1, 0), k * cell, k * cell + 1, k * cell + cell // 2}
        vals |= {top - 1, top}
        rest = rng.permutation(np.setdiff1d(np.arange(top + 1), sorted(vals)))[:128 - len(vals)]
        vals = sorted(vals) + [int(v) for v in rest]
        assert len(set(vals)) == 128 and max(vals) == top < 32768 and min(vals) == 0
        table[g - 1] = vals
    return table


def half_quantisers(cu):
    """what steps inside resolveHalfFake along one channel's cumulative: the accurate form's two wrapping quantisers, the table
    form's two bases and cu >> 8, where cu + (cu >> 8) steps twice"""
    cu = np.asarray(cu, np.int64)
    fill = cu + (cu >> 8)
    return [((((cu << 5) - ((cu << 1) & 0xffff)) + (cu >> 3)) & 0xffff) >> 12, ((((cu << 5) - cu) + (cu >> 3)) & 0xffff) >> 11,
            fill >> 7, fill >> 6, cu >> 8]


def half_table():
    """[256] candidates of the third channel: 0, 2040, every point where one of half_quantisers steps with its two neighbours
    (243 values), the rest seeded"""
    cu = np.arange(2041)
    pts = {0, 2040}
    for q in half_quantisers(cu):
        for s in np.flatnonzero(np.diff(q)) + 1:
            pts |= {int(s) - 1, int(s), min(int(s) + 1, 2040)}
    assert len(pts) <= 256 and min(pts) == 0 and max(pts) == 2040
    rng = np.random.Generator(np.random.PCG64(20261022))
    rest = [int(v) for v in rng.permutation(np.setdiff1d(cu, sorted(pts)))[:256 - len(pts)]]
    return np.array(sorted(pts) + rest, np.int32)


def to_fake709(rgb):
    """ConvertToFakeBT709 in binary32, operation by operation (only to make pre-weighted pixels that a colour can meet exactly)"""
    r, g, b = (np.asarray(rgb, np.float32)[..., i] for i in range(3))
    f = np.float32
    y = ((r * f(0.368233989135369)).astype(f) + (g * f(1.23876274963149)).astype(f)).astype(f) + (b * f(0.125054068802017)).astype(f)
    u = ((r * f(0.5)).astype(f) - (g * f(0.4541529)).astype(f)).astype(f) - (b * f(0.04584709)).astype(f)
    v = ((r * f(-0.081014709086133)).astype(f) - (g * f(0.272538676238785)).astype(f)).astype(f) + (b * f(0.353553390593274)).astype(f)
    return np.stack([y, u, v], axis=-1).astype(f)


def pixels():
    """64 pixels: black, white, the primaries, mid-grey and its neighbours, the rest seeded"""
    rng = np.random.Generator(np.random.PCG64(20261023))
    px = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0),
          (128, 128, 128), (127, 128, 129), (1, 254, 0), (17, 34, 51)]
    px += [tuple(int(c) for c in rng.integers(0, 256, 3)) for _ in range(64 - len(px))]
    return np.array(px, np.int32)


def pixel_table(weights=None):
    """int px[64][3], then the bits of float pw[64][3]: the pixels pre-weighted as ExtractBlocks does -- px * weight, or
    (weights None) their fake-BT.709 luma / chroma.  Every pixel is also a colour of the sweep, so a difference of exactly zero
    is in every sweep"""
    px = pixels()
    if weights is None:
        pw = to_fake709(px)
    else:
        pw = (px.astype(np.float32) * np.asarray(weights, np.float32)[None, :]).astype(np.float32)
    return np.concatenate([px.ravel(), pw.ravel().view(np.int32)]).astype(np.int32)


# ---- the sweeps: name -> (part, variant, weights, table maker, host (part, variant, weights) where it differs) ----------------
def _sweeps():
    t = {"resolveTHFake": ("resolve_th", 0, None, "th")}
    for v, name in enumerate(("table form, individual", "table form, differential", "accurate, individual", "accurate, differential")):
        t["resolveHalfFake (%s)" % name] = ("resolve_half", v, None, "half")
    t["EtcErr::operator() fake"] = ("err_fake", 0, None, "fake pixels")
    t["EtcErr::wu uniform"] = ("err_wu", 0, None, "pixels")
    for wname, w in WEIGHT_SETS.items():
        t["EtcErr::wu weighted (%s)" % wname] = ("err_wu", 1, w, "pixels")
        t["EtcErr::err2(weigh2(a, b)).x (%s)" % wname] = ("err2", 0, w, "pixels")
        t["EtcErr::err2(weigh2(a, b)).y (%s)" % wname] = ("err2", 1, w, "pixels")
    t["planarDecode"] = ("planar", 0, None, None)
    for part, fn in (("emit_t", "emitT"), ("emit_h", "emitH")):
        t["%s high word" % fn] = (part, 0, None, None)
        t["%s low word" % fn] = (part, 1, None, None)
    t["emitT high word, a channel at 16"] = ("emit_t", 2, None, None)
    t["emitT low word, a channel at 16"] = ("emit_t", 3, None, None)
    t["emitH high word, a field above 15"] = ("emit_h", 2, None, None)
    t["emitH low word, a field above 15"] = ("emit_h", 3, None, None)
    return t


SWEEPS = _sweeps()
# the device functions the table reaches, for tests/test_etc_primitives_cpu.py: every function of etc2_metric.h is one of them
# or is called by one
SWEPT_FUNCTIONS = ("toFake709", "fakeOctant", "resolveTHFake", "resolveHalfFake", "EtcErr", "planarDecode", "emitT", "emitH")
DEVICE_SYMBOLS = ("lanetest_etc_tables_size", "lanetest_etc_tables", "lanetest_etc_sums", "lanetest_etc_chunk", "lanetest_etc_round_trip",
                  "lanetest_etc_emit_sample")

_tables = {}


def table_of(kind, weights):
    key = (kind, weights)
    if key not in _tables:
        _tables[key] = {None: lambda: None, "th": th_table, "half": half_table, "fake pixels": lambda: pixel_table(None),
                        "pixels": lambda: pixel_table(weights or (1.0, 1.0, 1.0))}[kind]()
    return _tables[key]


def sweep_args(name):
    part, variant, weights, kind = SWEEPS[name]
    return part, variant, weights, table_of(kind, weights)


def host_key(name):
    """what the host computes for a sweep: err2's first colour is the weighted metric's own input"""
    part, variant, weights, kind = SWEEPS[name]
    if part == "err2" and variant == 0:
        part, variant = "err_wu", 1
    return part, variant, weights, kind


def describe(name, n):
    """the arguments behind input n of a sweep, as etc_parts.h derives them"""
    part, variant, weights, table = sweep_args(name)
    if part == "resolve_th":
        g = ((n >> 21) & 15) + 1
        t = [int(table[g - 1][(n >> (7 * ch)) & 127]) for ch in range(3)]
        return "granularity %d, targets %s, quantised %s" % (g, t, [min(15, v // (34 * g)) for v in t])
    if part == "resolve_half":
        c0, c1 = (n >> 17) & 2047, (n >> 6) & 2047
        return "cumulative %s" % [min(c0, 2040), min(c1, 2040), int(table[(n & 63) * 4 + ((c0 + c1) & 3)])]
    if part in ("err_fake", "err_wu", "err2"):
        c = (n >> 6) & 0xffffff
        return "colour (%d, %d, %d), pixel %s, weights %s" % (c >> 16, (c >> 8) & 255, c & 255, table[3 * (n & 63):3 * (n & 63) + 3].tolist(), weights)
    if part == "planar":
        return "coefficient %d, channel %d" % (n & 127, (n >> 7) & 3)
    if variant & 2:
        return "sample %d" % n
    return "opaque %d, table %d, colours 0x%03x 0x%03x" % ((n >> 27) & 1, (n >> 24) & 7, (n >> 12) & 0xfff, n & 0xfff)


# ---- host side ---------------------------------------------------------------------------------------------------------------
_host_cache = {}


def host_sums(lib, name):
    """(checksums of every chunk, results that carry the range flag) of sweep `name` from `lib` (pyref.OracleLib or
    pyref.RefEtcParts); kept per library, since sweeps share host references"""
    key = (id(lib),) + host_key(name)
    if key not in _host_cache:
        part, variant, weights, kind = host_key(name)
        sums, _, flagged = lib.etc_parts(part, variant, weights, table_of(kind, weights), threads=host_threads())
        _host_cache[key] = (sums, flagged)
    return _host_cache[key]


def host_chunk(lib, name, chunk):
    part, variant, weights, kind = host_key(name)
    return lib.etc_parts(part, variant, weights, table_of(kind, weights), first_chunk=chunk, num_chunks=1, full=True)[1]


def chunk_mismatches(name, want_sums, got_sums, want_chunk, got_chunk, sides=("the device", "the host")):
    """None, or the failure message of a sweep whose checksums differ: the count of mismatching inputs (exact while at most 64
    chunks differ) and the lowest one, with its arguments and both results"""
    bad = np.flatnonzero(np.asarray(want_sums) != np.asarray(got_sums))
    if len(bad) == 0:
        return None
    count, lowest = 0, None
    for c in bad[:64]:
        w, g = want_chunk(int(c)), got_chunk(int(c))
        j = np.flatnonzero(w != g)
        count += len(j)
        if lowest is None and len(j):
            n = int(c) * CHUNK + int(j[0])
            lowest = "input %d (%s): %s gives 0x%x, %s 0x%x" % (n, describe(name, n), sides[0], int(g[j[0]]), sides[1], int(w[j[0]]))
    more = "" if len(bad) <= 64 else " in the first 64 of %d differing chunks" % len(bad)
    return "%s: %d of %d inputs differ%s, the lowest %s" % (name, count, len(want_sums) * CHUNK, more, lowest)


# ---- device side -------------------------------------------------------------------------------------------------------------
_device = {}


def _lt():
    import lanetest
    return lanetest


def device_tables():
    """the CvttDeviceTables of the lane-test library on the device (thDistance, etc1Modifiers, fake709Rounding from the product's
    table headers)"""
    if "tables" not in _device:
        import torch
        lt = _lt()
        lib = lt.load()
        lib.lanetest_etc_tables_size.restype = ctypes.c_size_t
        buf = torch.zeros(int(lib.lanetest_etc_tables_size()), dtype=torch.uint8, device="cuda:0")
        lt._check(lib.lanetest_etc_tables(lt.ptr(buf), lt._stream()), "lanetest_etc_tables")
        _device["tables"] = buf
    return _device["tables"]


def _device_table(kind, weights):
    key = ("table", kind, weights)
    if key not in _device:
        t = table_of(kind, weights)
        _device[key] = _lt().to_device(t if t is not None else np.zeros(1, np.int32))
    return _device[key]


def _device_head(name):
    part, variant, weights, kind = SWEEPS[name]
    w = (ctypes.c_float * 3)(*(weights or (0.0, 0.0, 0.0)))
    lt = _lt()
    return part, variant, [ctypes.c_int(pyref.ETC_PARTS[part]), ctypes.c_int(variant), w, lt.ptr(_device_table(kind, weights)), lt.ptr(device_tables())]


def device_sums(name):
    import torch
    lt = _lt()
    part, variant, head = _device_head(name)
    n = pyref.etc_parts_chunks(part, variant)
    sums = torch.empty(n, dtype=torch.int64, device="cuda:0")
    lt._check(lt.load().lanetest_etc_sums(*head, ctypes.c_uint32(0), ctypes.c_uint32(n), lt.ptr(sums), lt._stream()), "lanetest_etc_sums")
    torch.cuda.synchronize()
    return sums.cpu().numpy().view(np.uint64)


def device_chunk(name, chunk):
    import torch
    lt = _lt()
    part, variant, head = _device_head(name)
    out = torch.empty(CHUNK, dtype=torch.int32, device="cuda:0")
    lt._check(lt.load().lanetest_etc_chunk(*head, ctypes.c_uint32(chunk), lt.ptr(out), lt._stream()), "lanetest_etc_chunk")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def device_mismatches(name, lib, host_name=None):
    """None, or the failure message of the device sweep `name` held against `lib`'s host sweep `host_name` (default: its own)"""
    host_name = host_name or name
    want, _ = host_sums(lib, host_name)
    return chunk_mismatches(name, want, device_sums(name), lambda c: host_chunk(lib, host_name, c), lambda c: device_chunk(name, c))

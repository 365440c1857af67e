#!/usr/bin/env python3
"""Developer tool (GPU box): how the resident waves of a SIMD line up in time during the BC7 encoder's main launch, from the
per-wave records of a profile build (csrc/bc7_kernel.hip, "One record per wave"):
   make -C convectionkernels_amd/csrc VARIANT=trace EXTRA=-DCVTT_BC7_PROFILE=2      (the records alone: no scratch, four waves per SIMD)
   CVTTMI_LIB=convectionkernels_amd/lib/variants/libcvtt_mi355x_trace.so python tools/bc7_phase_overlap.py [size] [opaque]
RGBA noise of size x size pixels (default 4096), default options and plan.  Shader-clock stamps are compared only among the waves
of one SIMD (XCC, SE, SH, CU, SIMD of the hardware-id registers); the tail table uses the 100 MHz wall clock of the records.
Prints
  * the start offsets between the waves that share a SIMD, by resident generation (generation g of a wave slot = the g-th wave
    that ran in it), in units of the median wave duration: waves in step have offsets near 0, evenly spread ones near 0.25;
  * the share of the SIMDs' busy time in which 0, 1, 2, 3, 4 resident waves are in the dual-plane search at once, and the same
    for the partition bounds (the longest bounds interval of each wave); beside it what independent waves would give
    (binomial, from the phase's share of a wave's life);
  * the number of resident waves over the last 150 us of the launch."""
import ctypes
import os
import sys
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from convectionkernels_amd import api, synth

WORDS = 10


def occupancy_shares(begin, end, busy_begin, busy_end):
    """share of the union of [busy_begin, busy_end) in which k = 0..4 of the intervals [begin, end) are open"""
    ok = end > begin
    t = np.concatenate([begin[ok], end[ok], busy_begin, busy_end])
    d_phase = np.concatenate([np.ones(ok.sum(), np.int64), -np.ones(ok.sum(), np.int64), np.zeros(2 * len(busy_begin), np.int64)])
    d_busy = np.concatenate([np.zeros(2 * ok.sum(), np.int64), np.ones(len(busy_begin), np.int64), -np.ones(len(busy_end), np.int64)])
    order = np.argsort(t, kind="stable")
    t, n_phase, n_busy = t[order], np.cumsum(d_phase[order]), np.cumsum(d_busy[order])
    dt = np.diff(t).astype(np.float64)
    live = n_busy[:-1] > 0
    shares = np.bincount(np.clip(n_phase[:-1][live], 0, 4), weights=dt[live], minlength=5)
    return shares, dt[live].sum()


def main():
    args = [a for a in sys.argv[1:]]
    save = load = None
    while args and args[0] in ("--save", "--load"):  # the raw records as .npy: keep them, or analyse kept ones without a GPU
        save, load = (args[1], load) if args[0] == "--save" else (save, args[1])
        args = args[2:]
    size = int(args[0]) if args else 4096
    opaque = len(args) > 1 and args[1] == "opaque"
    if load:
        rec = np.load(load)
        return analyse(rec, size, opaque)
    ctx = api.Context(0)
    lib = api.load_library()
    if not hasattr(lib, "cvttmi_bc7_wave_trace_set"):
        sys.exit("the loaded library is no profile build (CVTTMI_LIB=.../libcvtt_mi355x_trace.so)")
    lib.cvttmi_bc7_wave_trace_set.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    t = torch.from_numpy(synth.tile_blocks(synth.image_rgba8(2, size, size, opaque=opaque))).cuda()
    waves = (t.shape[0] + 15) // 16
    out = ctx.encode_bc7(t)  # warm: tables, work buffers, code objects
    torch.cuda.synchronize()
    buf = torch.zeros((waves, WORDS), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.cvttmi_bc7_wave_trace_set(buf.data_ptr(), waves) == 0
    ctx.encode_bc7(t, out=out)
    torch.cuda.synchronize()
    assert lib.cvttmi_bc7_wave_trace_set(None, 0) == 0
    rec = buf.cpu().numpy().view(np.uint64)
    del buf
    if save:
        np.save(save, rec)
    analyse(rec, size, opaque)


def analyse(rec, size, opaque):
    waves = len(rec)
    hw = rec[:, 0]
    slot, simd, cu, sh, se, xcc = (hw & 15).astype(int), ((hw >> 4) & 3).astype(int), ((hw >> 8) & 15).astype(int), ((hw >> 12) & 1).astype(int), \
        ((hw >> 13) & 7).astype(int), ((hw >> 32) & 15).astype(int)
    key = (((xcc * 8 + se) * 2 + sh) * 16 + cu) * 4 + simd
    start, at6, at0, at1, b2a, b2b, end = (rec[:, i].astype(np.int64) for i in range(1, 8))
    rt0, rt1 = rec[:, 8].astype(np.int64), rec[:, 9].astype(np.int64)
    written = end > 0
    dur = (end - start)[written]
    cyc_per_us = float(np.median(dur[rt1[written] > rt0[written]] / ((rt1 - rt0)[written][rt1[written] > rt0[written]] / 100.0)))
    simds = np.unique(key[written])
    print("BC7 %dx%d RGBA noise%s: %d waves, %d recorded, on %d SIMDs (%d XCCs); shader clock %.0f cycles/us" % (
        size, size, " (opaque)" if opaque else "", waves, int(written.sum()), len(simds), len(np.unique(xcc[written])), cyc_per_us))
    med = float(np.median(dur))
    print("wave duration: median %.1f us, 10th / 90th percentile %.1f / %.1f us;  of it dual-plane search %.1f %%, longest bounds interval %.1f %%" % (
        med / cyc_per_us, np.percentile(dur, 10) / cyc_per_us, np.percentile(dur, 90) / cyc_per_us,
        100.0 * np.median((at1 - at0)[written] / dur), 100.0 * np.median((b2b - b2a)[written] / dur)))
    launch_us = (rt1[written].max() - rt0[written].min()) / 100.0
    print("launch, first start to last end: %.1f us (wall clock of the records)" % launch_us)

    # ---- per SIMD: generations, start offsets, phase overlap
    gens, gen_dur = {}, {}
    dual = np.zeros(5)
    bounds = np.zeros(5)
    busy = 0.0
    slots_seen = []
    for k in simds:
        m = np.flatnonzero(written & (key == k))
        slots_seen.append(len(np.unique(slot[m])))
        gen = np.zeros(len(m), int)
        for s in np.unique(slot[m]):
            i = np.flatnonzero(slot[m] == s)
            gen[i[np.argsort(start[m][i], kind="stable")]] = np.arange(len(i))
        for g in np.unique(gen):
            gen_dur.setdefault(int(g), []).append((end[m] - start[m])[gen == g])
            st = np.sort(start[m][gen == g])
            if len(st) >= 2:
                gens.setdefault(int(g), []).append(np.diff(st) / med)
        s5, b = occupancy_shares(at0[m], at1[m], start[m], end[m])
        dual += s5
        busy += b
        bounds += occupancy_shares(b2a[m], b2b[m], start[m], end[m])[0]
    print("wave slots used per SIMD: %s" % dict(zip(*np.unique(slots_seen, return_counts=True))))
    print()
    print("start offsets between neighbouring waves of a SIMD (sorted by start), in median wave durations, by generation")
    print("%-12s %8s %8s %8s %8s %8s %14s" % ("generation", "SIMDs", "p10", "median", "p90", "< 0.05", "wave, median"))
    order = sorted(gens)
    groups = [(str(g), [g]) for g in order[:4]] + ([("%d..%d" % (order[4], order[-1]), order[4:])] if len(order) > 4 else [])
    if len(order) > 8:
        groups.insert(4, ("%d" % order[len(order) // 2], [order[len(order) // 2]]))
        groups.insert(5, ("%d" % order[-2], [order[-2]]))
    for name, gs in groups:
        v = np.concatenate([np.concatenate(gens[g]) for g in gs])
        n = sum(len(gens[g]) for g in gs)
        d = np.concatenate([np.concatenate(gen_dur[g]) for g in gs])
        print("%-12s %8d %8.3f %8.3f %8.3f %7.1f%% %11.1f us" % (name, n, np.percentile(v, 10), np.median(v), np.percentile(v, 90), 100.0 * (v < 0.05).mean(),
                                                          np.median(d) / cyc_per_us))
    print()

    def table(name, shares, frac):
        print("%s: share of SIMD busy time with k resident waves in the phase at once (independent waves: binomial of 4 at p = %.3f)" % (name, frac))
        print("   k        " + "".join("%9d" % k for k in range(5)))
        print("   measured " + "".join("%8.1f%%" % (100.0 * shares[k] / busy) for k in range(5)))
        print("   binomial " + "".join("%8.1f%%" % (100.0 * comb(4, k) * frac ** k * (1 - frac) ** (4 - k)) for k in range(5)))
        mean = sum(k * shares[k] for k in range(5)) / busy
        var = sum(k * k * shares[k] for k in range(5)) / busy - mean * mean
        print("   mean %.3f, variance %.3f (binomial %.3f; four waves in step %.3f)" % (mean, var, 4 * frac * (1 - frac), 16 * frac * (1 - frac)))

    table("dual-plane search", dual, float(np.mean((at1 - at0)[written] / dur)))
    table("partition bounds (longest interval)", bounds, float(np.mean((b2b - b2a)[written] / dur)))
    print()
    print("resident waves over the last 150 us of the launch (all SIMDs; full = %d)" % (4 * len(simds)))
    last = rt1[written].max()
    r0, r1 = rt0[written], rt1[written]
    for us in range(150, 0, -10):
        at = last - us * 100
        print("   -%3d us %7d" % (us, int(((r0 <= at) & (r1 > at)).sum())))


if __name__ == "__main__":
    main()

"""The dual-plane set-up sweep of the lane-test library (tests/device/lanetest_dual.hip) from Python: the call of the level-table
comparison and the numpy restatement of a level table."""
import ctypes

import numpy as np

import lanetest

# 2-bit and 3-bit index weights of BC7 (reference IndexSelector.h:90-100 through g_weights)
WEIGHTS = {2: (0, 21, 43, 64), 3: (0, 9, 18, 27, 37, 46, 55, 64)}

SYMBOLS = ("lanetest_dual_tables",)


def level_table_ref(e0, e1, bits):
    """((64 - w) e0 + w e1 + 32) >> 6 for every weight of a `bits`-bit index, packed four levels to a word, level 0 lowest:
    (tabLo, tabHi), tabHi = 0 for two bits"""
    e0, e1 = np.asarray(e0, np.int64), np.asarray(e1, np.int64)
    levels = [((64 - w) * e0 + w * e1 + 32) >> 6 for w in WEIGHTS[bits]]
    assert all(((l >= 0) & (l <= 255)).all() for l in levels)
    pack = lambda four: sum(l << (8 * k) for k, l in enumerate(four)).astype(np.uint32)
    return pack(levels[:4]), (pack(levels[4:]) if bits == 3 else np.zeros(e0.shape, np.uint32))


def device_tables():
    """((mismatches, lowest input) of dualLevelTables against the table it replaces, the 2-bit table, the 3-bit tabLo, tabHi of
    every pair e0 << 8 | e1)"""
    import torch
    lib = lanetest.load()
    res = lanetest.to_device(np.array([0, 0xffffffffffffffff], np.uint64).view(np.int64))
    outs = [torch.empty(65536, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    rc = lib.lanetest_dual_tables(*[lanetest.ptr(t) for t in outs], lanetest.ptr(res), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, "lanetest_dual_tables: hipError %d" % rc
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(np.uint64)
    return (int(r[0]), int(r[1])), [t.cpu().numpy().view(np.uint32) for t in outs]


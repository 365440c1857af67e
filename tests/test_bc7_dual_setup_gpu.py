"""What a refine round of the BC7 dual-plane search sets up ahead of its pixel loop (csrc/bc7_dual_setup.h), swept on the device
over its whole domain (tests/device/lanetest_dual.hip, tests/lanetest_dual.py): the level tables of the two planes -- a 2-bit
plane builds levels 1 and 2 and takes levels 0 and 3 from the end points, the 3-bit plane of mode 4 alone builds eight --
against the table they replace (kept verbatim in the test source) and against numpy, on all 256^2 end-point pairs, in the
three shapes the search has.  Every comparison is for equality.

(The short division of the index axes that was measured with them is not in the product -- level on top of the other two
items, docs/history.md -- so it has no sweep here.)"""
import numpy as np
import pytest

import lanetest
import lanetest_dual as D


def test_level_table_restatement_is_the_format():
    """the numpy restatement against the interpolation written out for a few pairs (no GPU): ends reproduced, weights summing to 64"""
    for bits, w in D.WEIGHTS.items():
        assert w[0] == 0 and w[-1] == 64 and all(a + b == 64 for a, b in zip(w, reversed(w)))
    lo, hi = D.level_table_ref(np.array([0, 255, 10]), np.array([255, 0, 10]), 2)
    assert [int(x) for x in lo] == [0x00 | 84 << 8 | 171 << 16 | 255 << 24, 255 | 171 << 8 | 84 << 16 | 0 << 24, 0x0a0a0a0a] and not hi.any()
    lo, hi = D.level_table_ref(np.array([0]), np.array([255]), 3)
    assert int(lo[0]) == 0 | 36 << 8 | 72 << 16 | 108 << 24 and int(hi[0]) == 147 | 183 << 8 | 219 << 16 | 255 << 24


def test_library_exports_the_dual_sweeps():
    lib = lanetest.load()
    for s in D.SYMBOLS:
        assert hasattr(lib, s), s


@pytest.fixture(scope="module")
def lt(gpu_ctx):
    return lanetest.load()


@pytest.fixture(scope="module")
def tables(lt):
    return D.device_tables()


@pytest.mark.gpu
def test_level_tables_equal_the_table_they_replace(tables):
    (count, lowest), _ = tables
    assert count == 0, "dualLevelTables: %d of 3 x 4 x 65 536 tables differ from levelTable, the lowest shape %d channel %d e0 %d e1 %d" % (
        count, lowest >> 20, (lowest >> 16) & 15, (lowest >> 8) & 255, lowest & 255)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", (2, 3))
def test_level_tables_equal_numpy(tables, bits):
    _, (two, three_lo, three_hi) = tables
    t = np.arange(65536)
    want_lo, want_hi = D.level_table_ref(t >> 8, t & 255, bits)
    describe = lambda i: "e0 %d e1 %d" % (i >> 8, i & 255)
    got_lo, got_hi = (two, np.zeros(65536, np.uint32)) if bits == 2 else (three_lo, three_hi)
    for name, got, want in (("tabLo", got_lo, want_lo), ("tabHi", got_hi, want_hi)):
        msg = lanetest.first_difference("%d-bit %s" % (bits, name), got, want, describe)
        assert msg is None, msg

"""The operand maps of v_mfma_i32_32x32x16_i8 that the BC7 first-tier sums rely on (csrc/mfma_i8.h): the self-test entry
multiplies a caller-given (32, 16) by (16, 32) int8 pair on the matrix cores and must return NumPy's integer product.  One-hot
operands place a single product: a wrong lane, byte or register map moves or drops it."""
import numpy as np
import pytest


def _check(ctx, a, b, what):
    got = ctx.selftest_mfma_i8(a, b)
    exp = a.astype(np.int32) @ b.astype(np.int32)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d entries differ, first at (row, column) %s: %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.gpu
def test_random_operands(gpu_ctx):
    rng = np.random.default_rng(16)
    for i in range(8):
        _check(gpu_ctx, rng.integers(-128, 128, (32, 16), dtype=np.int8), rng.integers(-128, 128, (16, 32), dtype=np.int8), "random %d" % i)


@pytest.mark.gpu
def test_extreme_operands(gpu_ctx):
    for x in (127, -127, -128):
        for y in (127, -127, -128):
            _check(gpu_ctx, np.full((32, 16), x, np.int8), np.full((16, 32), y, np.int8), "all %d by all %d" % (x, y))


@pytest.mark.gpu
def test_one_hot_rows_and_columns(gpu_ctx):
    """a: one non-zero entry per row, walking through K; b: every entry distinct -- then a: distinct, b: one-hot columns"""
    dense_b = (np.arange(16 * 32).reshape(16, 32) % 251 - 125).astype(np.int8)
    dense_a = (np.arange(32 * 16).reshape(32, 16) * 7 % 253 - 126).astype(np.int8)
    for shift in range(16):
        a = np.zeros((32, 16), np.int8)
        a[np.arange(32), (np.arange(32) + shift) % 16] = (np.arange(32) % 5 - 2) * 25 + 3
        _check(gpu_ctx, a, dense_b, "one-hot rows, shift %d" % shift)
        b = np.zeros((16, 32), np.int8)
        b[(np.arange(32) * 3 + shift) % 16, np.arange(32)] = (np.arange(32) % 7 - 3) * 17 - 1
        _check(gpu_ctx, dense_a, b, "one-hot columns, shift %d" % shift)
    # a single 1 by a single 1: exactly one entry of the tile is set, at (row, column), for every K
    for k in range(16):
        a = np.zeros((32, 16), np.int8)
        b = np.zeros((16, 32), np.int8)
        a[(5 * k + 3) % 32, k] = 1
        b[k, (11 * k + 7) % 32] = 1
        _check(gpu_ctx, a, b, "single product at K = %d" % k)

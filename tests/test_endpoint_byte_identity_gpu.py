"""The two-instruction endpoint byte of the BC7 kernels (csrc/cvtt_kernel_common.h: endpointByte = v_cvt_pk_u8_f32 of
fminf(x, 255)) against (int)clampRound(x, 255) on every one of the 2^32 binary32 bit patterns -- NaNs, infinities, zeros of
both signs and denormals included -- swept on the device (csrc/selftest_kernel.hip, cvttmi_selftest_endpoint_byte)."""
import pytest


@pytest.mark.gpu
def test_endpoint_byte_is_clamp_round_on_every_bit_pattern(gpu_ctx):
    mismatches, first = gpu_ctx.selftest_endpoint_byte()
    assert mismatches == 0, "%d of 2^32 patterns differ, the lowest 0x%08x" % (mismatches, first)

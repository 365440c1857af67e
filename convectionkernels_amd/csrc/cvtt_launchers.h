// The kernel launchers: host functions with C linkage, each defined in the *_kernel.hip beside its kernels and called from the
// host side of the C ABI (shim*.cpp).  Declared here ONCE: the host files call through these prototypes, and every .hip that
// defines one includes this header, so the compiler holds each definition against the declaration its callers use (C linkage
// carries no mangled argument list that the linker could check).  The argument structs are cvtt_device.h's.
#ifndef CVTTMI_LAUNCHERS_H
#define CVTTMI_LAUNCHERS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include "cvtt_device.h"

extern "C"
{
// bc7_kernel.hip, bc1_kernel.hip, bc6h_kernel.hip, etc2_kernel.hip, s3tc_alpha_kernel.hip: the encoders
hipError_t cvttmi_launch_bc7(const void *d_blocks, void *d_out, const CvttBc7Args *args, const CvttDeviceTables *d_tables,
                             const CvttBc7DevicePlan *d_plan, hipStream_t stream);
hipError_t cvttmi_launch_bc1(const void *d_blocks, void *d_out, const CvttBc1Args *args, const CvttDeviceTables *d_tables, hipStream_t stream);
hipError_t cvttmi_launch_bc6h(const void *d_blocks, void *d_out, const CvttBc6hArgs *args, const CvttDeviceTables *d_tables, int isSigned,
                              hipStream_t stream);
hipError_t cvttmi_launch_etc2(const void *d_blocks, void *d_out, const CvttEtcArgs *args, const CvttDeviceTables *d_tables, int mode,
                              hipStream_t stream);
hipError_t cvttmi_launch_eac11(const void *d_blocksS16, void *d_out, uint32_t numBlocks, int isSigned, const CvttDeviceTables *d_tables,
                               hipStream_t stream);
hipError_t cvttmi_launch_s3tc_alpha(const void *d_blocks, void *d_out, uint32_t numBlocks, uint32_t channel, uint32_t outStride,
                                    uint32_t outOffset, int isSigned, int explicitAlpha, int seedPoints, int refineRounds,
                                    const CvttDeviceTables *d_tables, hipStream_t stream);

// tile_kernel.hip, texture_kernel.hip: images <-> blocks
hipError_t cvttmi_launch_tile(const void *d_image, void *d_blocks, uint32_t width, uint32_t height, size_t rowPitch, uint32_t bytesPerPixel,
                              hipStream_t stream);
hipError_t cvttmi_launch_compact_rows(const void *d_packed, void *d_out, uint32_t width, uint32_t height, uint32_t bytesPerBlock,
                                      hipStream_t stream);
hipError_t cvttmi_launch_tile_chain(const CvttTextureLevels *levels, void *d_tiles, uint32_t bytesPerPixel, hipStream_t stream);
hipError_t cvttmi_launch_compact_chain(const CvttTextureLevels *levels, const void *d_packed, void *d_out, uint32_t bytesPerBlock,
                                       hipStream_t stream);

// mip_filter_kernel.hip (both downsample entries), mip_resample_kernel.hip, resize_kernel.hip
hipError_t cvttmi_launch_downsample(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch, size_t dstLayer,
                                    uint32_t srcW, uint32_t srcH, uint32_t layers, int kind, hipStream_t stream);
hipError_t cvttmi_launch_downsample_filtered(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch,
                                             size_t dstLayer, uint32_t srcW, uint32_t srcH, uint32_t layers, int kind, uint32_t filter,
                                             hipStream_t stream);
hipError_t cvttmi_launch_resample(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch, size_t dstLayer,
                                  uint32_t srcW, uint32_t srcH, uint32_t layers, int kind, uint32_t rule, uint32_t wrap, uint32_t range,
                                  const int16_t *taps, uint32_t count, hipStream_t stream);
size_t cvttmi_resize_entry_bytes(int kind, uint32_t rule);
uint32_t cvttmi_resize_fused_rows(int kind, uint32_t rule, const int32_t *first, uint32_t dstH, uint32_t ny);
hipError_t cvttmi_launch_resize(const void *d_src, size_t srcPitch, size_t srcLayer, uint32_t srcW, uint32_t srcH, void *d_dst,
                                size_t dstPitch, size_t dstLayer, uint32_t dstW, uint32_t dstH, uint32_t layers, int kind, uint32_t rule,
                                uint32_t wrap, uint32_t range, const int16_t *d_wx, const int32_t *d_fx, uint32_t nx, const int16_t *d_wy,
                                const int32_t *d_fy, uint32_t ny, void *d_mid, uint32_t fusedRows, hipStream_t stream);

// decode_kernel.hip
hipError_t cvttmi_launch_decode(const void *d_bc, void *d_out, uint32_t numBlocks, int format, const CvttDeviceTables *d_tables,
                                hipStream_t stream);
hipError_t cvttmi_launch_measure(const void *d_bc, const void *d_source, int source, uint32_t width, uint32_t height, size_t pitch,
                                 size_t firstBlock, uint32_t numBlocks, int format, void *d_blockError, void *d_slab,
                                 cvttmi_error_totals *d_totals, int accumulate, uint64_t texels, const CvttDeviceTables *d_tables,
                                 hipStream_t stream);
hipError_t cvttmi_launch_decode_image(const void *d_bc, void *d_image, size_t pitch, uint32_t width, uint32_t height, int format,
                                      const CvttDeviceTables *d_tables, hipStream_t stream);
hipError_t cvttmi_launch_decode_mips(const void *d_bc, const CvttDecodeLevels *levels, int format, const CvttDeviceTables *d_tables,
                                     hipStream_t stream);

// selftest_kernel.hip
hipError_t cvttmi_launch_selftest(uint64_t seed, uint64_t first, uint32_t count, void *d_operands, void *d_results, hipStream_t stream);
hipError_t cvttmi_launch_selftest_mfma_i8(const void *d_a, const void *d_b, void *d_out, hipStream_t stream);
hipError_t cvttmi_launch_selftest_endpoint_byte(void *d_result, hipStream_t stream);
}

#endif

// What the device sweeps and their host references share: a 2^32 domain is cut into 2^20 chunks of 4096 consecutive inputs
// (input = chunk << 12 | j), and a chunk's results r_j are folded into one 64-bit checksum.  Every term multiplies a word that
// differs whenever r_j differs by an odd number, so a single wrong result in a chunk always changes the chunk's checksum; the
// terms are independent of each other, so neither side serialises on the sum.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LANETEST_HD __host__ __device__
#else
#define LANETEST_HD
#endif

namespace lanetest
{
const uint32_t kChunk = 4096;      // inputs per chunk
const uint32_t kChunks = 1u << 20; // chunks per 2^32 domain

LANETEST_HD inline uint64_t term(uint32_t r, uint32_t j)
{
    return (uint64_t)(r ^ (j * 0x9E3779B1u)) * (0x9E3779B97F4A7C15ull + 2ull * j);
}
} // namespace lanetest

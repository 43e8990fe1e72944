// subset_common.hpp — what the host and the device share of the surface subset (subset_kernels.hip):
// the key of a row and the launch geometry.  Plain C++ (host and device).
#pragma once

#include <cstdint>

#include "../../include/cvhip.h"

#if defined(__HIPCC__)
#define CVHIP_SUBSET_HD __host__ __device__ __forceinline__
#else
#define CVHIP_SUBSET_HD inline
#endif

namespace cvhip {
namespace subset {

constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr uint32_t BLOCK = 256;                                   // lanes of a workgroup
constexpr uint32_t LANE_ROWS = CVHIP_SUBSET_WG_ROWS / BLOCK;      // rows of a lane per trip: row = chunk * WG_ROWS + j * BLOCK + lane
constexpr uint32_t GRID_BLOCKS = CVHIP_SUBSET_GRID_ROWS / CVHIP_SUBSET_WG_ROWS; // workgroups of a launch, at most
constexpr uint32_t DIGIT_BITS = 8, DIGITS = 1u << DIGIT_BITS, PASSES = 64 / DIGIT_BITS;
static_assert(CVHIP_SUBSET_WG_ROWS % BLOCK == 0 && CVHIP_SUBSET_GRID_ROWS % CVHIP_SUBSET_WG_ROWS == 0, "subset launch geometry");
static_assert(DIGITS == BLOCK, "one lane per histogram bin");

// splitmix64's finaliser: a bijection of the 64-bit words
CVHIP_SUBSET_HD uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// key(seed, i) = mix64(mix64(seed) + (i + 1) * GOLDEN): output i of splitmix64 started at mix64(seed).  `start` = mix64(seed).
CVHIP_SUBSET_HD uint64_t hashed_key(uint64_t start, uint64_t row) { return mix64(start + (row + 1) * GOLDEN); }

} // namespace subset
} // namespace cvhip

// npd_conv_common.hpp -- device pieces the conv-model kernel files share (npd_conv.hip, npd_conv_slab.hip,
// npd_conv_ws.hip, npd_conv_fc.hip): vector types, the activation-range words, GELU, MFMA wrappers.
#pragma once

#include <math.h>

#include "npd_common.hpp"

namespace npd {
namespace conv {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef _Float16 hf8 __attribute__((ext_vector_type(8)));
typedef _Float16 hf4 __attribute__((ext_vector_type(4)));

constexpr int kLayers = 10;
constexpr int kChunk = 8192;  // codewords per pass through the layer pipeline (FC0: 256-row tiles fill 256 CUs)

// fp16x3: activations are split as fp16(a 2^SA) + fp16(a 2^SA - hi) when staged: SA = 4 (lo normal for |a| >= 2^-7,
// below that lo's absolute resolution is 2^-28) while max |a| < 2^11, lower where a layer's inputs reach further
// (split_sa: max |a| 2^SA < 2^15, so hi cannot overflow fp16); the weights of each layer are scaled by 2^SW on the host
// so that max |w| 2^SW is in [2^12, 2^13) (hi and lo normal for |w| >= max |w| 2^-11)
constexpr int kSplitSA = 4;

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// The max |a| of one activation is kept in kAmaxSpread words kAmaxStride words apart (4 KB): each producing wave
// atomicMax-es one of them (by block and wave), so tens of thousands of small blocks (layer 0) do not serialise on one
// address; a consumer reads all of them with one load per lane and reduces over the wave.
constexpr int kAmaxSpread = 64;
constexpr int kAmaxStride = 16;
constexpr int kAmaxWords = kAmaxSpread * kAmaxStride;  // per activation
// max |activation| records of one chunk (fp16x3; kAmaxWords words each): conv layer i's output at record i, FC f's at
// record kLayers + f
constexpr int kAmaxSlots = kLayers + 3;

// max over a full wave, returned wave-uniform: DPP within rows of 16 lanes, then the 4 row results by readlane
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}

__device__ __forceinline__ int split_sa(const uint32_t* amax) {
    if (amax == nullptr) return kSplitSA;
    const uint32_t m = wave_max_u32(__builtin_nontemporal_load(amax + (threadIdx.x & 63) * kAmaxStride));
    const int e = (int)((m >> 23) & 0xFFu) - 126;  // max |a| < 2^e
    return min(kSplitSA, 15 - e);
}

// the activation split of every fp16x3 stager: x = v 2^SA (sc = 2^SA) -> hi = fp16(x), lo = fp16(x - hi)
__device__ __forceinline__ void split4(const f4& v, float sc, hf4& hi, hf4& lo) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x = v[j] * sc;
        hi[j] = (_Float16)x;
        lo[j] = (_Float16)(x - (float)hi[j]);
    }
}

__device__ __forceinline__ float amax4(const f4& v) {
    return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
}

// max over the wave of m (m >= 0, not NaN), then one atomicMax of its bits (non-negative floats order as unsigned
// integers)
__device__ __forceinline__ void publish_amax(uint32_t* amax, float m) {
    const uint32_t w = wave_max_u32(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0) {
        const uint32_t blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        atomicMax(amax + ((blk * 8 + (threadIdx.x >> 6)) % kAmaxSpread) * kAmaxStride, w);
    }
}

__device__ __forceinline__ f16v mfma(float a, float b, const f16v& c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f16v mfma16(const hf8& a, const hf8& b, const f16v& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

}  // namespace conv
}  // namespace npd

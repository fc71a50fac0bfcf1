// npd_sc_prim.hpp -- the one definition of each primitive the successive-cancellation families share: the SC units
// (npd_sc.hpp), npd_sc_fast.hip, the SC-List kernels (npd_scl.hpp), npd_lse.hip and npd_gen.hip.  These kernels are
// pinned bit for bit to the reference's fp32 sequence, so a change to rmul's barrier or to f_minsum is made here, once.
#pragma once
#include <stdlib.h>

#include "npd_common.hpp"

namespace npd {

// A/B and test switches are environment flags read per call (a getenv per launch), so a test can run both sides in
// one process: on for "1", off when unset, empty or "0".
inline bool env_flag(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
}

template <int N>
constexpr int log2c() {
    int n = 0;
    while ((1 << n) < N) ++n;
    return n;
}

// XOR swizzle of row r's 16-B chunks in a staged tile of C chunks per row (row-per-lane ds_read_b128 conflict-free)
template <int C>
__device__ __forceinline__ int swz(int r) {
    if constexpr (C >= 16) return r & 15;
    else return (r / (16 / C)) % C;
}

// The reference rounds L = fl32(scale*y) before any add (polar.py:468).  hipcc contracts fmul+fadd
// into fma by default, even for __fmul_rn; an empty asm makes the rounded product opaque.
__device__ __forceinline__ float rmul(float a, float b) {
    float r = a * b;
    asm("" : "+v"(r));
    return r;
}

// fl32(s * v) for 4 values in two packed multiplies (each product rounded, never contracted: see rmul)
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 rmul4(float s, float4 v) {
    f2v lo = {v.x, v.y}, hi = {v.z, v.w};
    const f2v ss = {s, s};
    lo = lo * ss;
    hi = hi * ss;
    asm("" : "+v"(lo), "+v"(hi));
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// sign(a) sign(b) min(|a|, |b|) in two VALU ops: med3(|a|, -|a|, b) = clamp(b, -|a|, |a|) has the
// magnitude min(|a|, |b|) and the sign of b; xor in the sign of a (v_med3_f32 + v_bitop3_b32).
// Equal in value to the reference's product form (utils.py:272-275; zeros may differ only in their sign bit, which
// no later step reads: sign(+-0) = 0, |+-0| = 0, u * (+-0) + b = b).
__device__ __forceinline__ float f_minsum(float a, float b) {
    const float m = __builtin_amdgcn_fmed3f(__builtin_fabsf(a), -__builtin_fabsf(a), b);
    return bitsf(__builtin_amdgcn_bitop3_b32(fbits(m), fbits(a), 0x80000000u, 0x78));  // m ^ (a & 0x80000000)
}

// The SC-List kernels' form of the same value: v_min_f32 on the magnitudes, then the xor of both sign bits or-ed in
// (three VALU ops).  Kept apart from f_minsum because it is another instruction sequence, and the list kernels'
// listings are pinned to it.
__device__ __forceinline__ float f_minsum_fmin(float a, float b) {
    const float m = __builtin_fminf(__builtin_fabsf(a), __builtin_fabsf(b));
    return bitsf(fbits(m) | ((fbits(a) ^ fbits(b)) & 0x80000000u));
}

// sign(x) in {-1, 0, +1} (torch.sign): copy the sign bit onto 1.0, 0 for +-0
__device__ __forceinline__ float sgn_bits(float x) {
    const float s = bitsf((fbits(x) & 0x80000000u) | 0x3f800000u);
    return (x == 0.0f) ? 0.0f : s;
}

// g with the left partial sum given as sign/zero bits of one position
__device__ __forceinline__ float g_bits(uint32_t sw, uint32_t zw, int bit, float a, float b) {
    const float s = bitsf(fbits(a) ^ ((sw << (31 - bit)) & 0x80000000u)) + b;
    return ((zw >> bit) & 1u) ? b : s;
}

// number of nonzero bytes in x
__device__ __forceinline__ uint32_t nz_bytes(uint32_t x) {
    const uint32_t t = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;
    return (uint32_t)__builtin_popcount(t & 0x80808080u);
}

// LDS at a byte offset: floats, and decisions in {-1, 0, 1} as int8
__device__ __forceinline__ void lds_wr(char* lds, uint32_t byte, float v) { *reinterpret_cast<float*>(lds + byte) = v; }
__device__ __forceinline__ float lds_rd(const char* lds, uint32_t byte) { return *reinterpret_cast<const float*>(lds + byte); }
__device__ __forceinline__ void lds_wr8(char* lds, uint32_t byte, float v) {
    *reinterpret_cast<int8_t*>(lds + byte) = (int8_t)(int)v;  // v in {-1, 0, 1}
}
__device__ __forceinline__ float lds_rd8(const char* lds, uint32_t byte) {
    return (float)*reinterpret_cast<const int8_t*>(lds + byte);
}

// Plotkin transform (encode_plotkin, polar.py:128-148) of N code bits held as bit words (bit i set iff u_i = -1):
// the butterfly is an XOR of shifted words below 32 positions and of whole words above
template <int N>
__device__ __forceinline__ void plotkin_bits(uint32_t (&U)[(N + 31) / 32]) {
    constexpr int NW = (N + 31) / 32;
#pragma unroll
    for (int h = 1; h < 32 && h < N; h <<= 1) {
        uint32_t msk = 0;
        for (int i = 0; i < 32; ++i)
            if (((i / h) & 1) == 0) msk |= 1u << i;
#pragma unroll
        for (int w = 0; w < NW; ++w) U[w] ^= (U[w] >> h) & msk;
    }
#pragma unroll
    for (int hw = 1; hw < NW; hw <<= 1)
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if (((w / hw) & 1) == 0) U[w] ^= U[w + hw];
}

// Elements 4q .. 4q+3 of the received word of codeword cw, value for value what npd_mc_generate writes
// (npd_gen.hip): Philox noise block (cw, q) -> 4 Box-Muller normals -> y = x + fl32(sigma z), x from the code bits U.
// Each value goes to emit(e, y) as it is made, so a caller's scaling stays next to it in the instruction stream.
template <class Emit>
__device__ __forceinline__ void noisy_chunk(const uint32_t* U, uint64_t seed, uint32_t stream, uint64_t cw, int q,
                                            float sigma, Emit&& emit) {
    const u32x4 o = philox_block(seed, stream, cw, (uint32_t)q);
    float z[4];
    normals4(o, z);
    const uint32_t bits = (U[(4 * q) >> 5] >> ((4 * q) & 31)) & 0xFu;
#pragma unroll
    for (int e = 0; e < 4; ++e) emit(e, __fadd_rn(((bits >> e) & 1u) ? -1.0f : 1.0f, __fmul_rn(sigma, z[e])));
}

}  // namespace npd

// npd_gru_common.hpp -- what the RNN decoder kernels share (npd_gru.hip, npd_gru_lstm.hip, npd_gru_split.hip,
// npd_gru_split16.hip, npd_gru_wide.hip, npd_gru_list.hip, npd_gru_wide_list.hip): the handle, the MFMA tile geometry (Geo, LGeo, hid_of), the
// LDS weight image layout, gemm_chain and the gate math.  Host-only declarations are in npd_gru_host.hpp.
#pragma once

#include "npd_common.hpp"

struct npd_gru {
    int N, F, layers, onehot, precision, device;
    float b_lin;
    float* img;   // LDS image (device)
    float* wy;    // y-projection A operands (device)
    int64_t img_floats;
    int64_t wy_lo;
    float* img16;  // 16-codeword split kernel's image (F = 64, 2 layers, split precisions), or NULL
    float* wy16;
    int64_t wy16_lo;
    int split16;   // its SplitT variant
    int cell;      // 0 GRU, 1 LSTM (fp32)
    int ln;        // use_layernorm head (rnn_all.py:317-320, :387-398): linear weights hold w * gamma, b_lin b + w . beta
    float ln_eps;
    float* hd;     // out_linear_depth > 1 head image (device; head_image below), or NULL
    int hd_depth, hd_tiles;
    float hd_bout;
};

namespace npd {
namespace gru {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

template <int N>
struct IC {
    static constexpr int value = N;
};
// compile-time loop: f(IC<i>{}) for i in [B, E)
template <int B, int E, typename Fn>
__device__ __forceinline__ void static_for(Fn&& f) {
    if constexpr (B < E) {
        f(IC<B>{});
        static_for<B + 1, E>(f);
    }
}

template <int F, int L>
struct Geo {
    static constexpr int TT = 3 * F / 32;  // 32-row tiles of the 3F gate rows
    static constexpr int HT = F / 32;      // 32-row tiles of the hidden state
    static constexpr int KS = F / 2;       // k-steps (2 hidden units each) per matvec
    static constexpr int KG = KS / 4;      // groups of 4 k-steps (one ds_read_b128)
    static constexpr int NG = (L == 2) ? 3 : 1;     // weight images: L0 hh, L1 ih, L1 hh
    static constexpr int G_SIZE = TT * KG * 64 * 4;  // floats per image
    static constexpr int OFF_X = NG * G_SIZE;        // extra k-step A operands [g][t][64]
    static constexpr int OFF_IN = OFF_X + NG * TT * 64;  // layer-0 n-gate input extra [HT][64]
    static constexpr int OFF_WL = OFF_IN + HT * 64;      // linear weights [half][HT][16]
    // bias vectors in accumulator-register order (tile, lane half, register i = row (i&3) + 8(i>>2) + 4 half) for the
    // folded kernel's accumulator initialisation: [b_hh0 n: HT tiles][layer-1 c0: TT tiles][b_hh1 n: HT tiles]
    static constexpr int OFF_CV = OFF_WL + 2 * HT * 16;
    static constexpr int TOTAL = OFF_CV + (2 * HT + TT) * 32;
};

// LSTM cells (lstm_decode_kernel, lstm_wide_kernel): Geo with 4F gate rows i, f, g, o
template <int F, int L>
struct LGeo {
    static constexpr int TT = 4 * F / 32;
    static constexpr int HT = F / 32;
    static constexpr int KS = F / 2;
    static constexpr int KG = KS / 4;
    static constexpr int NG = (L == 2) ? 3 : 1;
    static constexpr int G_SIZE = TT * KG * 64 * 4;
    static constexpr int OFF_X = NG * G_SIZE;           // layer-0 [1, x_i] k-step A operands [TT][64]
    static constexpr int OFF_WL = OFF_X + TT * 64;       // linear weights [half][HT][16]
    static constexpr int OFF_CV = OFF_WL + 2 * HT * 16;  // bias tiles in accumulator order: [layer][TT][half][16]
    static constexpr int TOTAL = OFF_CV + L * TT * 32;
};

__device__ __forceinline__ float sig2(float a) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(a)); }

// hidden unit fed by lane half `kk` at k-step s (accumulator row map of the 32x32 MFMA tile)
__host__ __device__ inline int hid_of(int s, int kk) {
    const int i = s & 15;
    return 32 * (s >> 4) + (i & 3) + 8 * (i >> 2) + 4 * kk;
}

struct Args {
    const float* img;
    const f4* wy;
    const float* y;   // NULL: no y input (decoding_type 'y_h0': the RNN input is the previous bit alone)
    const float* h0;  // NULL: zero initial state; else (B, F L), element f L + l = layer l, unit f (get_h0's x)
    const float* gt;
    float* decoded;
    float* logits;
    int64_t B;
    int N;
    int rev;
    int onehot;
    float b_lin;
    uint32_t info[kMaxWords];
    int ln;                // LayerNorm head (gru_decode_kernel only)
    float ln_eps;
    const f4* hd;          // out_linear_depth > 1 head (gru_decode_kernel<.., HDT > 0>): image, depth, last bias
    int hd_depth;
    float hd_bout;
};

__device__ __forceinline__ f16v mfma(float a, float b, const f16v& c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// acc[0..NT) += W_g[tiles t0..t0+NT) . h  over all KS k-steps.  Weight groups (4 k-steps, one
// ds_read_b128 per tile) are read one group ahead of the MFMAs that consume them; the empty asm with a
// memory clobber bounds that look-ahead so the weights of a whole matvec are never hoisted into VGPRs.
template <int TT, int KG, int NT, int HT>
__device__ __forceinline__ void gemm_chain(const f4* __restrict__ smem4, int g, int t0, int lane, f16v (&acc)[NT],
                                           const f16v (&h)[HT]) {
    f4 wc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wc[t] = smem4[((g * TT + t0 + t) * KG + 0) * 64 + lane];
#pragma unroll
    for (int s4 = 0; s4 < KG; ++s4) {
        f4 wn[NT];
        if (s4 + 1 < KG) {
#pragma unroll
            for (int t = 0; t < NT; ++t) wn[t] = smem4[((g * TT + t0 + t) * KG + s4 + 1) * 64 + lane];
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = 4 * s4 + e;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma(wc[t][e], h[s >> 4][s & 15], acc[t]);
        }
        if (s4 + 1 < KG) {
#pragma unroll
            for (int t = 0; t < NT; ++t) wc[t] = wn[t];
        }
    }
}

// Gate nonlinearities on the hardware transcendentals (gru_update below): sigmoid(x) = rcp(1 + exp2(-x log2 e)),
// tanh(x) = 2 sigmoid(2x) - 1 (v_exp_f32 / v_rcp_f32, ~1 ulp each; absolute error of tanh ~1e-7 near 0).
// PyTorch's CPU kernels are not bit-reproducible either; the logit tolerance (tests) covers both.

// PyTorch GRUCell update on one 32x32 tile pair: h = (h - n) * z + n,
// r = sigmoid(a_r), z = sigmoid(a_z), n = tanh(a_in + r * a_hn)
// The fp32 MFMAs and this VALU work do not co-issue (PMC: MFMA-busy + VALU-active ~ 1), so the update's
// instruction count is on the critical path: element pairs go through v_pk_mul/add/fma_f32 (two lanes'
// worth of fp32 per instruction); only exp2 / rcp stay scalar.  Same operations and rounding per element.
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v exp2_2(f2v x) { return f2v{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)}; }
__device__ __forceinline__ f2v rcp_2(f2v x) { return f2v{__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)}; }

// FOLD: the image's gate rows were pre-multiplied by their exp2 constants (build_image(..., fold)): the accumulators
// already hold -log2(e) a (r, z) and -2 log2(e) a (n), so no scaling multiply per gate
// gemm_chain with the A operands in global memory (the out_linear_depth > 1 head's image: a few KB, the same for every
// wave, so they come from L1 / L2), one group of 4 k-steps ahead of the MFMAs
template <int KG, int NT, int HT>
__device__ __forceinline__ void gemm_chain_g(const f4* __restrict__ W, int lane, f16v (&acc)[NT], const f16v (&h)[HT]) {
    f4 wc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wc[t] = W[(t * KG) * 64 + lane];
#pragma unroll
    for (int s4 = 0; s4 < KG; ++s4) {
        f4 wn[NT];
        if (s4 + 1 < KG) {
#pragma unroll
            for (int t = 0; t < NT; ++t) wn[t] = W[(t * KG + s4 + 1) * 64 + lane];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = 4 * s4 + e;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma(wc[t][e], h[s >> 4][s & 15], acc[t]);
        }
        if (s4 + 1 < KG) {
#pragma unroll
            for (int t = 0; t < NT; ++t) wc[t] = wn[t];
        }
    }
}

// nn.SELU (the out_linear_depth > 1 head's activation, rnn_all.py:336-343)
__device__ __forceinline__ float selu(float x) {
    return 1.0507009873554805f * (x > 0.0f ? x : 1.6732632423543772f * expm1f(x));
}

// head image (floats): per hidden layer l = 0 .. depth - 2: A operands [HDT tiles][K_l / 8 groups][64 lanes][4] (K_0 = F,
// else 32 HDT), then its bias in accumulator order [HDT][2 halves][16]; then the last Linear's weights [2][HDT][16]
__host__ __device__ inline int head_layer_off(int l, int F, int hdt) {
    return l == 0 ? 0 : hdt * (F / 8) * 256 + hdt * 32 + (l - 1) * (hdt * (4 * hdt) * 256 + hdt * 32);
}

template <bool FOLD = false>
__device__ __forceinline__ void gru_update(f16v& h, const f16v& ar, const f16v& az, const f16v& ain, const f16v& ahn) {
    const f2v one = {1.0f, 1.0f};
    const f2v two = {2.0f, 2.0f};
    // (2x)(-log2 e) == x(-2 log2 e), both exact scalings
    constexpr float k1 = FOLD ? 1.0f : -1.44269504088896340736f, k2 = FOLD ? 1.0f : -2.88539008177792681472f;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        f2v er = f2v{ar[i], ar[i + 1]}, ez = f2v{az[i], az[i + 1]};
        if constexpr (!FOLD) {
            er = f2v{k1, k1} * er;
            ez = f2v{k1, k1} * ez;
        }
        const f2v r = rcp_2(one + exp2_2(er));
        const f2v z = rcp_2(one + exp2_2(ez));
        f2v x = f2v{ain[i], ain[i + 1]} + f2v{ahn[i], ahn[i + 1]} * r;
        if constexpr (!FOLD) x = f2v{k2, k2} * x;
        const f2v s2 = rcp_2(one + exp2_2(x));
        const f2v nn = __builtin_elementwise_fma(two, s2, -one);
        const f2v hv = f2v{h[i], h[i + 1]};
        const f2v hn = (hv - nn) * z + nn;
        h[i] = hn.x;
        h[i + 1] = hn.y;
    }
}

// Waves per workgroup of the F <= 64 kernels: all share the workgroup's LDS copy of the weights.  8 waves
// would put two on every SIMD (one wave's gate VALU work overlapping the other's MFMAs), but at <= 256
// registers per wave the F = 64, 2-layer kernel spills (P, both states, the gate accumulators and the
// weight look-ahead need ~300): measured 0.63 of the fp32 MFMA peak vs 0.77 with 4 waves.
#define NPD_GRU_WPB 4  // measured: 8 waves spill 716 B/lane and run 0.63 vs 0.77 of peak
#ifndef NPD_GRU_BF_WPB
#define NPD_GRU_BF_WPB 4
#endif

}  // namespace gru
}  // namespace npd

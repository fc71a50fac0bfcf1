// npd_gru_train.hpp -- training of the CRISP GRU (RNN_decoder.decode(net, True, ...), rnn_all.py:422-512) on fused
// kernels (npd_gru_train.hip): the plan handle, the flat weight vector's offsets, the two LDS images' layouts and the
// layout of the caller's saved / scratch buffers.
#pragma once

#include "npd_gru_host.hpp"

// The plan of one shape: it owns the device images only; the weights come with every call (they change every
// optimiser step) and are packed into the images on the device.  One plan serves one stream at a time.
struct npd_gru_train {
    int N, F, layers, onehot, device;
    float* img_f;  // forward image: gemm_chain A operands of [W_hh0, W_ih1, W_hh1], then the vectors (TGeo::V_*)
    float* wy;     // forward y projection A operands (fill_wy's order)
    float* img_b;  // backward image: A operands of the three transposed matrices, then the Linear weights
};

namespace npd {
namespace gru {

// offsets (floats) into the flat weight / gradient vector, npd_gru_create order
struct TrainOff {
    int64_t wih[2], whh[2], bih[2], bhh[2], wlin, blin, total;
    int Din;
};
__host__ __device__ inline TrainOff train_off(int N, int F, int L, int onehot) {
    TrainOff o{};
    o.Din = N + (onehot ? 2 : 1);
    int64_t p = 0;
    for (int l = 0; l < 2; ++l) {
        if (l >= L) {
            o.wih[l] = o.whh[l] = o.bih[l] = o.bhh[l] = 0;
            continue;
        }
        o.wih[l] = p; p += (int64_t)3 * F * (l == 0 ? o.Din : F);
        o.whh[l] = p; p += (int64_t)3 * F * F;
        o.bih[l] = p; p += 3 * F;
        o.bhh[l] = p; p += 3 * F;
    }
    o.wlin = p; p += F;
    o.blin = p; p += 1;
    o.total = p;
    return o;
}

template <int F, int L>
struct TGeo {
    using G = Geo<F, L>;
    static constexpr int TT = G::TT, HT = G::HT, KG = G::KG, NG = G::NG;
    static constexpr int MATS = NG * G::G_SIZE;
    // forward vectors, 32 floats each in accumulator-register order [lane half][register i] (row (i&3) + 8(i>>2) + 4 half)
    static constexpr int V_B0 = 0;              // TT tiles: layer-0 r, z rows b_ih + b_hh; n rows b_ih
    static constexpr int V_XA = TT;             // TT: W_ih0[:, N] (the fed value's column; onehot: index 0's)
    static constexpr int V_XB = 2 * TT;         // TT: onehot W_ih0[:, N + 1], else 0
    static constexpr int V_HN0 = 3 * TT;        // HT: layer-0 b_hh of the n rows
    static constexpr int V_B1 = 3 * TT + HT;    // TT: layer 1, as V_B0
    static constexpr int V_HN1 = 4 * TT + HT;   // HT
    static constexpr int V_WL = 4 * TT + 2 * HT;  // HT: Linear weights
    static constexpr int NV = 4 * TT + 3 * HT;
    static constexpr int OFF_V = MATS;
    static constexpr int F_TOTAL = MATS + NV * 32;
    // backward: W^T (F x 3F) as HT row tiles over 3F/2 k-steps
    static constexpr int KGB = 3 * F / 8;
    static constexpr int B_GSIZE = HT * KGB * 256;
    static constexpr int B_MATS = NG * B_GSIZE;
    static constexpr int B_OFF_WL = B_MATS;
    static constexpr int B_TOTAL = B_MATS + HT * 32;
};

inline int64_t train_fwd_image_floats(int F, int L) {
    const int TT = 3 * F / 32, HT = F / 32, NG = L == 2 ? 3 : 1;
    return (int64_t)NG * TT * (F / 8) * 256 + (4 * TT + 3 * HT) * 32;
}
inline int64_t train_bwd_image_floats(int F, int L) {
    const int HT = F / 32, NG = L == 2 ? 3 : 1;
    return (int64_t)NG * HT * (3 * F / 8) * 256 + HT * 32;
}
inline int64_t train_wy_floats(int N, int F) { return (int64_t)(3 * F / 32) * (N / 8) * 256; }

// ---- the caller's buffers.  NB = N B samples, sample (step ii, word w) = ii B + w.
// saved:   5 L arrays [NB][F] -- layer l: h' (5l), r (5l + 1), z (5l + 2), n (5l + 3), a_hn = W_hn h + b_hn (5l + 4) --
//          then aux [NB][3] = [1, xa, xb], the fed input as the layer-0 columns see it (onehot: xa, xb = the one-hot
//          pair; else xa = the fed value, xb = 0)
// scratch: L arrays [NB][4F] of Delta = [da_r, da_z, da_in, da_hn], then the step-major grad_out [NB], then the
//          contraction's partial sums
constexpr int kTrainMaxJobs = 12;
// splits of the samples: ~256 per workgroup keeps one fp32 accumulation chain short (128 MFMAs), at most 256 partials
inline int train_splits(int64_t NB) {
    const int64_t p = (NB + 255) / 256;
    return (int)(p < 1 ? 1 : (p > 256 ? 256 : p));
}
// outputs (M x Nc, summed over the jobs) of the weight-gradient contraction = the flat vector's length
inline int64_t train_saved_floats(int N, int F, int L, int64_t B) { return (int64_t)N * B * (5 * L * F + 3); }
inline int64_t train_scratch_floats(int N, int F, int L, int onehot, int64_t B) {
    const int64_t NB = (int64_t)N * B;
    return NB * (4 * F * L + 1) + (int64_t)train_splits(NB) * train_off(N, F, L, onehot).total;
}

}  // namespace gru
}  // namespace npd

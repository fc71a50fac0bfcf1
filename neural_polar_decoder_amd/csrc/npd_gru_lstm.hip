// npd_gru_lstm.hip -- LSTM cells (fp32) with LDS-resident weights: F = 32 (1-2 layers) and F = 64 x 1; the other
// shapes run lstm_wide_kernel (npd_gru_wide.hip) on the same image.
// rnn_all.py:69 offers --rnn_type LSTM; RNN_decoder's y_input test branch then carries (h, c) pairs (rnn_all.py:536-547)
// through nn.LSTM: gates i, f, g, o (PyTorch row order) = W_ih x + b_ih + W_hh h + b_hh, c' = sig(f) c + sig(i) tanh(g),
// h' = sig(o) tanh(c').  Same layout as gru_decode_kernel with 4F gate rows: images [L0 hh | L1 ih | L1 hh] of 4F x F in
// A-operand order, every gate row pre-multiplied by its exp2 constant (i, f, o: -log2 e; g: -2 log2 e), all biases
// (+ the one-hot column 0 on layer 0) as accumulator initialisation, the x_i column one [1, x_i] k-step on layer 0.
#include "npd_gru_host.hpp"

namespace npd {
namespace gru {

template <int F, int L>
__global__ __launch_bounds__(64 * NPD_GRU_WPB) void lstm_decode_kernel(const Args a) {
    using G = LGeo<F, L>;
    constexpr int TT = G::TT, HT = G::HT, KG = G::KG;
    extern __shared__ __attribute__((aligned(16))) f4 smem4[];
    const float* smem = reinterpret_cast<const float*>(smem4);
    {
        const f4* src = reinterpret_cast<const f4*>(a.img);
        for (int i = threadIdx.x; i < G::TOTAL / 4; i += blockDim.x) smem4[i] = src[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    const int col = lane & 31;
    const int N = a.N;
    const int64_t ntiles = (a.B + 31) / 32;
    const f16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto cvec = [&](int off) -> f16v {
        const f4* p = reinterpret_cast<const f4*>(smem + off + half * 16);
        const f4 x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
        return f16v{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3],
                    x2[0], x2[1], x2[2], x2[3], x3[0], x3[1], x3[2], x3[3]};
    };
    constexpr float kT = -2.88539008177792681472f;  // tanh(c) = 2 sig2(kT c) - 1
    for (int64_t tile = (int64_t)blockIdx.x * NPD_GRU_WPB + wave; tile < ntiles; tile += (int64_t)gridDim.x * NPD_GRU_WPB) {
        const int64_t cw = tile * 32 + col;
        const bool valid = cw < a.B;
        const int64_t cwc = valid ? cw : a.B - 1;
        f16v P[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) P[t] = cvec(G::OFF_CV + t * 32);
        if (a.y) {  // y = NULL: decoding_type y_h0 (no y input; the state starts from the y-MLP's output)
            const f4* yr = reinterpret_cast<const f4*>(a.y + cwc * N + half * (N / 2));
            const int ng = N / 8;
            for (int s4 = 0; s4 < ng; ++s4) {
                const f4 yv = yr[s4];
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    const f4 w = a.wy[(t * ng + s4) * 64 + lane];
                    P[t] = mfma(w.x, yv.x, P[t]);
                    P[t] = mfma(w.y, yv.y, P[t]);
                    P[t] = mfma(w.z, yv.z, P[t]);
                    P[t] = mfma(w.w, yv.w, P[t]);
                }
            }
        }
        f16v h0[HT], c0[HT], h1[HT], c1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            h0[t] = zero;
            c0[t] = zero;
            h1[t] = zero;
            c1[t] = zero;
        }
        if (a.h0) {  // y_h0: get_h0 returns (x, x) for LSTM cells (rnn_all.py:370-375): h and c both start from x
            const float* hr = a.h0 + cwc * (int64_t)(F * L);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int f = hid_of(16 * t + i, half);
                    h0[t][i] = c0[t][i] = hr[f * L];
                    if constexpr (L == 2) h1[t][i] = c1[t][i] = hr[f * L + 1];
                }
        }
        float xb = 1.0f;
        auto cell = [&](f16v& h, f16v& c, const f16v (&acc)[TT], int j) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float ig = sig2(acc[j][i]), fg = sig2(acc[HT + j][i]);
                const float gg = fmaf(2.0f, sig2(acc[2 * HT + j][i]), -1.0f);
                const float og = sig2(acc[3 * HT + j][i]);
                c[i] = fmaf(fg, c[i], ig * gg);
                h[i] = og * fmaf(2.0f, sig2(kT * c[i]), -1.0f);
            }
        };
        for (int ii = 0; ii < N; ++ii) {
            const int jj = a.rev ? N - 1 - ii : ii;
            const float xbe = half ? xb : 1.0f;
            {
                f16v acc[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t] = mfma(smem[G::OFF_X + t * 64 + lane], xbe, P[t]);
                gemm_chain<TT, KG, TT, HT>(smem4, 0, 0, lane, acc, h0);
#pragma unroll
                for (int j = 0; j < HT; ++j) cell(h0[j], c0[j], acc, j);
            }
            if constexpr (L == 2) {
                f16v acc1[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc1[t] = cvec(G::OFF_CV + (TT + t) * 32);
                gemm_chain<TT, KG, TT, HT>(smem4, 1, 0, lane, acc1, h0);
                gemm_chain<TT, KG, TT, HT>(smem4, 2, 0, lane, acc1, h1);
#pragma unroll
                for (int j = 0; j < HT; ++j) cell(h1[j], c1[j], acc1, j);
            }
            float part = 0.0f;
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) part += smem[G::OFF_WL + (half * HT + t) * 16 + i] * (L == 2 ? h1[t][i] : h0[t][i]);
            const float out = part + __shfl_xor(part, 32, 64) + a.b_lin;
            const bool info = (a.info[jj >> 5] >> (jj & 31)) & 1u;
            float d;
            if (info) d = out > 0.0f ? 1.0f : (out < 0.0f ? -1.0f : 0.0f);
            else d = a.gt ? a.gt[cwc * N + jj] : 1.0f;
            if (half == 0 && valid) {
                a.decoded[cw * N + jj] = d;
                if (a.logits) a.logits[cw * N + ii] = out;
            }
            const float sd = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            xb = a.onehot ? (sd > 0.0f ? 1.0f : 0.0f) : sd;
        }
    }
}

// host image of lstm_decode_kernel from the npd_gru_create weight order with 4F gate rows
template <int F, int L>
static void build_image_lstm(const float* W, int N, int onehot, std::vector<float>& img, std::vector<float>& wy,
                             float& b_lin) {
    using G = LGeo<F, L>;
    constexpr int TT = G::TT, HT = G::HT;
    const int Din = N + (onehot ? 2 : 1);
    const Weights u = unpack_weights(W, 4, F, L, Din);
    const auto &wih = u.wih, &bih = u.bih, &bhh = u.bhh;
    b_lin = u.b_lin;
    img.assign(G::TOTAL, 0.0f);
    auto fr = [&](int row) { return (row >= 2 * F && row < 3 * F) ? -2.88539008177792681472f : -1.44269504088896340736f; };
    fill_mats(u, G::NG, TT, F, fr, img);
    // layer-0 [1, x_i] k-step: half 0 pairs with 1 (nothing left: the one-hot column 0 is in the bias tile), half 1
    // with x_i (one-hot: column 1 - column 0; sign input: its column)
    for (int t = 0; t < TT; ++t)
        for (int l = 32; l < 64; ++l) {
            const int row = 32 * t + (l & 31);
            const float v = onehot ? wih[0][(size_t)row * Din + N + 1] - wih[0][(size_t)row * Din + N]
                                   : wih[0][(size_t)row * Din + N];
            img[G::OFF_X + t * 64 + l] = fr(row) * v;
        }
    for (int hf = 0; hf < 2; ++hf)
        for (int t = 0; t < HT; ++t)
            for (int i = 0; i < 16; ++i) img[G::OFF_WL + (hf * HT + t) * 16 + i] = u.wlin[32 * t + (i & 3) + 8 * (i >> 2) + 4 * hf];
    for (int l = 0; l < L; ++l)
        for (int t = 0; t < TT; ++t)
            for (int hf = 0; hf < 2; ++hf)
                for (int i = 0; i < 16; ++i) {
                    const int row = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * hf;
                    float v = bih[l][row] + bhh[l][row];
                    if (l == 0 && onehot) v += wih[0][(size_t)row * Din + N];
                    img[G::OFF_CV + ((l * TT + t) * 2 + hf) * 16 + i] = fr(row) * v;
                }
    fill_wy(wih[0], TT, N, Din, fr, wy);
}

void build_image_lstm(int F, int L, const float* W, int N, int onehot, std::vector<float>& img, std::vector<float>& wy,
                      float& b_lin) {
    dispatch(AllShapes{}, [&](auto f, auto l) { build_image_lstm<f.value, l.value>(W, N, onehot, img, wy, b_lin); },
             F, L);
}

int launch_lstm(const npd_gru* g, const Args& a, hipStream_t s) {
    const int grid = grid_for(((a.B + 31) / 32 + NPD_GRU_WPB - 1) / NPD_GRU_WPB, 1, device_cu_count());
    return dispatch(Combos<Combo<64, 1>, Combo<32, 2>, Combo<32, 1>>{}, [&](auto f, auto l) {
        return launch_lds<lstm_decode_kernel<f.value, l.value>>("lstm_decode_kernel launch", grid, 64 * NPD_GRU_WPB,
                                                                (size_t)LGeo<f.value, l.value>::TOTAL * 4, s, a);
    }, g->F, g->layers);
}

}  // namespace gru
}  // namespace npd

// npd_gru.hip -- CRISP GRU autoregressive decoder (RNN_decoder.decode, y_input, test branch).
//
// Reference: rnn_all.py:294-398 (RNN_Model: nn.GRU(N+2, F, layers) + Linear(F, 1)), rnn_all.py:532-547
// (per-bit loop: x_i = [y, onehot(prev)], one GRU step, d_i = sign(out) on information positions),
// get_onehot rnn_all.py:258-260, PyTorch GRUCell (r, z, n gate order; h' = (h - n) * z + n).
//
// MI355X design: the per-step matvecs of all codewords of a wave form GEMMs
//   gates^T (3F x 32 codewords) = W (3F x F) . h^T (F x 32)
// computed with v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains).  Gate rows are the MFMA rows and
// codewords the columns, so a 32x32 accumulator tile of h' is, register for register, the B operand
// of the next step's MFMAs (no transpose, no LDS round trip for the state); the weight matrices are
// permuted once on the host into the matching A-operand order and live in LDS for the whole launch
// (one 256-thread workgroup per CU, four waves, 32 codewords per wave).  The y part of the input
// projection, W_ih0[:, :N] y, is constant over the N steps and computed once per codeword (P); the
// one-hot / previous-decision column and all biases are folded into one extra MFMA k-step whose B
// operand is [1, x_i].
#include "npd_gru_host.hpp"

namespace npd {
namespace gru {

// The image's gate rows carry their exp2 constants (build_image(..., fold = true)) and the biases initialise the
// accumulators (Geo::OFF_CV): only layer 0's r, z tiles keep the [1, x_i] k-step.  Measured in round 3 (same box,
// alternating, 2^20 Polar(64,32) words): folding 41.0 -> 40.3 ms, bias initialisation 40.07 -> 39.70 ms.
template <int F, int L, int WPB = NPD_GRU_WPB, int HDT = 0>
__global__ __launch_bounds__(64 * WPB) void gru_decode_kernel(const Args a) {
    constexpr bool FOLD = true, BINIT = true;
    using G = Geo<F, L>;
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
    // this lane's 16 accumulator-row values of a bias vector tile at float offset `off` (Geo::OFF_CV region)
    auto cvec = [&](int off) -> f16v {
        const f4* p = reinterpret_cast<const f4*>(smem + off + half * 16);
        const f4 x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
        return f16v{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3],
                    x2[0], x2[1], x2[2], x2[3], x3[0], x3[1], x3[2], x3[3]};
    };

    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < ntiles; tile += (int64_t)gridDim.x * WPB) {
        const int64_t cw = tile * 32 + col;
        const bool valid = cw < a.B;
        const int64_t cwc = valid ? cw : a.B - 1;

        // ---- P = W_ih0[:, :N] . y  (k-step s pairs y[s] (half 0) with y[s + N/2] (half 1))
        f16v P[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) P[t] = zero;
        if (a.y) {
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

        f16v h0[HT], h1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            h0[t] = zero;
            h1[t] = zero;
        }
        if (a.h0) {  // register i of tile t = hidden unit hid_of(16 t + i, half) of codeword col
            const float* hr = a.h0 + cwc * (int64_t)(F * L);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int f = hid_of(16 * t + i, half);
                    h0[t][i] = hr[f * L];
                    if constexpr (L == 2) h1[t][i] = hr[f * L + 1];
                }
        }
        float xb = 1.0f;  // x_i: onehot index of the previous decision (or its sign); step 0: prev = +1
        const float one_or_zero = half ? 0.0f : 1.0f;

        for (int ii = 0; ii < N; ++ii) {
            const int jj = a.rev ? N - 1 - ii : ii;
            const float xbe = half ? xb : 1.0f;  // extra k-step B operand: [1, x_i]
            // ================= layer 0: acc = P + W_hh0 h0 + consts + x_i column
            {
                f16v acc[TT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) acc[t] = P[t];
#pragma unroll
                for (int t = 2 * HT; t < TT; ++t) acc[t] = BINIT ? cvec(G::OFF_CV + (t - 2 * HT) * 32) : zero;
                gemm_chain<TT, KG, TT, HT>(smem4, 0, 0, lane, acc, h0);
                // the [1, x_i] k-step: every tile, or (BINIT: hn tiles start from their bias) the r, z tiles only
#pragma unroll
                for (int t = 0; t < (BINIT ? 2 * HT : TT); ++t) acc[t] = mfma(smem[G::OFF_X + t * 64 + lane], xbe, acc[t]);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    const f16v ain = mfma(smem[G::OFF_IN + j * 64 + lane], xbe, P[2 * HT + j]);
                    gru_update<FOLD>(h0[j], acc[j], acc[HT + j], ain, acc[2 * HT + j]);
                }
            }
            if constexpr (L == 2) {
                // ================= layer 1: acc1 = W_ih1 h0' (+ W_hh1 h1 on r,z rows); ahn = W_hh1_n h1
                f16v acc1[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc1[t] = BINIT ? cvec(G::OFF_CV + (HT + t) * 32) : zero;
                gemm_chain<TT, KG, TT, HT>(smem4, 1, 0, lane, acc1, h0);
                if constexpr (!BINIT) {
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc1[t] = mfma(smem[G::OFF_X + (TT + t) * 64 + lane], one_or_zero, acc1[t]);
                }
                f16v arz[2 * HT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) arz[t] = acc1[t];
                gemm_chain<TT, KG, 2 * HT, HT>(smem4, 2, 0, lane, arz, h1);
                f16v ahn[HT];
#pragma unroll
                for (int j = 0; j < HT; ++j) ahn[j] = BINIT ? cvec(G::OFF_CV + (HT + TT + j) * 32) : zero;
                gemm_chain<TT, KG, HT, HT>(smem4, 2, 2 * HT, lane, ahn, h1);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    if constexpr (!BINIT) ahn[j] = mfma(smem[G::OFF_X + (2 * TT + 2 * HT + j) * 64 + lane], one_or_zero, ahn[j]);
                    gru_update<FOLD>(h1[j], arz[j], arz[HT + j], acc1[2 * HT + j], ahn[j]);
                }
            }
            // ================= output: Linear(F, 1) on the top layer
            float part = 0.0f;
#pragma unroll
            for (int t = 0; t < HT; ++t) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float wl = smem[G::OFF_WL + (half * HT + t) * 16 + i];
                    part += wl * (L == 2 ? h1[t][i] : h0[t][i]);
                }
            }
            float out;
            if constexpr (HDT > 0) {
                // out_linear_depth > 1 head (rnn_all.py:336-343: Linear(F, H), SELU, [Linear(H, H), SELU] ..., Linear(H, 1)),
                // H padded to 32 HDT with zero rows / columns: each layer is a GEMM whose accumulator tiles are,
                // register for register, the next layer's B operand (as the GRU states are)
                const float* hdf = reinterpret_cast<const float*>(a.hd);
                f16v hx[HDT];
                auto bias_init = [&](int l, f16v (&acc)[HDT]) {
                    const int boff = head_layer_off(l, F, HDT) + HDT * (l == 0 ? F / 8 : 4 * HDT) * 256;
#pragma unroll
                    for (int t = 0; t < HDT; ++t) {
                        const f4* p = reinterpret_cast<const f4*>(hdf + boff + (t * 2 + half) * 16);
                        const f4 x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
                        acc[t] = f16v{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3],
                                      x2[0], x2[1], x2[2], x2[3], x3[0], x3[1], x3[2], x3[3]};
                    }
                };
                bias_init(0, hx);
                if constexpr (L == 2) gemm_chain_g<F / 8, HDT, HT>(a.hd, lane, hx, h1);
                else gemm_chain_g<F / 8, HDT, HT>(a.hd, lane, hx, h0);
#pragma unroll
                for (int t = 0; t < HDT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) hx[t][i] = selu(hx[t][i]);
                for (int l = 1; l < a.hd_depth - 1; ++l) {
                    f16v hn[HDT];
                    bias_init(l, hn);
                    gemm_chain_g<4 * HDT, HDT, HDT>(a.hd + head_layer_off(l, F, HDT) / 4, lane, hn, hx);
#pragma unroll
                    for (int t = 0; t < HDT; ++t)
#pragma unroll
                        for (int i = 0; i < 16; ++i) hx[t][i] = selu(hn[t][i]);
                }
                const float* wo = hdf + head_layer_off(a.hd_depth - 1, F, HDT);
                float po = 0.0f;
#pragma unroll
                for (int t = 0; t < HDT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) po = fmaf(wo[(half * HDT + t) * 16 + i], hx[t][i], po);
                out = po + __shfl_xor(po, 32, 64) + a.hd_bout;
            } else if (a.ln) {
                // LayerNorm head (rnn_all.py:387-398: linear(layernorm(out))): two-pass mean / biased variance over the
                // F units of this codeword, then sum_i w_i gamma_i (h_i - mu) rstd + (b + w . beta) with the
                // gamma-folded weights in the image (npd_rnn_create_ex)
                float s1 = 0.0f;
#pragma unroll
                for (int t = 0; t < HT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s1 += L == 2 ? h1[t][i] : h0[t][i];
                const float mu = (s1 + __shfl_xor(s1, 32, 64)) * (1.0f / (float)F);
                float s2 = 0.0f, pw = 0.0f;
#pragma unroll
                for (int t = 0; t < HT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float d = (L == 2 ? h1[t][i] : h0[t][i]) - mu;
                        s2 = fmaf(d, d, s2);
                        pw = fmaf(smem[G::OFF_WL + (half * HT + t) * 16 + i], d, pw);
                    }
                const float var = (s2 + __shfl_xor(s2, 32, 64)) * (1.0f / (float)F);
                out = (pw + __shfl_xor(pw, 32, 64)) / sqrtf(var + a.ln_eps) + a.b_lin;
            } else {
                out = part + __shfl_xor(part, 32, 64) + a.b_lin;
            }
            const bool info = (a.info[jj >> 5] >> (jj & 31)) & 1u;
            float d;
            if (info) {
                d = out > 0.0f ? 1.0f : (out < 0.0f ? -1.0f : 0.0f);
            } else {
                d = a.gt ? a.gt[cwc * N + jj] : 1.0f;
            }
            if (half == 0 && valid) {
                a.decoded[cw * N + jj] = d;
                if (a.logits) a.logits[cw * N + ii] = out;
            }
            // next input: onehot(sign(d)) -> index (0.5 + 0.5*s).long() (rnn_all.py:258-260); else sign(d)
            const float sd = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            xb = a.onehot ? (sd > 0.0f ? 1.0f : 0.0f) : sd;
        }
    }
}

// ---------------------------------------------------------------------------------- host image
template <int F, int L>
static void build_image(const float* W, int N, int onehot, std::vector<float>& img, std::vector<float>& wy,
                        float& b_lin, bool fold = false) {
    using G = Geo<F, L>;
    constexpr int TT = G::TT, HT = G::HT;
    const int Din = N + (onehot ? 2 : 1);
    const Weights u = unpack_weights(W, 3, F, L, Din);
    const auto &wih = u.wih, &bih = u.bih, &bhh = u.bhh;
    b_lin = u.b_lin;
    img.assign(G::TOTAL, 0.0f);
    // fold: every gate row times its exp2 constant (r, z: -log2 e; n: -2 log2 e; one fp32 rounding), the kernel's
    // gate nonlinearities then take the accumulators as they are (gru_update<true>)
    auto fr = [&](int row) { return fold ? (row < 2 * F ? -1.44269504088896340736f : -2.88539008177792681472f) : 1.0f; };
    fill_mats(u, G::NG, TT, F, fr, img);
    // extra k-step A operands: column 0 pairs with B = 1, column 1 with B = x_i (layer 0) / 0 (layer 1)
    for (int t = 0; t < TT; ++t)
        for (int l = 0; l < 64; ++l) {
            const int row = 32 * t + (l & 31);
            const int kk = l >> 5;
            const bool rz = row < 2 * F;
            // layer 0, hidden-side image: r,z rows carry every input-side constant too
            float v0;
            if (kk == 0) {
                v0 = rz ? bih[0][row] + bhh[0][row] + (onehot ? wih[0][(size_t)row * Din + N] : 0.0f) : bhh[0][row];
            } else {
                v0 = rz ? (onehot ? wih[0][(size_t)row * Din + N + 1] - wih[0][(size_t)row * Din + N]
                                  : wih[0][(size_t)row * Din + N])
                        : 0.0f;
            }
            img[G::OFF_X + (0 * TT + t) * 64 + l] = fr(row) * v0;
            if (L == 2) {
                img[G::OFF_X + (1 * TT + t) * 64 + l] = fr(row) * (kk == 0 ? (rz ? bih[1][row] + bhh[1][row] : bih[1][row]) : 0.0f);
                img[G::OFF_X + (2 * TT + t) * 64 + l] = fr(row) * (kk == 0 ? (rz ? 0.0f : bhh[1][row]) : 0.0f);
            }
        }
    for (int j = 0; j < HT; ++j)
        for (int l = 0; l < 64; ++l) {
            const int row = 2 * F + 32 * j + (l & 31);
            const int kk = l >> 5;
            float v;
            if (kk == 0) v = bih[0][row] + (onehot ? wih[0][(size_t)row * Din + N] : 0.0f);
            else v = onehot ? wih[0][(size_t)row * Din + N + 1] - wih[0][(size_t)row * Din + N] : wih[0][(size_t)row * Din + N];
            img[G::OFF_IN + j * 64 + l] = fr(row) * v;
        }
    for (int hf = 0; hf < 2; ++hf)
        for (int t = 0; t < HT; ++t)
            for (int i = 0; i < 16; ++i) img[G::OFF_WL + (hf * HT + t) * 16 + i] = u.wlin[32 * t + (i & 3) + 8 * (i >> 2) + 4 * hf];
    for (int v = 0; v < 2 * HT + TT; ++v)
        for (int hf = 0; hf < 2; ++hf)
            for (int i = 0; i < 16; ++i) {
                const int r = (i & 3) + 8 * (i >> 2) + 4 * hf;
                float val = 0.0f;
                int row;
                if (v < HT) {  // layer-0 hn bias
                    row = 2 * F + 32 * v + r;
                    val = bhh[0][row];
                } else if (v < HT + TT) {  // layer-1 r, z (both biases) / in (b_ih) constants
                    row = 32 * (v - HT) + r;
                    val = L == 2 ? (row < 2 * F ? bih[1][row] + bhh[1][row] : bih[1][row]) : 0.0f;
                } else {  // layer-1 hn bias
                    row = 2 * F + 32 * (v - HT - TT) + r;
                    val = L == 2 ? bhh[1][row] : 0.0f;
                }
                img[G::OFF_CV + (v * 2 + hf) * 16 + i] = fr(row) * val;
            }
    fill_wy(wih[0], TT, N, Din, fr, wy);
}

// the out_linear_depth > 1 head's image (layout: head_layer_off): hw = the Sequential's Linear layers in order, W_0 (H, F),
// b_0 (H), [W_l (H, H), b_l (H)] for l = 1 .. depth - 2, W_last (1, H), b_last (1); H padded to 32 hdt with zeros
void build_head_image(const float* hw, int F, int H, int depth, int hdt, std::vector<float>& img, float& bout) {
    const int HP = 32 * hdt;
    img.assign((size_t)head_layer_off(depth - 1, F, hdt) + 2 * hdt * 16, 0.0f);
    const float* p = hw;
    for (int l = 0; l < depth - 1; ++l) {
        const int K = l == 0 ? F : H, KP = l == 0 ? F : HP, KG = KP / 8;
        const float* W = p;
        const float* b = p + (size_t)H * K;
        p = b + H;
        float* im = img.data() + head_layer_off(l, F, hdt);
        for (int t = 0; t < hdt; ++t)
            for (int s = 0; s < KP / 2; ++s)
                for (int ln = 0; ln < 64; ++ln) {
                    const int row = 32 * t + (ln & 31), k = hid_of(s, ln >> 5);
                    im[((size_t)(t * KG + s / 4) * 64 + ln) * 4 + (s & 3)] = row < H && k < K ? W[(size_t)row * K + k] : 0.0f;
                }
        float* bv = im + (size_t)hdt * KG * 256;
        for (int t = 0; t < hdt; ++t)
            for (int hf = 0; hf < 2; ++hf)
                for (int i = 0; i < 16; ++i) {
                    const int row = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * hf;
                    bv[(t * 2 + hf) * 16 + i] = row < H ? b[row] : 0.0f;
                }
    }
    float* wo = img.data() + head_layer_off(depth - 1, F, hdt);
    for (int hf = 0; hf < 2; ++hf)
        for (int t = 0; t < hdt; ++t)
            for (int i = 0; i < 16; ++i) {
                const int k = hid_of(16 * t + i, hf);
                wo[(hf * hdt + t) * 16 + i] = k < H ? p[k] : 0.0f;
            }
    bout = p[H];
}

void build_image(int F, int L, const float* W, int N, int onehot, bool fold, std::vector<float>& img,
                 std::vector<float>& wy, float& b_lin) {
    dispatch(AllShapes{}, [&](auto f, auto l) { build_image<f.value, l.value>(W, N, onehot, img, wy, b_lin, fold); },
             F, L);
}

// the out_linear_depth > 1 head on 1, 2 or 4 tiles of 32 head units, or (HDT 0) the plain Linear / LayerNorm head
int launch_f32(const npd_gru* g, const Args& a, hipStream_t s) {
    constexpr int WPB = NPD_GRU_WPB;
    const int grid = grid_for(((a.B + 31) / 32 + WPB - 1) / WPB, 1, device_cu_count());
    return dispatch(NarrowShapes{}, [&](auto f, auto l) {
        return dispatch(Combos<Combo<1>, Combo<2>, Combo<4>, Combo<0>>{}, [&](auto hdt) {
            return launch_lds<gru_decode_kernel<f.value, l.value, WPB, hdt.value>>(
                "gru_decode_kernel launch", grid, 64 * WPB, (size_t)Geo<f.value, l.value>::TOTAL * 4, s, a);
        }, g->hd ? g->hd_tiles : 0);
    }, g->F, g->layers);
}

}  // namespace gru
}  // namespace npd

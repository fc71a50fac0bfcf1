// npd_xfdec.hip -- XFormerEndToEndDecoder.decode (models.py:599-654, --model decoder) in one launch, fp32 on
// v_mfma_f32_32x32x2_f32.
//
// What decode computes (with the masking branch under which the reference runs at any batch size).  Once per word the
// memory Mem[j] = LN_cross(y_j emb_cross[j + 1] + table_5000[j]), j = 0 .. N - 1: there is no encoder stack.  At every
// information position i the whole layer stack runs on the decoder tokens D[t] = LN_dec(emb_inputs[idx_t] +
// table_10000[t]) (idx_0 = 2, idx_t = 1 if the bit at position t - 1 is +1, else 0); in every layer
//   * self-attention with the single mask row i: every token 0 .. i attends to every key <= i, so the kernel works on
//     the prefix of n = i + 1 tokens, as the GPT kernel does (it is not a KV-cached causal decode);
//   * cross-attention, in every layer: queries from the tokens, keys and values from all N rows of Mem;
//   * the FFN;
// and logit_i = Lin_Decoder(token i).
//
// Mapping: npd_xformer.hpp's, G = 64 / N codewords per workgroup, their prefixes stacked into M = G n rows.  A seventh
// LDS buffer holds Mem (row g N + j).  The cross keys and values of a layer are recomputed from Mem at every step into
// the K and V buffers, once the layer's self-attention has been folded into X: all layers' cross K / V would need
// 2 L 64 x 68 floats, 209 KB at 6 layers, more than LDS holds.  The last layer runs fc, the cross-attention queries,
// the FFN and all three LayerNorms for token i only (G compact rows).  The decoder tokens take three values per
// position, so create() tabulates LN_dec(emb_inputs[idx] + table[t]) once, in double.
// Rows of different codewords never meet, so a codeword's result does not depend on the batch around it.
#include <string.h>

#include <new>
#include <vector>

#include "npd_xformer.hpp"

namespace npd {
namespace xfdec {

using namespace npd::xf;

struct Image {
    int emb_cross, table_cross;  // emb_cross.weight rows 1 .. N and the num = 5000 sinusoid table: [N][64] each
    int ln_cross;                // gamma[64], beta[64]
    int tokens;                  // [3][N][64]: LN_dec(emb_inputs[idx] + table[t])
    LayerOff layer[kMaxLayers];
    CrossOff cross[kMaxLayers];
    int lin;                     // Lin_Decoder weight[64], bias
};

struct Lds : Bufs {
    float Mem[kRows * kLS];
    float feed[4 * 64];  // feed[g][j]: the bit at position j that token j + 1 is built from
};

template <int N>
__global__ __launch_bounds__(kThreads, 1) void xfdec_decode_kernel(const float* __restrict__ img, Image im, int n_layers,
                                                                   const float* __restrict__ y, uint64_t info_mask,
                                                                   const float* __restrict__ forced,
                                                                   float* __restrict__ decoded,
                                                                   float* __restrict__ logits, int64_t B) {
    constexpr int G = kRows / N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Lds& s = *reinterpret_cast<Lds*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * G;

    // ---- the memory: all G N = 64 rows, then LN_cross
    for (int e = tid; e < kRows * (kE / 4); e += kThreads) {
        const int row = e >> 4, c4 = (e & 15) * 4;
        const int g = row / N, j = row - g * N;
        int64_t b = b0 + g;
        b = b < B ? b : B - 1;
        f4 v = y[b * N + j] * *reinterpret_cast<const f4*>(img + im.emb_cross + j * kE + c4);
        v += *reinterpret_cast<const f4*>(img + im.table_cross + j * kE + c4);
        *reinterpret_cast<f4*>(&s.Mem[row * kLS + c4]) = v;
    }
    // frozen positions decide +1 (or take the forced bit); their outputs are written here, once
    for (int e = tid; e < G * N; e += kThreads) {
        const int gg = e / N, j = e % N;
        const int64_t bb = b0 + gg;
        const bool frozen = !((info_mask >> j) & 1);
        const int64_t bc = bb < B ? bb : B - 1;
        s.feed[gg * 64 + j] = forced != nullptr ? forced[bc * N + j] : 1.0f;
        if (frozen && bb < B) {
            if (decoded != nullptr) decoded[bb * N + j] = 1.0f;
            if (logits != nullptr) logits[bb * N + j] = 0.0f;
        }
    }
    __syncthreads();
    ln_rows(s.Mem, nullptr, kRows, img + im.ln_cross, wave, lane);
    __syncthreads();

    for (int i = 0; i < N; ++i) {
        if (!((info_mask >> i) & 1)) continue;  // nothing runs at a frozen position
        const int n = i + 1, M = G * n;
        // ---- X = the tabulated tokens: index 2 at t = 0, then 1 where the bit before is +1, else 0
        for (int e = tid; e < M * (kE / 4); e += kThreads) {
            const int row = e >> 4, c4 = (e & 15) * 4;
            const int g = row / n, t = row - g * n;
            const int idx = t == 0 ? 2 : (s.feed[g * 64 + t - 1] == 1.0f ? 1 : 0);
            *reinterpret_cast<f4*>(&s.X[row * kLS + c4]) =
                *reinterpret_cast<const f4*>(img + im.tokens + (idx * N + t) * kE + c4);
        }
        __syncthreads();
        for (int layer = 0; layer < n_layers; ++layer) {
            const LayerOff lo = im.layer[layer];
            const CrossOff co = im.cross[layer];
            const bool last = layer == n_layers - 1;
            // ---- self-attention over the prefix
            stage_qkv(s, s.X, M, s.X, M, img + lo.qkv, wave, lane);
            __syncthreads();
            int Mq = M;
            if (last) {
                // only token i of each codeword goes on: attention into compact rows of T, X gathered the same way
                stage_attention(s, s.T, n, n, G, true, tid);
                float xv = 0.0f;
                if (tid < G * kE) xv = s.X[((tid >> 6) * n + n - 1) * kLS + (tid & 63)];
                __syncthreads();
                if (tid < G * kE) s.X[(tid >> 6) * kLS + (tid & 63)] = xv;
                Mq = G;
            } else {
                stage_attention(s, s.Q, n, n, M, false, tid);
            }
            __syncthreads();
            stage_fc(s, last ? s.T : s.Q, Mq, img + lo.fc, wave, lane);
            __syncthreads();
            stage_ln(s, Mq, false, img + lo.ln1, wave, lane);
            __syncthreads();
            // ---- cross-attention: queries from the Mq token rows, keys and values from the N memory rows of the
            // query's codeword (compact row g is codeword g: n = 1)
            stage_qkv(s, s.X, Mq, s.Mem, kRows, img + co.qkv, wave, lane);
            __syncthreads();
            stage_attention(s, s.Q, last ? 1 : n, N, Mq, false, tid);
            __syncthreads();
            stage_fc(s, s.Q, Mq, img + co.fc, wave, lane);
            __syncthreads();
            stage_ln(s, Mq, false, img + co.ln, wave, lane);
            __syncthreads();
            stage_ffn(s, Mq, img, lo, wave, lane);
        }
        // ---- logit = Lin_Decoder(X_out[token i]) (compact row g after the last layer); one wave per codeword
        if (wave < G) {
            const int g = wave;
            const float v = wave_sum(s.X[g * kLS + lane] * img[im.lin + lane]) + img[im.lin + kE];
            const float bit = sgnf(v);
            const int64_t b = b0 + g;
            if (lane == 0) {
                if (forced == nullptr) s.feed[g * 64 + i] = bit;
                if (b < B) {
                    if (decoded != nullptr) decoded[b * N + i] = bit;
                    if (logits != nullptr) logits[b * N + i] = v;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace xfdec
}  // namespace npd

using namespace npd;
using namespace npd::xfdec;

struct npd_xfdec {
    int N, L, device;
    float* img;
    Image im;
};

static int64_t xfdec_weight_count(int N, int L) {
    return (int64_t)(N + 1) * kE + (int64_t)N * kE + 2 * kE + 4 * kE + (int64_t)N * kE + 2 * kE +
           (int64_t)L * (kLayerWeights + kCrossWeights) + kE + 1;
}

extern "C" int npd_xfdec_create(int N, int embed_dim, int n_head, int n_layers, const float* weights, int64_t n_weights,
                                npd_xfdec** out) {
    NPD_ARG(out != nullptr, "npd_xfdec_create: out is NULL");
    *out = nullptr;
    NPD_ARG(weights != nullptr, "npd_xfdec_create: weights is NULL");
    NPD_ARG(embed_dim == kE, "npd_xfdec_create: embed_dim must be 64");
    NPD_ARG(n_head == kH, "npd_xfdec_create: n_head must be 8");
    NPD_ARG(N == 16 || N == 32 || N == 64, "npd_xfdec_create: N must be 16, 32 or 64");
    NPD_ARG(n_layers >= 1 && n_layers <= kMaxLayers, "npd_xfdec_create: n_layers must be 1 .. 8");
    NPD_ARG(n_weights == xfdec_weight_count(N, n_layers), "npd_xfdec_create: weight count does not match (N, n_layers)");
    npd_xfdec* h = new (std::nothrow) npd_xfdec;
    if (!h) return fail(NPD_ENOMEM, "npd_xfdec_create: out of memory");
    memset(h, 0, sizeof(*h));
    h->N = N;
    h->L = n_layers;
    std::vector<float> img;
    const float* p = weights;
    Image& im = h->im;
    im.emb_cross = push(img, p + kE, (int64_t)N * kE); p += (int64_t)(N + 1) * kE;  // row 0 is the padding row
    im.table_cross = push(img, p, (int64_t)N * kE); p += (int64_t)N * kE;
    im.ln_cross = push(img, p, 2 * kE); p += 2 * kE;
    {
        // tokens[idx][t] = LN_dec(emb_inputs[idx] + table[t]), idx = 0, 1, 2 (3 is the padding index, never fed)
        const float *emb = p, *table = p + 4 * kE, *gam = table + (int64_t)N * kE, *bet = gam + kE;
        im.tokens = (int)img.size();
        for (int idx = 0; idx < 3; ++idx)
            for (int t = 0; t < N; ++t) {
                double v[kE], mean = 0.0, var = 0.0;
                for (int c = 0; c < kE; ++c) {
                    v[c] = (double)emb[idx * kE + c] + (double)table[t * kE + c];
                    mean += v[c];
                }
                mean /= kE;
                for (int c = 0; c < kE; ++c) var += (v[c] - mean) * (v[c] - mean);
                var /= kE;
                for (int c = 0; c < kE; ++c)
                    img.push_back((float)((v[c] - mean) / sqrt(var + 1e-6) * (double)gam[c] + (double)bet[c]));
            }
        p = bet + kE;
    }
    for (int l = 0; l < n_layers; ++l) {
        LayerOff& lo = im.layer[l];
        CrossOff& co = im.cross[l];
        p = push_attention(img, p, &lo.qkv, &lo.fc, &lo.ln1);
        p = push_attention(img, p, &co.qkv, &co.fc, &co.ln);
        p = push_ffn(img, p, lo);
    }
    im.lin = push(img, p, kE + 1); p += kE + 1;
    const hipError_t e = upload(img, &h->device, &h->img);
    if (e != hipSuccess) {
        delete h;
        return hip_fail(e, "npd_xfdec_create");
    }
    *out = h;
    return NPD_OK;
}

extern "C" int npd_xfdec_destroy(npd_xfdec* h) {
    NPD_ARG(h != nullptr, "npd_xfdec_destroy: handle is NULL");
    if (h->img) (void)hipFree(h->img);
    delete h;
    return NPD_OK;
}

// the whole decode lives in LDS and registers: no scratch memory is taken from the caller
extern "C" int64_t npd_xfdec_workspace_bytes(const npd_xfdec* h, int64_t B) {
    NPD_ARG(h != nullptr, "npd_xfdec_workspace_bytes: handle is NULL");
    NPD_ARG(B >= 0, "npd_xfdec_workspace_bytes: B < 0");
    return 0;
}

template <int N>
static int xfdec_launch(const npd_xfdec* h, const float* y, uint64_t mask, const float* forced, float* decoded,
                        float* logits, int64_t B, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        NPD_HIP(hipFuncSetAttribute((const void*)xfdec_decode_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sizeof(Lds)));
        attr = true;
    }
    constexpr int G = kRows / N;
    const int64_t blocks = (B + G - 1) / G;
    hipLaunchKernelGGL(xfdec_decode_kernel<N>, dim3((unsigned)blocks), dim3(kThreads), sizeof(Lds), s, h->img, h->im, h->L,
                       y, mask, forced, decoded, logits, B);
    return launch_check("xfdec_decode_kernel");
}

extern "C" int npd_xfdec_decode(const npd_xfdec* h, const float* y, const uint8_t* is_info, const float* forced,
                                float* decoded, float* logits, int64_t B, void* stream) {
    NPD_ARG(h != nullptr, "npd_xfdec_decode: handle is NULL");
    NPD_ARG(B >= 0, "npd_xfdec_decode: B < 0");
    NPD_ARG(is_info != nullptr, "npd_xfdec_decode: is_info is NULL");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr, "npd_xfdec_decode: y is NULL");
    NPD_ARG(decoded != nullptr, "npd_xfdec_decode: decoded is NULL");
    NPD_ARG(B <= 0x7fffffff, "npd_xfdec_decode: B too large for one launch");
    uint64_t mask = 0;
    for (int j = 0; j < h->N; ++j)
        if (is_info[j]) mask |= (uint64_t)1 << j;
    hipStream_t s = (hipStream_t)stream;
    switch (h->N) {
        case 16: return xfdec_launch<16>(h, y, mask, forced, decoded, logits, B, s);
        case 32: return xfdec_launch<32>(h, y, mask, forced, decoded, logits, B, s);
        default: return xfdec_launch<64>(h, y, mask, forced, decoded, logits, B, s);
    }
}

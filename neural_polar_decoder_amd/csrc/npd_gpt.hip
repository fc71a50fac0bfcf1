// npd_gpt.hip -- XFormerEndToEndGPT.decode (models.py:340-423) in one launch, fp32 on v_mfma_f32_32x32x2_f32.
//
// What decode computes.  At every information position i the reference runs the whole layer stack again on the
// sequence built so far, with the single mask row i: every token 0 .. i attends to every key <= i and only token i's
// output reaches Lin_Decoder.  Tokens past i cannot reach token i (their keys are masked to an exact 0 after softmax),
// so this kernel works on the prefix of n = i + 1 tokens only.  It is not a KV-cached causal decode: token j's
// activations at step i differ from those at step i - 1, because token j now also sees keys j + 1 .. i.
//
// Mapping.  One workgroup (512 threads, 8 waves) owns G = 64 / N codewords for the whole decode; all of them are at
// the same step, so their prefixes are stacked into M = G n <= 64 activation rows (row g n + t = codeword g, token t).
// The LDS buffers, the weight packing and the stages of a layer are in npd_xformer.hpp, shared with the encoder and
// decoder models' kernels (1.2 MB of weights for 6 layers: L2 resident).
//   * the last layer needs K and V for the whole prefix but attention, fc, the FFN and both LayerNorms for token i only:
//     those rows are gathered into G compact rows first.
// Rows of different codewords never meet, so a codeword's result does not depend on the batch around it.
#include <string.h>

#include <new>
#include <vector>

#include "npd_xformer.hpp"

namespace npd {
namespace gpt {

using namespace npd::xf;

struct Image {
    int s0, sb0, s1, sb1, s2, sb2;  // start MLP: transposed weights [k][64] and biases
    int pos_emb, pos_table;          // [N][64] each
    LayerOff layer[kMaxLayers];
    int lin;                         // Lin_Decoder weight[64], bias
};

struct Lds : Bufs {
    float start[4 * kE];   // the start token of each codeword
    float hid[2][4 * kE];  // start MLP activations
    float feed[4 * 64];    // feed[g][j]: the bit at position j that token j + 1 is built from
};

template <int N>
__global__ __launch_bounds__(kThreads, 1) void gpt_decode_kernel(const float* __restrict__ img, Image im, int n_layers,
                                                                 const float* __restrict__ y, uint64_t info_mask,
                                                                 const float* __restrict__ forced,
                                                                 float* __restrict__ decoded, float* __restrict__ logits,
                                                                 int64_t B) {
    constexpr int G = kRows / N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Lds& s = *reinterpret_cast<Lds*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * G;

    // ---- start token: Linear(N, E) -> GELU -> Linear(E, E) -> GELU -> Linear(E, E); thread (g, c), tid < G E <= 256
    {
        const int g = tid >> 6, c = tid & 63;
        const bool on = tid < G * kE;
        int64_t b = b0 + g;
        b = b < B ? b : B - 1;
        if (on) {
            float acc = img[im.sb0 + c];
            for (int k = 0; k < N; ++k) acc = fmaf(y[b * N + k], img[im.s0 + k * kE + c], acc);
            s.hid[0][g * kE + c] = gelu(acc);
        }
        __syncthreads();
        if (on) {
            float acc = img[im.sb1 + c];
            for (int k = 0; k < kE; ++k) acc = fmaf(s.hid[0][g * kE + k], img[im.s1 + k * kE + c], acc);
            s.hid[1][g * kE + c] = gelu(acc);
        }
        __syncthreads();
        if (on) {
            float acc = img[im.sb2 + c];
            for (int k = 0; k < kE; ++k) acc = fmaf(s.hid[1][g * kE + k], img[im.s2 + k * kE + c], acc);
            s.start[g * kE + c] = acc;
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
    }

    for (int i = 0; i < N; ++i) {
        if (!((info_mask >> i) & 1)) continue;  // nothing runs at a frozen position
        const int n = i + 1, M = G * n;
        // ---- X = tokens + pos_table: token 0 = start, token t = feed[t - 1] pos_emb[t]
        for (int e = tid; e < M * (kE / 4); e += kThreads) {
            const int row = e >> 4, c4 = (e & 15) * 4;
            const int g = row / n, t = row - g * n;
            f4 v;
            if (t == 0) {
                v = *reinterpret_cast<const f4*>(&s.start[g * kE + c4]);
            } else {
                v = s.feed[g * 64 + t - 1] * *reinterpret_cast<const f4*>(img + im.pos_emb + t * kE + c4);
            }
            v += *reinterpret_cast<const f4*>(img + im.pos_table + t * kE + c4);
            *reinterpret_cast<f4*>(&s.X[row * kLS + c4]) = v;
        }
        __syncthreads();
        for (int layer = 0; layer < n_layers; ++layer) {
            const LayerOff lo = im.layer[layer];
            const bool last = layer == n_layers - 1;
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

}  // namespace gpt
}  // namespace npd

using namespace npd;
using namespace npd::gpt;

struct npd_gpt {
    int N, L, device;
    float* img;
    Image im;
};

static int64_t gpt_weight_count(int N, int L) {
    return (int64_t)N * kE + kE + 2 * (kE * kE + kE) + 2 * (int64_t)N * kE +
           (int64_t)L * kLayerWeights + kE + 1;
}

extern "C" int npd_gpt_create(int N, int embed_dim, int n_head, int n_layers, const float* weights, int64_t n_weights,
                              npd_gpt** out) {
    NPD_ARG(out != nullptr, "npd_gpt_create: out is NULL");
    *out = nullptr;
    NPD_ARG(weights != nullptr, "npd_gpt_create: weights is NULL");
    NPD_ARG(embed_dim == kE, "npd_gpt_create: embed_dim must be 64");
    NPD_ARG(n_head == kH, "npd_gpt_create: n_head must be 8");
    NPD_ARG(N == 16 || N == 32 || N == 64, "npd_gpt_create: N must be 16, 32 or 64");
    NPD_ARG(n_layers >= 1 && n_layers <= kMaxLayers, "npd_gpt_create: n_layers must be 1 .. 8");
    NPD_ARG(n_weights == gpt_weight_count(N, n_layers), "npd_gpt_create: weight count does not match (N, n_layers)");
    npd_gpt* h = new (std::nothrow) npd_gpt;
    if (!h) return fail(NPD_ENOMEM, "npd_gpt_create: out of memory");
    memset(h, 0, sizeof(*h));
    h->N = N;
    h->L = n_layers;
    std::vector<float> img;
    const float* p = weights;
    Image& im = h->im;
    im.s0 = push_t(img, p, kE, N); p += (int64_t)kE * N;
    im.sb0 = push(img, p, kE); p += kE;
    im.s1 = push_t(img, p, kE, kE); p += kE * kE;
    im.sb1 = push(img, p, kE); p += kE;
    im.s2 = push_t(img, p, kE, kE); p += kE * kE;
    im.sb2 = push(img, p, kE); p += kE;
    im.pos_emb = push(img, p, (int64_t)N * kE); p += (int64_t)N * kE;
    im.pos_table = push(img, p, (int64_t)N * kE); p += (int64_t)N * kE;
    for (int l = 0; l < n_layers; ++l) {
        LayerOff& lo = im.layer[l];
        p = push_attention(img, p, &lo.qkv, &lo.fc, &lo.ln1);
        p = push_ffn(img, p, lo);
    }
    im.lin = push(img, p, kE + 1); p += kE + 1;
    const hipError_t e = upload(img, &h->device, &h->img);
    if (e != hipSuccess) {
        delete h;
        return hip_fail(e, "npd_gpt_create");
    }
    *out = h;
    return NPD_OK;
}

extern "C" int npd_gpt_destroy(npd_gpt* h) {
    NPD_ARG(h != nullptr, "npd_gpt_destroy: handle is NULL");
    if (h->img) (void)hipFree(h->img);
    delete h;
    return NPD_OK;
}

// the whole decode lives in LDS and registers: no scratch memory is taken from the caller
extern "C" int64_t npd_gpt_workspace_bytes(const npd_gpt* h, int64_t B) {
    NPD_ARG(h != nullptr, "npd_gpt_workspace_bytes: handle is NULL");
    NPD_ARG(B >= 0, "npd_gpt_workspace_bytes: B < 0");
    return 0;
}

template <int N>
static int gpt_launch(const npd_gpt* h, const float* y, uint64_t mask, const float* forced, float* decoded, float* logits,
                      int64_t B, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        NPD_HIP(hipFuncSetAttribute((const void*)gpt_decode_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sizeof(Lds)));
        attr = true;
    }
    constexpr int G = kRows / N;
    const int64_t blocks = (B + G - 1) / G;
    hipLaunchKernelGGL(gpt_decode_kernel<N>, dim3((unsigned)blocks), dim3(kThreads), sizeof(Lds), s, h->img, h->im, h->L, y,
                       mask, forced, decoded, logits, B);
    return launch_check("gpt_decode_kernel");
}

extern "C" int npd_gpt_decode(const npd_gpt* h, const float* y, const uint8_t* is_info, const float* forced,
                              float* decoded, float* logits, int64_t B, void* stream) {
    NPD_ARG(h != nullptr, "npd_gpt_decode: handle is NULL");
    NPD_ARG(B >= 0, "npd_gpt_decode: B < 0");
    NPD_ARG(is_info != nullptr, "npd_gpt_decode: is_info is NULL");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr, "npd_gpt_decode: y is NULL");
    NPD_ARG(decoded != nullptr, "npd_gpt_decode: decoded is NULL");
    NPD_ARG((B + 3) / 4 <= 0x7fffffff, "npd_gpt_decode: B too large for one launch");
    uint64_t mask = 0;
    for (int j = 0; j < h->N; ++j)
        if (is_info[j]) mask |= (uint64_t)1 << j;
    hipStream_t s = (hipStream_t)stream;
    switch (h->N) {
        case 16: return gpt_launch<16>(h, y, mask, forced, decoded, logits, B, s);
        case 32: return gpt_launch<32>(h, y, mask, forced, decoded, logits, B, s);
        default: return gpt_launch<64>(h, y, mask, forced, decoded, logits, B, s);
    }
}

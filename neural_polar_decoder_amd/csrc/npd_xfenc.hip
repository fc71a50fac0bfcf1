// npd_xfenc.hip -- XFormerEndToEndEncoder.forward / decode (models.py:662-686, --model encoder) in one launch, fp32 on
// v_mfma_f32_32x32x2_f32.
//
// One pass, no autoregression: X[j] = LN_enc(y_j pos_emb[j + 1] + table_10000[j]), then n_layers post-LN encoder layers
// with full attention over the N tokens of a word, and logit[j] = Lin_Decoder(X[j]) for every j.  The bit is the sign
// of the logit at every position, frozen ones included.
//
// Mapping: npd_xformer.hpp's at n = N, so the G = 64 / N codewords of a workgroup fill all M = 64 rows (row g N + j);
// every token's output is used, so no layer is cut short.  Rows of different codewords never meet, so a codeword's
// result does not depend on the batch around it.
#include <string.h>

#include <new>
#include <vector>

#include "npd_xformer.hpp"

namespace npd {
namespace xfenc {

using namespace npd::xf;

struct Image {
    int pos_emb, table;  // pos_emb.weight rows 1 .. N and the sinusoid table: [N][64] each
    int ln;              // Encoder.layer_norm: gamma[64], beta[64]
    LayerOff layer[kMaxLayers];
    int lin;             // Lin_Decoder weight[64], bias
};

template <int N>
__global__ __launch_bounds__(kThreads, 1) void xfenc_forward_kernel(const float* __restrict__ img, Image im, int n_layers,
                                                                    const float* __restrict__ y, float* __restrict__ bits,
                                                                    float* __restrict__ logits, int64_t B) {
    constexpr int G = kRows / N;
    constexpr int M = kRows;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Bufs& s = *reinterpret_cast<Bufs*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * G;

    for (int e = tid; e < M * (kE / 4); e += kThreads) {
        const int row = e >> 4, c4 = (e & 15) * 4;
        const int g = row / N, j = row - g * N;
        int64_t b = b0 + g;
        b = b < B ? b : B - 1;
        f4 v = y[b * N + j] * *reinterpret_cast<const f4*>(img + im.pos_emb + j * kE + c4);
        v += *reinterpret_cast<const f4*>(img + im.table + j * kE + c4);
        *reinterpret_cast<f4*>(&s.X[row * kLS + c4]) = v;
    }
    __syncthreads();
    stage_ln(s, M, false, img + im.ln, wave, lane);
    __syncthreads();
    for (int layer = 0; layer < n_layers; ++layer) {
        const LayerOff lo = im.layer[layer];
        stage_qkv(s, s.X, M, s.X, M, img + lo.qkv, wave, lane);
        __syncthreads();
        stage_attention(s, s.Q, N, N, M, false, tid);
        __syncthreads();
        stage_fc(s, s.Q, M, img + lo.fc, wave, lane);
        __syncthreads();
        stage_ln(s, M, false, img + lo.ln1, wave, lane);
        __syncthreads();
        stage_ffn(s, M, img, lo, wave, lane);
    }
    // ---- logit = Lin_Decoder(X[row]) for every row; one wave per row
    const float w = img[im.lin + lane], bias = img[im.lin + kE];
    for (int row = wave; row < M; row += kWaves) {
        const float v = wave_sum(s.X[row * kLS + lane] * w) + bias;
        const int64_t b = b0 + row / N;
        if (lane == 0 && b < B) {
            const int64_t o = b * N + row % N;
            if (bits != nullptr) bits[o] = sgnf(v);
            if (logits != nullptr) logits[o] = v;
        }
    }
}

}  // namespace xfenc
}  // namespace npd

using namespace npd;
using namespace npd::xfenc;

struct npd_xfenc {
    int N, L, device;
    float* img;
    Image im;
};

static int64_t xfenc_weight_count(int N, int L) {
    return (int64_t)(N + 1) * kE + (int64_t)N * kE + 2 * kE + (int64_t)L * kLayerWeights + kE + 1;
}

extern "C" int npd_xfenc_create(int N, int embed_dim, int n_head, int n_layers, const float* weights, int64_t n_weights,
                                npd_xfenc** out) {
    NPD_ARG(out != nullptr, "npd_xfenc_create: out is NULL");
    *out = nullptr;
    NPD_ARG(weights != nullptr, "npd_xfenc_create: weights is NULL");
    NPD_ARG(embed_dim == kE, "npd_xfenc_create: embed_dim must be 64");
    NPD_ARG(n_head == kH, "npd_xfenc_create: n_head must be 8");
    NPD_ARG(N == 16 || N == 32 || N == 64, "npd_xfenc_create: N must be 16, 32 or 64");
    NPD_ARG(n_layers >= 1 && n_layers <= kMaxLayers, "npd_xfenc_create: n_layers must be 1 .. 8");
    NPD_ARG(n_weights == xfenc_weight_count(N, n_layers), "npd_xfenc_create: weight count does not match (N, n_layers)");
    npd_xfenc* h = new (std::nothrow) npd_xfenc;
    if (!h) return fail(NPD_ENOMEM, "npd_xfenc_create: out of memory");
    memset(h, 0, sizeof(*h));
    h->N = N;
    h->L = n_layers;
    std::vector<float> img;
    const float* p = weights;
    Image& im = h->im;
    im.pos_emb = push(img, p + kE, (int64_t)N * kE); p += (int64_t)(N + 1) * kE;  // row 0 is the padding row
    im.table = push(img, p, (int64_t)N * kE); p += (int64_t)N * kE;
    im.ln = push(img, p, 2 * kE); p += 2 * kE;
    for (int l = 0; l < n_layers; ++l) {
        LayerOff& lo = im.layer[l];
        p = push_attention(img, p, &lo.qkv, &lo.fc, &lo.ln1);
        p = push_ffn(img, p, lo);
    }
    im.lin = push(img, p, kE + 1); p += kE + 1;
    const hipError_t e = upload(img, &h->device, &h->img);
    if (e != hipSuccess) {
        delete h;
        return hip_fail(e, "npd_xfenc_create");
    }
    *out = h;
    return NPD_OK;
}

extern "C" int npd_xfenc_destroy(npd_xfenc* h) {
    NPD_ARG(h != nullptr, "npd_xfenc_destroy: handle is NULL");
    if (h->img) (void)hipFree(h->img);
    delete h;
    return NPD_OK;
}

// the whole forward lives in LDS and registers: no scratch memory is taken from the caller
extern "C" int64_t npd_xfenc_workspace_bytes(const npd_xfenc* h, int64_t B) {
    NPD_ARG(h != nullptr, "npd_xfenc_workspace_bytes: handle is NULL");
    NPD_ARG(B >= 0, "npd_xfenc_workspace_bytes: B < 0");
    return 0;
}

template <int N>
static int xfenc_launch(const npd_xfenc* h, const float* y, float* bits, float* logits, int64_t B, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        NPD_HIP(hipFuncSetAttribute((const void*)xfenc_forward_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sizeof(Bufs)));
        attr = true;
    }
    constexpr int G = kRows / N;
    const int64_t blocks = (B + G - 1) / G;
    hipLaunchKernelGGL(xfenc_forward_kernel<N>, dim3((unsigned)blocks), dim3(kThreads), sizeof(Bufs), s, h->img, h->im,
                       h->L, y, bits, logits, B);
    return launch_check("xfenc_forward_kernel");
}

extern "C" int npd_xfenc_forward(const npd_xfenc* h, const float* y, float* bits, float* logits, int64_t B, void* stream) {
    NPD_ARG(h != nullptr, "npd_xfenc_forward: handle is NULL");
    NPD_ARG(B >= 0, "npd_xfenc_forward: B < 0");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr, "npd_xfenc_forward: y is NULL");
    NPD_ARG(bits != nullptr, "npd_xfenc_forward: bits is NULL");
    NPD_ARG(B <= 0x7fffffff, "npd_xfenc_forward: B too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    switch (h->N) {
        case 16: return xfenc_launch<16>(h, y, bits, logits, B, s);
        case 32: return xfenc_launch<32>(h, y, bits, logits, B, s);
        default: return xfenc_launch<64>(h, y, bits, logits, B, s);
    }
}

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
// Six (64 rows x 64 features, stride 68) fp32 buffers live in LDS: X (the residual stream), Q, K, V, T and P.
//   * every Linear is rows x W^T on MFMA: a wave takes a (32-row, 32-column) tile, reads A = activations from LDS (one
//     ds_read_b128 = four k-steps) and B = weights from global memory, packed on the host in B-operand order so that the
//     four k-steps are one coalesced 16-B load per lane (1.2 MB for 6 layers: L2 resident).  K-step s of a 64-wide K
//     block pairs k = s (lanes 0 .. 31) with k = s + 32 (lanes 32 .. 63).
//   * w_1's 256 hidden features are written over Q, K, V, T (64 each); w_2's K = 256 is split in two halves so that a
//     short prefix (one row tile) still has four tile jobs; the halves meet in the LayerNorm (X + P), in a fixed order.
//   * attention (d = 8 per head) runs on the VALU, one thread per (row, head): scores in chunks of 8 keys with a running
//     maximum, exp, and the weighted sum of V; lanes h = 0 .. 7 of a row read one whole K / V row between them.
//   * the last layer needs K and V for the whole prefix but attention, fc, the FFN and both LayerNorms for token i only:
//     those rows are gathered into G compact rows first.
// Rows of different codewords never meet, so a codeword's result does not depend on the batch around it.
#include <math.h>
#include <string.h>

#include <new>
#include <vector>

#include "npd_common.hpp"

namespace npd {
namespace gpt {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kE = 64;          // embed_dim
constexpr int kH = 8;           // heads
constexpr int kD = 8;           // head width
constexpr int kFF = 256;        // FFN hidden width
constexpr int kRows = 64;       // activation rows per workgroup (G N)
constexpr int kLS = kE + 4;     // LDS row stride: 16-B aligned, 32 rows x ds_read_b128 at one k offset are conflict-free
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 8 * 64 * 4;  // floats of one packed (32 columns x 64 k) weight tile
constexpr int kMaxLayers = 8;

// offsets (floats) into the device weight image
struct LayerOff {
    int qkv;   // 6 tiles: q (2), k (2), v (2)
    int fc;    // 2 tiles
    int ln1;   // gamma[64], beta[64]
    int w1;    // 8 tiles
    int b1;    // 256
    int w2;    // 2 column tiles x 4 K blocks
    int b2;    // 64
    int ln2;   // gamma[64], beta[64]
};

struct Image {
    int s0, sb0, s1, sb1, s2, sb2;  // start MLP: transposed weights [k][64] and biases
    int pos_emb, pos_table;          // [N][64] each
    LayerOff layer[kMaxLayers];
    int lin;                         // Lin_Decoder weight[64], bias
};

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__device__ __forceinline__ f16v mfma(float a, float b, const f16v& c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// acc += A[row0 .. row0 + 31][64 k] x tile^T: A rows in LDS (rows past M - 1 read row M - 1; the caller drops them)
__device__ __forceinline__ f16v tile_k64(f16v acc, const float* a_lds, int row0, int M, const float* __restrict__ tile,
                                         int lane) {
    int row = row0 + (lane & 31);
    row = row < M ? row : M - 1;
    const f4* a = reinterpret_cast<const f4*>(a_lds + row * kLS + 32 * (lane >> 5));
    const f4* b = reinterpret_cast<const f4*>(tile) + lane;
    f4 bv[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) bv[g] = b[g * 64];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const f4 av = a[g];
        acc = mfma(av.x, bv[g].x, acc);
        acc = mfma(av.y, bv[g].y, acc);
        acc = mfma(av.z, bv[g].z, acc);
        acc = mfma(av.w, bv[g].w, acc);
    }
    return acc;
}

__device__ __forceinline__ f16v zero16() {
    return f16v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of the tile
#define NPD_GPT_EPILOGUE(row0, M, body)                                          \
    _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                          \
        const int row = (row0) + (r_ & 3) + 8 * (r_ >> 2) + 4 * (lane >> 5);     \
        const float a = acc[r_];                                                 \
        if (row < (M)) { body; }                                                 \
    }

struct Lds {
    float X[kRows * kLS], Q[kRows * kLS], K[kRows * kLS], V[kRows * kLS], T[kRows * kLS], P[kRows * kLS];
    float start[4 * kE];   // the start token of each codeword
    float hid[2][4 * kE];  // start MLP activations
    float feed[4 * 64];    // feed[g][j]: the bit at position j that token j + 1 is built from
};

// q, k, v = X W^T (no bias); q is divided by sqrt(d) as the reference does before the product with k
__device__ __forceinline__ void stage_qkv(Lds& s, int M, const float* __restrict__ w, int wave, int lane) {
    const int T = (M + 31) >> 5;
    for (int job = wave; job < 6 * T; job += kWaves) {
        const int ct = job % 6, rt = job / 6;
        const f16v acc = tile_k64(zero16(), s.X, rt * 32, M, w + ct * kTile, lane);
        float* dst = ct < 2 ? s.Q : (ct < 4 ? s.K : s.V);
        const int col = (ct & 1) * 32 + (lane & 31);
        if (ct < 2) {
            NPD_GPT_EPILOGUE(rt * 32, M, dst[row * kLS + col] = a / 2.8284271247461903f)
        } else {
            NPD_GPT_EPILOGUE(rt * 32, M, dst[row * kLS + col] = a)
        }
    }
}

// One thread per (query, head).  Query qi is row qi (last == false) or the last token of codeword qi (last == true, the
// result goes to compact row qi); the keys are the n rows of the query's codeword.  out may be the Q buffer itself when
// last == false: a thread reads its own 8 q values before it writes the same 8 places.
__device__ __forceinline__ void stage_attention(const Lds& s, float* out, int n, int nq, bool last, int tid) {
    for (int item = tid; item < nq * kH; item += kThreads) {
        const int h = item & (kH - 1), qi = item >> 3;
        const int g = last ? qi : qi / n;
        const int qrow = last ? g * n + n - 1 : qi;
        const int k0 = g * n;
        const f4 q0 = *reinterpret_cast<const f4*>(s.Q + qrow * kLS + h * kD);
        const f4 q1 = *reinterpret_cast<const f4*>(s.Q + qrow * kLS + h * kD + 4);
        float m = -INFINITY, l = 0.0f;
        f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < n; j0 += 8) {
            float sc[8];
            float cm = -INFINITY;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u < n ? j0 + u : n - 1;
                const f4 ka = *reinterpret_cast<const f4*>(s.K + (k0 + j) * kLS + h * kD);
                const f4 kb = *reinterpret_cast<const f4*>(s.K + (k0 + j) * kLS + h * kD + 4);
                float d = q0.x * ka.x;
                d = fmaf(q0.y, ka.y, d);
                d = fmaf(q0.z, ka.z, d);
                d = fmaf(q0.w, ka.w, d);
                d = fmaf(q1.x, kb.x, d);
                d = fmaf(q1.y, kb.y, d);
                d = fmaf(q1.z, kb.z, d);
                d = fmaf(q1.w, kb.w, d);
                sc[u] = j0 + u < n ? d : -INFINITY;
                cm = fmaxf(cm, sc[u]);
            }
            const float mn = fmaxf(m, cm);
            const float scale = expf(m - mn);  // first chunk: exp(-inf) = 0
            l *= scale;
            o0 *= scale;
            o1 *= scale;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u < n ? j0 + u : n - 1;
                const float p = expf(sc[u] - mn);  // masked tail: exp(-inf) = 0
                const f4 va = *reinterpret_cast<const f4*>(s.V + (k0 + j) * kLS + h * kD);
                const f4 vb = *reinterpret_cast<const f4*>(s.V + (k0 + j) * kLS + h * kD + 4);
                l += p;
                o0 += p * va;
                o1 += p * vb;
            }
            m = mn;
        }
        const float inv = 1.0f / l;
        const int orow = last ? qi : qrow;
        *reinterpret_cast<f4*>(out + orow * kLS + h * kD) = o0 * inv;
        *reinterpret_cast<f4*>(out + orow * kLS + h * kD + 4) = o1 * inv;
    }
}

// X += A fc^T (in place: each element of X is read and written by one lane only)
__device__ __forceinline__ void stage_fc(Lds& s, const float* a_lds, int M, const float* __restrict__ w, int wave,
                                         int lane) {
    const int T = (M + 31) >> 5;
    for (int job = wave; job < 2 * T; job += kWaves) {
        const int ct = job & 1, rt = job >> 1;
        const f16v acc = tile_k64(zero16(), a_lds, rt * 32, M, w + ct * kTile, lane);
        const int col = ct * 32 + (lane & 31);
        NPD_GPT_EPILOGUE(rt * 32, M, s.X[row * kLS + col] += a)
    }
}

// X = LayerNorm(X (+ P)) over the 64 features, eps 1e-6, biased variance: one wave per row
__device__ __forceinline__ void stage_ln(Lds& s, int M, bool add_p, const float* __restrict__ gb, int wave, int lane) {
    const float gam = gb[lane], bet = gb[kE + lane];
    for (int row = wave; row < M; row += kWaves) {
        float v = s.X[row * kLS + lane];
        if (add_p) v += s.P[row * kLS + lane];
        const float mean = wave_sum(v) * (1.0f / kE);
        const float d = v - mean;
        const float var = wave_sum(d * d) * (1.0f / kE);
        s.X[row * kLS + lane] = d / sqrtf(var + 1e-6f) * gam + bet;
    }
}

// hidden = GELU(X w_1^T + b_1): 256 features over the Q, K, V, T buffers
__device__ __forceinline__ void stage_w1(Lds& s, int M, const float* __restrict__ w, const float* __restrict__ b1,
                                         int wave, int lane) {
    const int T = (M + 31) >> 5;
    for (int job = wave; job < 8 * T; job += kWaves) {
        const int ct = job & 7, rt = job >> 3;
        const f16v acc = tile_k64(zero16(), s.X, rt * 32, M, w + ct * kTile, lane);
        float* dst = (ct >> 1) == 0 ? s.Q : ((ct >> 1) == 1 ? s.K : ((ct >> 1) == 2 ? s.V : s.T));
        const int col = (ct & 1) * 32 + (lane & 31);
        const float bias = b1[ct * 32 + (lane & 31)];
        NPD_GPT_EPILOGUE(rt * 32, M, dst[row * kLS + col] = gelu(a + bias))
    }
}

// X += hidden[:, 0:128] w_2[:, 0:128]^T + b_2 (in place) and P = hidden[:, 128:256] w_2[:, 128:256]^T
__device__ __forceinline__ void stage_w2(Lds& s, int M, const float* __restrict__ w, const float* __restrict__ b2,
                                         int wave, int lane) {
    const int T = (M + 31) >> 5;
    for (int job = wave; job < 4 * T; job += kWaves) {
        const int ct = job & 1, half = (job >> 1) & 1, rt = job >> 2;
        const float* wt = w + (ct * 4 + half * 2) * kTile;
        f16v acc = tile_k64(zero16(), half ? s.V : s.Q, rt * 32, M, wt, lane);
        acc = tile_k64(acc, half ? s.T : s.K, rt * 32, M, wt + kTile, lane);
        const int col = ct * 32 + (lane & 31);
        if (half == 0) {
            const float bias = b2[col];
            NPD_GPT_EPILOGUE(rt * 32, M, s.X[row * kLS + col] += a + bias)
        } else {
            NPD_GPT_EPILOGUE(rt * 32, M, s.P[row * kLS + col] = a)
        }
    }
}

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
            stage_qkv(s, M, img + lo.qkv, wave, lane);
            __syncthreads();
            int Mq = M;
            if (last) {
                // only token i of each codeword goes on: attention into compact rows of T, X gathered the same way
                stage_attention(s, s.T, n, G, true, tid);
                float xv = 0.0f;
                if (tid < G * kE) xv = s.X[((tid >> 6) * n + n - 1) * kLS + (tid & 63)];
                __syncthreads();
                if (tid < G * kE) s.X[(tid >> 6) * kLS + (tid & 63)] = xv;
                Mq = G;
            } else {
                stage_attention(s, s.Q, n, M, false, tid);
            }
            __syncthreads();
            stage_fc(s, last ? s.T : s.Q, Mq, img + lo.fc, wave, lane);
            __syncthreads();
            stage_ln(s, Mq, false, img + lo.ln1, wave, lane);
            __syncthreads();
            stage_w1(s, Mq, img + lo.w1, img + lo.b1, wave, lane);
            __syncthreads();
            stage_w2(s, Mq, img + lo.w2, img + lo.b2, wave, lane);
            __syncthreads();
            stage_ln(s, Mq, true, img + lo.ln2, wave, lane);
            __syncthreads();
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

// B-operand order of W (rows = output features, K columns), column tile ct: [K block c][g][lane][e] =
// W[32 ct + (lane & 31)][64 c + 4 g + e + 32 (lane >> 5)]
static void pack_tiles(std::vector<float>& img, const float* W, int nout, int K) {
    for (int ct = 0; ct < nout / 32; ++ct)
        for (int c = 0; c < K / 64; ++c)
            for (int g = 0; g < 8; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 4; ++e)
                        img.push_back(W[(int64_t)(32 * ct + (l & 31)) * K + 64 * c + 4 * g + e + 32 * (l >> 5)]);
}

static int push(std::vector<float>& img, const float* p, int64_t n) {
    const int off = (int)img.size();
    img.insert(img.end(), p, p + n);
    while (img.size() % 4) img.push_back(0.0f);
    return off;
}

static int push_t(std::vector<float>& img, const float* W, int nout, int K) {  // (nout, K) -> [k][nout]
    const int off = (int)img.size();
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < nout; ++c) img.push_back(W[(int64_t)c * K + k]);
    return off;
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
           (int64_t)L * (4 * kE * kE + 2 * kE + kFF * kE + kFF + kE * kFF + kE + 2 * kE) + kE + 1;
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
        lo.qkv = (int)img.size();
        for (int m = 0; m < 3; ++m) { pack_tiles(img, p, kE, kE); p += kE * kE; }
        lo.fc = (int)img.size();
        pack_tiles(img, p, kE, kE); p += kE * kE;
        lo.ln1 = push(img, p, 2 * kE); p += 2 * kE;
        lo.w1 = (int)img.size();
        pack_tiles(img, p, kFF, kE); p += kFF * kE;
        lo.b1 = push(img, p, kFF); p += kFF;
        lo.w2 = (int)img.size();
        pack_tiles(img, p, kE, kFF); p += kE * kFF;
        lo.b2 = push(img, p, kE); p += kE;
        lo.ln2 = push(img, p, 2 * kE); p += 2 * kE;
    }
    im.lin = push(img, p, kE + 1); p += kE + 1;
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc((void**)&h->img, img.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->img, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->img) (void)hipFree(h->img);
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

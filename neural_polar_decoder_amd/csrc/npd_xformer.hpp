// npd_xformer.hpp -- what the fused transformer kernels share (npd_gpt.hip, npd_xfdec.hip, npd_xfenc.hip): the 64-row
// LDS tile, the B-operand weight packing and the stages of one post-LN layer, fp32 on v_mfma_f32_32x32x2_f32.
//
// One workgroup (512 threads, 8 waves) owns G = 64 / N codewords; their tokens are stacked into M <= 64 activation rows.
// Six (64 rows x 64 features, stride 68) fp32 buffers live in LDS: X (the residual stream), Q, K, V, T and P.
//   * every Linear is rows x W^T on MFMA: a wave takes a (32-row, 32-column) tile, reads A = activations from LDS (one
//     ds_read_b128 = four k-steps) and B = weights from global memory, packed on the host in B-operand order so that the
//     four k-steps are one coalesced 16-B load per lane (L2 resident).  K-step s of a 64-wide K block pairs k = s
//     (lanes 0 .. 31) with k = s + 32 (lanes 32 .. 63).
//   * w_1's 256 hidden features are written over Q, K, V, T (64 each); w_2's K = 256 is split in two halves so that a
//     short prefix (one row tile) still has four tile jobs; the halves meet in the LayerNorm (X + P), in a fixed order.
//   * attention (d = 8 per head) runs on the VALU, one thread per (query row, head): scores in chunks of 8 keys with a
//     running maximum, exp, and the weighted sum of V; lanes h = 0 .. 7 of a row read one whole K / V row between them.
//     The keys of a query are the kn rows of its codeword in the K / V buffers, whatever the number of query rows is:
//     kn = n for self-attention over a prefix, kn = N for cross-attention over the memory.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "npd_common.hpp"

namespace npd {
namespace xf {

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
constexpr int kLayerWeights = 4 * kE * kE + 2 * kE + kFF * kE + kFF + kE * kFF + kE + 2 * kE;  // attention block + FFN
constexpr int kCrossWeights = 4 * kE * kE + 2 * kE;                                              // one more attention block

// offsets (floats) into the device weight image: one self-attention block and the FFN
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

// the cross-attention block of a decoder layer
struct CrossOff {
    int qkv, fc, ln;
};

// the six activation buffers every kernel carves first out of its dynamic LDS
struct Bufs {
    float X[kRows * kLS], Q[kRows * kLS], K[kRows * kLS], V[kRows * kLS], T[kRows * kLS], P[kRows * kLS];
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
#define NPD_XF_EPILOGUE(row0, M, body)                                           \
    _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                          \
        const int row = (row0) + (r_ & 3) + 8 * (r_ >> 2) + 4 * (lane >> 5);     \
        const float a = acc[r_];                                                 \
        if (row < (M)) { body; }                                                 \
    }

// q = xq Wq^T over Mq rows, k, v = xkv Wk^T, xkv Wv^T over Mkv rows (no bias); q is divided by sqrt(d) as the reference
// does before the product with k.  Self-attention: xq = xkv = X; cross-attention: xkv = the memory.
__device__ __forceinline__ void stage_qkv(Bufs& s, const float* xq, int Mq, const float* xkv, int Mkv,
                                          const float* __restrict__ w, int wave, int lane) {
    const int Tq = (Mq + 31) >> 5, Tkv = (Mkv + 31) >> 5;
    const int T = Tq > Tkv ? Tq : Tkv;
    for (int job = wave; job < 6 * T; job += kWaves) {
        const int ct = job % 6, rt = job / 6;
        if (rt >= (ct < 2 ? Tq : Tkv)) continue;  // wave-uniform
        if (ct < 2) {
            const f16v acc = tile_k64(zero16(), xq, rt * 32, Mq, w + ct * kTile, lane);
            const int col = (ct & 1) * 32 + (lane & 31);
            NPD_XF_EPILOGUE(rt * 32, Mq, s.Q[row * kLS + col] = a / 2.8284271247461903f)
        } else {
            const f16v acc = tile_k64(zero16(), xkv, rt * 32, Mkv, w + ct * kTile, lane);
            float* dst = ct < 4 ? s.K : s.V;
            const int col = (ct & 1) * 32 + (lane & 31);
            NPD_XF_EPILOGUE(rt * 32, Mkv, dst[row * kLS + col] = a)
        }
    }
}

// One thread per (query, head).  Query qi is row qi of Q (last == false; its codeword is qi / n) or the last of the n
// tokens of codeword qi (last == true, the result goes to compact row qi); the keys are the kn rows of the query's
// codeword in K / V, rows g kn .. g kn + kn - 1.  out may be the Q buffer itself when last == false: a thread reads
// its own 8 q values before it writes the same 8 places.
__device__ __forceinline__ void stage_attention(const Bufs& s, float* out, int n, int kn, int nq, bool last, int tid) {
    for (int item = tid; item < nq * kH; item += kThreads) {
        const int h = item & (kH - 1), qi = item >> 3;
        const int g = last ? qi : qi / n;
        const int qrow = last ? g * n + n - 1 : qi;
        const int k0 = g * kn;
        const f4 q0 = *reinterpret_cast<const f4*>(s.Q + qrow * kLS + h * kD);
        const f4 q1 = *reinterpret_cast<const f4*>(s.Q + qrow * kLS + h * kD + 4);
        float m = -INFINITY, l = 0.0f;
        f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < kn; j0 += 8) {
            float sc[8];
            float cm = -INFINITY;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u < kn ? j0 + u : kn - 1;
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
                sc[u] = j0 + u < kn ? d : -INFINITY;
                cm = fmaxf(cm, sc[u]);
            }
            const float mn = fmaxf(m, cm);
            const float scale = expf(m - mn);  // first chunk: exp(-inf) = 0
            l *= scale;
            o0 *= scale;
            o1 *= scale;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u < kn ? j0 + u : kn - 1;
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
__device__ __forceinline__ void stage_fc(Bufs& s, const float* a_lds, int M, const float* __restrict__ w, int wave,
                                         int lane) {
    const int T = (M + 31) >> 5;
    for (int job = wave; job < 2 * T; job += kWaves) {
        const int ct = job & 1, rt = job >> 1;
        const f16v acc = tile_k64(zero16(), a_lds, rt * 32, M, w + ct * kTile, lane);
        const int col = ct * 32 + (lane & 31);
        NPD_XF_EPILOGUE(rt * 32, M, s.X[row * kLS + col] += a)
    }
}

// x = LayerNorm(x (+ p)) over the 64 features of M rows, eps 1e-6, biased variance: one wave per row
__device__ __forceinline__ void ln_rows(float* x, const float* p, int M, const float* __restrict__ gb, int wave,
                                        int lane) {
    const float gam = gb[lane], bet = gb[kE + lane];
    for (int row = wave; row < M; row += kWaves) {
        float v = x[row * kLS + lane];
        if (p != nullptr) v += p[row * kLS + lane];
        const float mean = wave_sum(v) * (1.0f / kE);
        const float d = v - mean;
        const float var = wave_sum(d * d) * (1.0f / kE);
        x[row * kLS + lane] = d / sqrtf(var + 1e-6f) * gam + bet;
    }
}

// X = LayerNorm(X (+ P))
__device__ __forceinline__ void stage_ln(Bufs& s, int M, bool add_p, const float* __restrict__ gb, int wave, int lane) {
    ln_rows(s.X, add_p ? s.P : nullptr, M, gb, wave, lane);
}

// hidden = GELU(X w_1^T + b_1): 256 features over the Q, K, V, T buffers
__device__ __forceinline__ void stage_w1(Bufs& s, int M, const float* __restrict__ w, const float* __restrict__ b1,
                                         int wave, int lane) {
    const int T = (M + 31) >> 5;
    for (int job = wave; job < 8 * T; job += kWaves) {
        const int ct = job & 7, rt = job >> 3;
        const f16v acc = tile_k64(zero16(), s.X, rt * 32, M, w + ct * kTile, lane);
        float* dst = (ct >> 1) == 0 ? s.Q : ((ct >> 1) == 1 ? s.K : ((ct >> 1) == 2 ? s.V : s.T));
        const int col = (ct & 1) * 32 + (lane & 31);
        const float bias = b1[ct * 32 + (lane & 31)];
        NPD_XF_EPILOGUE(rt * 32, M, dst[row * kLS + col] = gelu(a + bias))
    }
}

// X += hidden[:, 0:128] w_2[:, 0:128]^T + b_2 (in place) and P = hidden[:, 128:256] w_2[:, 128:256]^T
__device__ __forceinline__ void stage_w2(Bufs& s, int M, const float* __restrict__ w, const float* __restrict__ b2,
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
            NPD_XF_EPILOGUE(rt * 32, M, s.X[row * kLS + col] += a + bias)
        } else {
            NPD_XF_EPILOGUE(rt * 32, M, s.P[row * kLS + col] = a)
        }
    }
}

// the FFN block on M rows of X: w_1, GELU, w_2, residual, LayerNorm (the caller synchronises before it)
__device__ __forceinline__ void stage_ffn(Bufs& s, int M, const float* __restrict__ img, const LayerOff& lo, int wave,
                                          int lane) {
    stage_w1(s, M, img + lo.w1, img + lo.b1, wave, lane);
    __syncthreads();
    stage_w2(s, M, img + lo.w2, img + lo.b2, wave, lane);
    __syncthreads();
    stage_ln(s, M, true, img + lo.ln2, wave, lane);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ host: weight image
// B-operand order of W (rows = output features, K columns), column tile ct: [K block c][g][lane][e] =
// W[32 ct + (lane & 31)][64 c + 4 g + e + 32 (lane >> 5)]
static inline void pack_tiles(std::vector<float>& img, const float* W, int nout, int K) {
    for (int ct = 0; ct < nout / 32; ++ct)
        for (int c = 0; c < K / 64; ++c)
            for (int g = 0; g < 8; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 4; ++e)
                        img.push_back(W[(int64_t)(32 * ct + (l & 31)) * K + 64 * c + 4 * g + e + 32 * (l >> 5)]);
}

static inline int push(std::vector<float>& img, const float* p, int64_t n) {
    const int off = (int)img.size();
    img.insert(img.end(), p, p + n);
    while (img.size() % 4) img.push_back(0.0f);
    return off;
}

static inline int push_t(std::vector<float>& img, const float* W, int nout, int K) {  // (nout, K) -> [k][nout]
    const int off = (int)img.size();
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < nout; ++c) img.push_back(W[(int64_t)c * K + k]);
    return off;
}

// one attention block in the state dict's order: w_qs, w_ks, w_vs, fc (E,E each), layer_norm.weight, .bias
static inline const float* push_attention(std::vector<float>& img, const float* p, int* qkv, int* fc, int* ln) {
    *qkv = (int)img.size();
    for (int m = 0; m < 3; ++m) { pack_tiles(img, p, kE, kE); p += kE * kE; }
    *fc = (int)img.size();
    pack_tiles(img, p, kE, kE); p += kE * kE;
    *ln = push(img, p, 2 * kE); p += 2 * kE;
    return p;
}

// the FFN in the state dict's order: w_1.weight (4E,E), w_1.bias, w_2.weight (E,4E), w_2.bias, layer_norm.weight, .bias
static inline const float* push_ffn(std::vector<float>& img, const float* p, LayerOff& lo) {
    lo.w1 = (int)img.size();
    pack_tiles(img, p, kFF, kE); p += kFF * kE;
    lo.b1 = push(img, p, kFF); p += kFF;
    lo.w2 = (int)img.size();
    pack_tiles(img, p, kE, kFF); p += kE * kFF;
    lo.b2 = push(img, p, kE); p += kE;
    lo.ln2 = push(img, p, 2 * kE); p += 2 * kE;
    return p;
}

// the image on the current device; *dev is a hipMalloc'ed copy the caller frees
static inline hipError_t upload(const std::vector<float>& img, int* device, float** dev) {
    hipError_t e = hipGetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)dev, img.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(*dev, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess && *dev) {
        (void)hipFree(*dev);
        *dev = nullptr;
    }
    return e;
}

}  // namespace xf
}  // namespace npd

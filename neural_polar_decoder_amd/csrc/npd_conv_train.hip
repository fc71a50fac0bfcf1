// npd_conv_train.hip -- convNet training (models.py:742-767 in training mode) on MFMA: the kernels.  The plan, the
// workspace layout and the C ABI are in npd_conv_train_api.hip; npd_conv_train.hpp is what this file exports to it.
//
// fp32 throughout, exact fp32 FMA chains on v_mfma_f32_32x32x2_f32, the inference path's layouts: activations
// (B, N, C) with channels contiguous, FC0's flatten order l E + c.
//   * forward: the inference conv / FC kernels' tiling with one more store, the pre-activation z the backward
//     derives GELU' from.
//   * dX of a conv layer: the forward's implicit GEMM on the transposed, tap-flipped weight image; the epilogue adds
//     the gradient arriving along a residual's skip and multiplies by the previous layer's GELU'(z).
//   * dX of a Linear layer: the forward's GEMM on the transposed matrix, the same epilogue.
//   * dW: contractions over the samples (conv: the B N positions, rows = cout, columns = cin, one accumulator per
//     tap; Linear: the B words) into per-workgroup partial sums; db and the LayerNorm gradients: column sums into
//     partial sums.  A reduce kernel adds the partials in a fixed order: no floating-point atomics, equal calls give
//     equal bits.  Inside a workgroup one fp32 chain covers 1024 terms (kFcChain's rule), the chains are added in fp32,
//     the partials in double.
#include "npd_conv_train.hpp"

namespace npd {
namespace conv {

// GELU'(z) = Phi(z) + z phi(z), the erf form of gelu() in npd_conv_common.hpp
__device__ __forceinline__ float gelu_grad(float z) {
    const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    return cdf + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

constexpr f16v kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

// ------------------------------------------------------------------------------ weight images, packed on the device
// A-operand image of conv_layer_kernel (pack_conv_f32's order) of R rows and C contraction channels.  Forward
// (flip = 0): R = cout, C = cin, element (row, cc, t) = w[row][cc][t].  Backward (flip = 1): R = cin, C = cout,
// element (row, cc, t) = w[cc][row][6 - t], the transposed, tap-flipped weights.  w is (cout, cin, 7).
__global__ __launch_bounds__(256) void pack_conv_kernel(const float* __restrict__ w, float* __restrict__ img, int cout,
                                                        int cin, int flip) {
    const int R = flip ? cin : cout, C = flip ? cout : cin;
    const int t32n = (R + 63) / 64 * 2;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (C == 1) {  // layer 0 forward: [t32][lane][4], k-step s of lane half hh is tap 2 s + hh
        if (e >= (int64_t)t32n * 256) return;
        const int s2 = e & 3, l = (e >> 2) & 63, t32 = (int)(e >> 8);
        const int row = 32 * t32 + (l & 31), t = 2 * s2 + (l >> 5);
        img[e] = (row < R && t < 7) ? w[(int64_t)row * 7 + t] : 0.0f;
        return;
    }
    const int ng = C / 8;
    if (e >= (int64_t)t32n * 7 * ng * 256) return;
    const int e4 = e & 3, l = (e >> 2) & 63;
    int64_t rest = e >> 8;
    const int g = (int)(rest % ng);
    rest /= ng;
    const int t = (int)(rest % 7), t32 = (int)(rest / 7);
    const int row = 32 * t32 + (l & 31), cc = (l >> 5) * (C / 2) + 4 * g + e4;
    float v = 0.0f;
    if (row < R) v = flip ? w[((int64_t)cc * cin + row) * 7 + (6 - t)] : w[((int64_t)row * cin + cc) * 7 + t];
    img[e] = v;
}

// Linear images from w (J, K) row-major.  mode 0: FC0 forward, out[j][l E + c] = w[j][c N + l]; mode 1: FC0 backward,
// out[l E + c][j] = w[j][c N + l]; mode 2: the plain transpose out[k][j] = w[j][k].
__global__ __launch_bounds__(256) void pack_fc_kernel(const float* __restrict__ w, float* __restrict__ img, int J,
                                                      int64_t K, int mode, int E, int N) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)J * K) return;
    int64_t j, k;
    if (mode == 0) {
        j = e / K;
        k = e - j * K;
    } else {
        k = e / J;
        j = e - k * J;
    }
    int64_t src = k;
    if (mode < 2) {
        const int64_t l = k / E, c = k - l * E;
        src = c * N + l;
    }
    img[e] = w[j * K + src];
}

// ------------------------------------------------------------------------------ conv layer: forward and dX
// conv_layer_kernel's staging and MFMA loop (npd_conv.hip).  Epilogues, v = acc (+ bias):
//   forward (BWD = 0): zout = v; v = gelu(v) (+ res); out = v
//   dX      (BWD = 1): v += res (the gradient arriving along the skip, or NULL); gout = v (or NULL: the gradient a later
//                      skip needs); out = v * GELU'(gz)
// grid: (N / 64, cout_pad / 64, words); block 256.
template <bool CIN1, bool BWD>
__global__ __launch_bounds__(256) void conv_train_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         const float* __restrict__ res, const float* __restrict__ wimg,
                                                         const float* __restrict__ bias, float* __restrict__ zout,
                                                         const float* __restrict__ gz, float* __restrict__ gout, int cin,
                                                         int cout, int N, int dil) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int l0 = blockIdx.x * 64;
    const int64_t b = blockIdx.z;
    const int halo = 3 * dil;
    const int W = 64 + 2 * halo;
    const int CS = CIN1 ? 4 : cin + 4;
    if constexpr (CIN1) {
        const float* inb = in + b * (int64_t)N;
        for (int p = tid; p < W; p += 256) {
            const int l = l0 - halo + p;
            slab[p * CS] = (l >= 0 && l < N) ? inb[l] : 0.0f;
        }
    } else {
        const int c4n = cin >> 2;
        const f4* inb = reinterpret_cast<const f4*>(in + b * (int64_t)N * cin);
        for (int e = tid; e < W * c4n; e += 256) {
            const int p = e / c4n, c4 = e - p * c4n;
            const int l = l0 - halo + p;
            const f4 v = (l >= 0 && l < N) ? inb[(int64_t)l * c4n + c4] : f4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f4*>(slab + p * CS + 4 * c4) = v;
        }
    }
    __syncthreads();
    const int co_sub = wave & 1, pos_sub = wave >> 1;
    const int co_t32 = blockIdx.y * 2 + co_sub;
    const int pcol = pos_sub * 32 + col;
    f16v acc = kZero16;
    if constexpr (CIN1) {
        const f4 w = reinterpret_cast<const f4*>(wimg)[co_t32 * 64 + lane];
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            const int t = 2 * s2 + h;
            const float bv = t < 7 ? slab[(pcol + dil * t) * CS] : 0.0f;
            acc = mfma(w[s2], bv, acc);
        }
    } else {
        const int ng = cin >> 3;
        const f4* wq = reinterpret_cast<const f4*>(wimg) + (int64_t)co_t32 * 7 * ng * 64 + lane;
        f4 wn = wq[0];
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const f4* brow = reinterpret_cast<const f4*>(slab + (pcol + dil * t) * CS + h * (cin >> 1));
            for (int g = 0; g < ng; ++g) {
                const f4 w = wn;
                const int nxt = t * ng + g + 1;
                if (nxt < 7 * ng) wn = wq[nxt * 64];
                const f4 bv = brow[g];
                acc = mfma(w.x, bv.x, acc);
                acc = mfma(w.y, bv.y, acc);
                acc = mfma(w.z, bv.z, acc);
                acc = mfma(w.w, bv.w, acc);
            }
        }
    }
    const int l = l0 + pcol;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int co = co_t32 * 32 + 8 * q + 4 * h;
        if (co < cout) {
            const int64_t o = (b * N + l) * (int64_t)cout + co;
            f4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
            if constexpr (!BWD) {
                v += *reinterpret_cast<const f4*>(bias + co);
                *reinterpret_cast<f4*>(zout + o) = v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = gelu(v[e]);
                if (res != nullptr) v += *reinterpret_cast<const f4*>(res + o);
            } else {
                if (res != nullptr) v += *reinterpret_cast<const f4*>(res + o);
                if (gout != nullptr) *reinterpret_cast<f4*>(gout + o) = v;
                const f4 z = *reinterpret_cast<const f4*>(gz + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= gelu_grad(z[e]);
            }
            *reinterpret_cast<f4*>(out + o) = v;
        }
    }
}

// ------------------------------------------------------------------------------ Linear layer: forward and dX
// fc_kernel's tiling (npd_conv.hip): out[m][j] = sum_k X[m][k] Wt[j][k], v = that (+ bias[j]); zout = v (or NULL);
// v = gelu(v) if act; v *= GELU'(gz[m][j]) (or NULL); out = v.
constexpr int GK = 32;
constexpr int GS = GK + 4;
constexpr int kChain = 32;  // 32-term blocks per fp32 accumulation chain: 1024 terms, fc_kernel's kFcChain

__global__ __launch_bounds__(256) void fc_train_kernel(const float* __restrict__ X, const float* __restrict__ Wt,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       float* __restrict__ zout, const float* __restrict__ gz, int M,
                                                       int64_t K, int64_t Nout, int act) {
    __shared__ __attribute__((aligned(16))) float As[2][64 * GS];
    __shared__ __attribute__((aligned(16))) float Bs[2][64 * GS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int m0 = blockIdx.y * 64;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    const int msub = wave & 1, jsub = wave >> 1;
    f4 ra[2], rb[2];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx >> 3, c4 = (idx & 7) * 4;
            int mr = m0 + r;
            if (mr >= M) mr = M - 1;
            ra[u] = *reinterpret_cast<const f4*>(X + (int64_t)mr * K + k0 + c4);
            rb[u] = *reinterpret_cast<const f4*>(Wt + (j0 + r) * K + k0 + c4);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx >> 3, c4 = (idx & 7) * 4;
            *reinterpret_cast<f4*>(&As[buf][r * GS + c4]) = ra[u];
            *reinterpret_cast<f4*>(&Bs[buf][r * GS + c4]) = rb[u];
        }
    };
    f16v acc = kZero16, tot = kZero16;
    const int64_t nk = K / GK;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int64_t kb0 = 0; kb0 < nk; kb0 += kChain) {
        const int64_t kend = kb0 + kChain < nk ? kb0 + kChain : nk;
        for (int64_t kb = kb0; kb < kend; ++kb) {
            const int cur = (int)(kb & 1);
            if (kb + 1 < nk) fetch((kb + 1) * GK);
            const f4* as = reinterpret_cast<const f4*>(&As[cur][(msub * 32 + col) * GS + h * (GK / 2)]);
            const f4* bs = reinterpret_cast<const f4*>(&Bs[cur][(jsub * 32 + col) * GS + h * (GK / 2)]);
#pragma unroll
            for (int g = 0; g < GK / 8; ++g) {
                const f4 a = as[g], bq = bs[g];
                acc = mfma(a.x, bq.x, acc);
                acc = mfma(a.y, bq.y, acc);
                acc = mfma(a.z, bq.z, acc);
                acc = mfma(a.w, bq.w, acc);
            }
            if (kb + 1 < nk) stash(cur ^ 1);
            __syncthreads();
        }
        tot += acc;
        acc = kZero16;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + msub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int64_t j = j0 + jsub * 32 + col;
        if (m < M) {
            const int64_t o = (int64_t)m * Nout + j;
            float v = tot[r] + (bias != nullptr ? bias[j] : 0.0f);
            if (zout != nullptr) zout[o] = v;
            if (act) v = gelu(v);
            if (gz != nullptr) v *= gelu_grad(gz[o]);
            out[o] = v;
        }
    }
}

// ------------------------------------------------------------------------------ Linear layer: dW
// dW[j][k] = sum_m dZ[m][j] X[m][k] over the words m of split blockIdx.z (rps words each, a multiple of 32): MFMA rows
// = j, columns = k, the contraction runs over 32-word blocks staged in LDS as [word][64 columns] rows of stride 96 (the
// two lane halves read words 2 s and 2 s + 1, 96 floats = 32 banks apart).  Words past M are zeros.  The tile goes to
// part[split][j][k], or with one split straight to the gradient (permE > 0: FC0, column k = l E + c lands at
// c N + l, torch's flatten order).  grid: (K / 64, J / 64, splits); block 256 = 2 (j) x 2 (k) waves.
constexpr int DS = 96;

__device__ __forceinline__ int64_t fc0_col(int64_t k, int permE, int permN) {
    if (permE == 0) return k;
    const int64_t l = k / permE, c = k - l * permE;
    return c * permN + l;
}

__global__ __launch_bounds__(256) void fc_dw_kernel(const float* __restrict__ dZ, const float* __restrict__ X,
                                                    float* __restrict__ part, int M, int64_t J, int64_t K, int rps,
                                                    int permE, int permN) {
    __shared__ __attribute__((aligned(16))) float As[2][32 * DS];
    __shared__ __attribute__((aligned(16))) float Bs[2][32 * DS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int64_t k0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
    const int jsub = wave & 1, ksub = wave >> 1;
    const int mb = blockIdx.z * rps;
    const int me = min(M, mb + rps);
    f4 ra[2], rb[2];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx >> 4, c4 = (idx & 15) * 4;
            const int m = m0 + r;
            const bool ok = m < me;
            ra[u] = ok ? *reinterpret_cast<const f4*>(dZ + (int64_t)m * J + j0 + c4) : f4{0.f, 0.f, 0.f, 0.f};
            rb[u] = ok ? *reinterpret_cast<const f4*>(X + (int64_t)m * K + k0 + c4) : f4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx >> 4, c4 = (idx & 15) * 4;
            *reinterpret_cast<f4*>(&As[buf][r * DS + c4]) = ra[u];
            *reinterpret_cast<f4*>(&Bs[buf][r * DS + c4]) = rb[u];
        }
    };
    f16v acc = kZero16, tot = kZero16;
    const int nblk = (me - mb + 31) / 32;
    fetch(mb);
    stash(0);
    __syncthreads();
    for (int i0 = 0; i0 < nblk; i0 += kChain) {
        const int iend = min(nblk, i0 + kChain);
        for (int i = i0; i < iend; ++i) {
            const int cur = i & 1;
            if (i + 1 < nblk) fetch(mb + (i + 1) * 32);
            const float* as = &As[cur][h * DS + jsub * 32 + col];
            const float* bs = &Bs[cur][h * DS + ksub * 32 + col];
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = mfma(as[2 * s * DS], bs[2 * s * DS], acc);
            if (i + 1 < nblk) stash(cur ^ 1);
            __syncthreads();
        }
        tot += acc;
        acc = kZero16;
    }
    float* dst = part + (int64_t)blockIdx.z * J * K;
    const int64_t k = fc0_col(k0 + ksub * 32 + col, permE, permN);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t j = j0 + jsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[j * K + k] = tot[r];
    }
}

// ------------------------------------------------------------------------------ conv layer: dW
// dW[co][ci][t] = sum_{b,l} dZ[b][l][co] X[b][l + d (t - 3)][ci], X zero outside [0, N).  An item is one word's 64
// positions; a workgroup takes the items [ipb blockIdx.y, ipb (blockIdx.y + 1)) of one (64 co) x (64 ci) tile, stages
// dZ's 64 x 64 tile and X's (64 + 6 d) x 64 slab (zero halo, zero channels past cout / cin) in LDS as rows of stride
// 96, and each wave holds a 32 x 32 (co, ci) tile for all 7 taps: one A operand (dZ) feeds 7 MFMAs.  The workgroup's
// items are one fp32 chain: conv_dw_splits gives a workgroup 16 items (1024 terms) while the partials fit its cap, and
// a second set of accumulators to end chains inside the kernel would leave one wave per SIMD.  CIN1 (layer 0): the
// columns are the 7 taps, one accumulator.
// part[split][co][ci][t] (the gradient's order).  grid: (co tiles x ci tiles, splits); block 256 = 2 (co) x 2 (ci).

template <bool CIN1>
__global__ __launch_bounds__(256) void conv_dw_kernel(const float* __restrict__ dZ, const float* __restrict__ X,
                                                      float* __restrict__ part, int cin, int cout, int N, int dil,
                                                      int64_t items, int ipb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NT = CIN1 ? 1 : 7;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int citn = CIN1 ? 1 : (cin + 63) / 64;
    const int co0 = (blockIdx.x / citn) * 64, ci0 = (blockIdx.x % citn) * 64;
    const int co_sub = wave & 1, ci_sub = wave >> 1;
    const int halo = 3 * dil, W = 64 + 2 * halo;
    float* dzs = lds;            // [64][DS]
    float* xs = lds + 64 * DS;   // [W][DS] (CIN1: [W])
    const int ntile = N / 64;
    const bool active = co0 + co_sub * 32 < cout && (CIN1 ? ci_sub == 0 : ci0 + ci_sub * 32 < cin);
    f16v acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = kZero16;
    const int64_t it0 = (int64_t)blockIdx.y * ipb;
    const int64_t it1 = it0 + ipb < items ? it0 + ipb : items;
    for (int64_t it = it0; it < it1; ++it) {
        const int64_t b = it / ntile;
        const int l0 = (int)(it - b * ntile) * 64;
        for (int e = tid; e < 64 * 16; e += 256) {
            const int p = e >> 4, c4 = (e & 15) * 4;
            const int ch = co0 + c4;
            const f4 v = ch < cout ? *reinterpret_cast<const f4*>(dZ + (b * N + l0 + p) * (int64_t)cout + ch)
                                   : f4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f4*>(dzs + p * DS + c4) = v;
        }
        if constexpr (CIN1) {
            for (int p = tid; p < W; p += 256) {
                const int l = l0 - halo + p;
                xs[p] = (l >= 0 && l < N) ? X[b * N + l] : 0.0f;
            }
        } else {
            for (int e = tid; e < W * 16; e += 256) {
                const int p = e >> 4, c4 = (e & 15) * 4;
                const int ch = ci0 + c4, l = l0 - halo + p;
                const f4 v = (ch < cin && l >= 0 && l < N) ? *reinterpret_cast<const f4*>(X + (b * N + l) * (int64_t)cin + ch)
                                                           : f4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f4*>(xs + p * DS + c4) = v;
            }
        }
        __syncthreads();
        if (active) {
            const float* ap = dzs + h * DS + co_sub * 32 + col;
            if constexpr (CIN1) {
#pragma unroll 8
                for (int s = 0; s < 32; ++s) {
                    const float bv = col < 7 ? xs[2 * s + h + dil * col] : 0.0f;
                    acc[0] = mfma(ap[2 * s * DS], bv, acc[0]);
                }
            } else {
                const float* bp = xs + h * DS + ci_sub * 32 + col;
#pragma unroll 4
                for (int s = 0; s < 32; ++s) {
                    const float a = ap[2 * s * DS];
#pragma unroll
                    for (int t = 0; t < 7; ++t) acc[t] = mfma(a, bp[(2 * s + dil * t) * DS], acc[t]);
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float* dst = part + (int64_t)blockIdx.y * cout * cin * 7;
    if constexpr (CIN1) {
        if (col < 7) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + co_sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < cout) dst[co * 7 + col] = acc[0][r];
            }
        }
    } else {
        const int ci = ci0 + ci_sub * 32 + col;
        if (ci < cin) {
#pragma unroll
            for (int t = 0; t < 7; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + co_sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (co < cout) dst[((int64_t)co * cin + ci) * 7 + t] = acc[t][r];
                }
        }
    }
}

// ------------------------------------------------------------------------------ column sums (db, LayerNorm dg / db)
// part[split][c] = sum of A[m][c] over the rows m of split blockIdx.y (rps rows): each thread sums every 4th row of
// one column in fp32 (rps / 4 <= 1024 terms), the 4 row groups are added in a fixed order.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ A, float* __restrict__ part, int64_t M,
                                                     int C, int rps) {
    __shared__ float sh[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.y * rps;
    const int64_t m1 = m0 + rps < M ? m0 + rps : M;
    float s = 0.0f;
    if (c < C)
        for (int64_t m = m0 + g; m < m1; m += 4) s += A[m * C + c];
    sh[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < C) part[(int64_t)blockIdx.y * C + c] = ((sh[0][c & 63] + sh[1][c & 63]) + sh[2][c & 63]) + sh[3][c & 63];
}

// out[dest(i)] = sum over the S partials of element i, added in order in double.  permE > 0: FC0's weight, element
// (j, l E + c) lands at (j, c N + l).
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n,
                                                     int S, int64_t K, int permE, int permN) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += (double)part[(int64_t)k * n + i];
    int64_t d = i;
    if (permE > 0) {
        const int64_t j = i / K;
        d = j * K + fc0_col(i - j * K, permE, permN);
    }
    out[d] = (float)s;
}

// ------------------------------------------------------------------------------ dropout + LayerNorm
// One wave per word.  Forward: d = fc2 * drop (in place; drop NULL: none), mean and rstd kept, logits =
// layernorm_sign_kernel's arithmetic.
__global__ __launch_bounds__(256) void ln_fwd_kernel(float* __restrict__ d, const float* __restrict__ drop,
                                                     const float* __restrict__ g, const float* __restrict__ be,
                                                     float* __restrict__ logits, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, int64_t M, int N) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    float* r = d + m * N;
    float s = 0.0f;
    for (int i = lane; i < N; i += 64) {
        float v = r[i];
        if (drop != nullptr) {
            v *= drop[m * N + i];
            r[i] = v;
        }
        s += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)N;
    float v = 0.0f;
    for (int i = lane; i < N; i += 64) {
        const float x = r[i] - mean;
        v += x * x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const float rstd = 1.0f / sqrtf(v / (float)N + 1e-6f);
    for (int i = lane; i < N; i += 64) logits[m * N + i] = (r[i] - mean) * rstd * g[i] + be[i];
    if (lane == 0) {
        mean_out[m] = mean;
        rstd_out[m] = rstd;
    }
}

// Backward: xh = (d - mean) rstd, a = dy g; dd = rstd (a - mean(a) - xh mean(a xh)); dz = dd * drop; dgt = dy xh
// (its column sum is the LayerNorm weight's gradient; dy's own is the bias's).
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ d, const float* __restrict__ drop,
                                                     const float* __restrict__ g, const float* __restrict__ dy,
                                                     const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                     float* __restrict__ dz, float* __restrict__ dgt, int64_t M, int N) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float mean = mean_in[m], rstd = rstd_in[m];
    const float* r = d + m * N;
    const float* gy = dy + m * N;
    float s1 = 0.0f, s2 = 0.0f;
    for (int i = lane; i < N; i += 64) {
        const float xh = (r[i] - mean) * rstd, a = gy[i] * g[i];
        s1 += a;
        s2 += a * xh;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    s1 /= (float)N;
    s2 /= (float)N;
    for (int i = lane; i < N; i += 64) {
        const float xh = (r[i] - mean) * rstd, a = gy[i] * g[i];
        float v = rstd * (a - s1 - xh * s2);
        if (drop != nullptr) v *= drop[m * N + i];
        dz[m * N + i] = v;
        dgt[m * N + i] = gy[i] * xh;
    }
}

// ------------------------------------------------------------------------------ host: launches
static unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

int train_pack_conv(const float* w, float* img, int cout, int cin, int flip, hipStream_t s) {
    const int R = flip ? cin : cout, C = flip ? cout : cin;
    hipLaunchKernelGGL(pack_conv_kernel, dim3(blocks_of(conv_img_floats(R, C))), dim3(256), 0, s, w, img, cout, cin, flip);
    return launch_check("pack_conv_kernel launch");
}

int train_pack_fc(const float* w, float* img, int J, int64_t K, int mode, int E, int N, hipStream_t s) {
    hipLaunchKernelGGL(pack_fc_kernel, dim3(blocks_of((int64_t)J * K)), dim3(256), 0, s, w, img, J, K, mode, E, N);
    return launch_check("pack_fc_kernel launch");
}

// grid.z carries the words: at most kWordsPerLaunch per launch
constexpr int64_t kWordsPerLaunch = 32768;

int train_conv_layer(bool bwd, const float* in, float* out, const float* res, const float* wimg, const float* bias,
                     float* zout, const float* gz, float* gout, int cin, int cout, int N, int dil, int64_t B,
                     hipStream_t s) {
    const size_t lds = (size_t)(cin == 1 ? 4 : cin + 4) * (64 + 6 * dil) * 4;
    for (int64_t b0 = 0; b0 < B; b0 += kWordsPerLaunch) {
        const int64_t nb = B - b0 < kWordsPerLaunch ? B - b0 : kWordsPerLaunch;
        const dim3 grid(N / 64, (cout + 63) / 64, (unsigned)nb);
        const int64_t oi = b0 * N * cin, oo = b0 * N * cout;
        auto at = [](auto* p, int64_t o) { return p ? p + o : p; };
        int rc;
        if (bwd)
            rc = launch_lds<conv_train_kernel<false, true>>("conv_train_kernel (dX) launch", grid, 256, lds, s, in + oi,
                                                            out + oo, at(res, oo), wimg, bias, at(zout, oo), at(gz, oo),
                                                            at(gout, oo), cin, cout, N, dil);
        else if (cin == 1)
            rc = launch_lds<conv_train_kernel<true, false>>("conv_train_kernel launch", grid, 256, lds, s, in + oi,
                                                            out + oo, at(res, oo), wimg, bias, at(zout, oo), at(gz, oo),
                                                            at(gout, oo), cin, cout, N, dil);
        else
            rc = launch_lds<conv_train_kernel<false, false>>("conv_train_kernel launch", grid, 256, lds, s, in + oi,
                                                             out + oo, at(res, oo), wimg, bias, at(zout, oo), at(gz, oo),
                                                             at(gout, oo), cin, cout, N, dil);
        if (rc) return rc;
    }
    return NPD_OK;
}

int train_fc(const float* X, const float* Wt, const float* bias, float* out, float* zout, const float* gz, int64_t M,
             int64_t K, int64_t Nout, int act, hipStream_t s) {
    hipLaunchKernelGGL(fc_train_kernel, dim3((unsigned)(Nout / 64), (unsigned)((M + 63) / 64)), dim3(256), 0, s, X, Wt, bias,
                       out, zout, gz, (int)M, K, Nout, act);
    return launch_check("fc_train_kernel launch");
}

int train_reduce(const float* part, float* out, int64_t n, int S, int64_t K, int permE, int permN, hipStream_t s) {
    hipLaunchKernelGGL(reduce_kernel, dim3(blocks_of(n)), dim3(256), 0, s, part, out, n, S, K, permE, permN);
    return launch_check("reduce_kernel launch");
}

int train_fc_dw(const float* dZ, const float* X, float* part, float* grad, int64_t M, int64_t J, int64_t K, int permE,
                int permN, hipStream_t s) {
    int rps;
    const int S = fc_dw_splits(M, J, K, &rps);
    const dim3 grid((unsigned)(K / 64), (unsigned)(J / 64), (unsigned)S);
    if (S == 1) {  // one split: the tile is the gradient
        hipLaunchKernelGGL(fc_dw_kernel, grid, dim3(256), 0, s, dZ, X, grad, (int)M, J, K, rps, permE, permN);
        return launch_check("fc_dw_kernel launch");
    }
    hipLaunchKernelGGL(fc_dw_kernel, grid, dim3(256), 0, s, dZ, X, part, (int)M, J, K, rps, 0, 0);
    const int rc = launch_check("fc_dw_kernel launch");
    return rc ? rc : train_reduce(part, grad, J * K, S, K, permE, permN, s);
}

int train_conv_dw(const float* dZ, const float* X, float* part, float* grad, int cin, int cout, int N, int dil, int64_t B,
                  hipStream_t s) {
    const int64_t items = B * (N / 64);
    int ipb;
    const int S = conv_dw_splits(items, cin, cout, &ipb);
    const int tiles = ((cout + 63) / 64) * (cin == 1 ? 1 : (cin + 63) / 64);
    const size_t lds = (size_t)(64 * DS + (cin == 1 ? 64 + 6 * dil : (64 + 6 * dil) * DS)) * 4;
    int rc;
    if (cin == 1)
        rc = launch_lds<conv_dw_kernel<true>>("conv_dw_kernel launch", dim3(tiles, S), 256, lds, s, dZ, X, part, cin, cout, N,
                                              dil, items, ipb);
    else
        rc = launch_lds<conv_dw_kernel<false>>("conv_dw_kernel launch", dim3(tiles, S), 256, lds, s, dZ, X, part, cin, cout,
                                               N, dil, items, ipb);
    return rc ? rc : train_reduce(part, grad, (int64_t)cout * cin * 7, S, 0, 0, 0, s);
}

int train_colsum(const float* A, float* part, float* grad, int64_t M, int C, hipStream_t s) {
    const int S = colsum_splits(M);
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 63) / 64, S), dim3(256), 0, s, A, part, M, C, kColsumRows);
    const int rc = launch_check("colsum_kernel launch");
    return rc ? rc : train_reduce(part, grad, C, S, 0, 0, 0, s);
}

int train_ln_fwd(float* d, const float* drop, const float* g, const float* be, float* logits, float* mean, float* rstd,
                 int64_t M, int N, hipStream_t s) {
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, d, drop, g, be, logits, mean, rstd, M, N);
    return launch_check("ln_fwd_kernel launch");
}

int train_ln_bwd(const float* d, const float* drop, const float* g, const float* dy, const float* mean, const float* rstd,
                 float* dz, float* dgt, int64_t M, int N, hipStream_t s) {
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, d, drop, g, dy, mean, rstd, dz, dgt, M,
                       N);
    return launch_check("ln_bwd_kernel launch");
}

}  // namespace conv
}  // namespace npd

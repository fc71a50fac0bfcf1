// npd_conv.hip -- convNet decoder (models.py:691-772) on MFMA.
//
// Reference forward (models.py:742-767): 10 dilated Conv1d(k=7) + GELU with three residual blocks,
// flatten (c*N + l), Linear(E*N -> 4N) + GELU, Linear(4N -> N) + GELU, Linear(N -> N), Dropout (eval:
// identity), LayerNorm(N, eps 1e-6), decisions = sign(logits).
//
// MI355X mapping (fp32 path, v_mfma_f32_32x32x2_f32, exact fp32 FMA chains):
//   * conv layer = implicit GEMM  out[co][l] = sum_{t,ci} W[co][ci][t] * in[ci][l + d(t-3)]:
//     MFMA rows = output channels (A = weights, pre-permuted on the host into A-operand order,
//     k = t*Cin + ci), columns = positions (B = the input slab staged in LDS with its zero halo);
//     the epilogue fuses bias + GELU (+ residual) and writes 32 consecutive positions per register.
//   * FC layers = LDS-tiled GEMM with MFMA rows = codewords, columns = output features (so the
//     epilogue writes contiguous feature runs), bias + GELU fused.
//   * LayerNorm + sign: one wave per codeword.
// Activations of a chunk of codewords live in a caller-provided workspace, (B, N, C) (channels
// contiguous); FC0's weights are permuted on the host to that flatten order.
//
// This file: the kernels every precision uses (the fp32 conv layer and FC GEMM, LayerNorm + sign, the tap transpose).
// The fp16x3 kernels (precision 3) are in npd_conv_slab.hip, npd_conv_ws.hip and npd_conv_fc.hip, the
// handle and the C ABI in npd_conv_api.hip; npd_conv_host.hpp holds the per-layer plan that ties them together.
#include "npd_conv_host.hpp"

namespace npd {
namespace conv {

// ------------------------------------------------------------------------------ conv layer
// Activations are (B, N, C) -- channels contiguous per position -- so a block's input slab (64 positions
// plus the dilation halo, all channels) is one contiguous run in HBM (16-B loads) and lands in LDS as
// [position][channel] rows of stride CS = cin + 4 (16-B aligned, conflict-free ds_read_b128 across the
// 32 position columns of a wave).  MFMA k-steps run tap by tap; within tap t, k-step s pairs channel s
// (lane half 0) with channel s + cin/2 (half 1), so the B operands of 4 consecutive k-steps are one
// ds_read_b128 and the A operands (weights, permuted on the host in the same order) one 16-B load.
// The accumulator's registers 4q..4q+3 hold 4 consecutive output channels of one position: bias, GELU,
// residual and the store are 16-B vectors.  Layer 0 (cin = 1): the 7 taps are the k-steps (padded to 8).
// grid: (N/64 position tiles, cout_pad/64 channel tiles, codewords); block 256 = 2 (co) x 2 (pos) waves.
template <bool CIN1>
__global__ __launch_bounds__(256) void conv_layer_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         const float* __restrict__ res, const float* __restrict__ wimg,
                                                         const float* __restrict__ bias, int cin, int cout, int N,
                                                         int dil, int do_res, uint32_t* __restrict__ amax_out) {
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
    const int co_t32 = blockIdx.y * 2 + co_sub;  // 32-channel tile index
    const int pcol = pos_sub * 32 + col;
    f16v acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (CIN1) {
        const f4 w = reinterpret_cast<const f4*>(wimg)[co_t32 * 64 + lane];
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            const int t = 2 * s2 + h;
            const float bv = t < 7 ? slab[(pcol + dil * t) * CS] : 0.0f;
            acc = mfma(w[s2], bv, acc);
        }
    } else {
        const int ng = cin >> 3;  // groups of 4 k-steps per tap
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
    // epilogue: registers 4q..4q+3 = channels co_t32*32 + 8q + 4h + 0..3 at position l0 + pcol
    const int l = l0 + pcol;
    float amx = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int co = co_t32 * 32 + 8 * q + 4 * h;
        if (co < cout) {
            const int64_t o = (b * N + l) * (int64_t)cout + co;
            const f4 bb = *reinterpret_cast<const f4*>(bias + co);
            f4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu(acc[4 * q + e] + bb[e]);
            if (do_res) {
                const f4 rv = *reinterpret_cast<const f4*>(res + o);
                v += rv;
            }
            *reinterpret_cast<f4*>(out + o) = v;
            amx = fmaxf(amx, amax4(v));
        }
    }
    if (amax_out != nullptr) publish_amax(amax_out, amx);
}

// ------------------------------------------------------------------------------ FC GEMM
// out[m][j] = act(sum_k X[m][k] * Wt[j][k] + bias[j]);  block tile 64 (m) x 64 (j), K step 32.
// LDS rows of stride GK + 4 (16-B aligned; 32 rows read with ds_read_b128 at one k offset hit every bank
// once per 16 lanes).  Within a K block, k-step s pairs k = s (lane half 0) with k = s + GK/2 (half 1),
// so the A and B operands of 4 consecutive k-steps are one ds_read_b128 each (round 1: two ds_read_b32
// per MFMA) and the tile lands in LDS with 16-B stores.
constexpr int GK = 32;
constexpr int GS = GK + 4;
constexpr int kFcChain = 32;  // K blocks per accumulation chain of fc_kernel

__global__ __launch_bounds__(256) void fc_kernel(const float* __restrict__ X, const float* __restrict__ Wt,
                                                 const float* __restrict__ bias, float* __restrict__ out, int M, int K,
                                                 int Nout, int act) {
    __shared__ __attribute__((aligned(16))) float As[2][64 * GS];
    __shared__ __attribute__((aligned(16))) float Bs[2][64 * GS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int m0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int msub = wave & 1, jsub = wave >> 1;
    // loader mapping: 64 rows x 32 k = 512 float4 per operand; thread loads 2 float4 of A and of B
    f4 ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;  // 0..511
            const int r = idx >> 3, c4 = (idx & 7) * 4;
            int mr = m0 + r;
            if (mr >= M) mr = M - 1;
            ra[u] = *reinterpret_cast<const f4*>(X + (int64_t)mr * K + k0 + c4);
            rb[u] = *reinterpret_cast<const f4*>(Wt + (int64_t)(j0 + r) * K + k0 + c4);
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
    // one fp32 accumulation chain covers kFcChain K blocks (1024 terms); the chains' sums are added in tot.  A single
    // chain over FC0's K = E N terms (up to 65536 here) rounds about sqrt(K) times: 1.3e-7 on O(0.1) outputs at
    // K = 65536, 14 x a blocked fp32 GEMM's error (tests/conv_layers_helper.py)
    f16v acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f16v tot = acc;
    const int nk = K / GK;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int kb0 = 0; kb0 < nk; kb0 += kFcChain) {
        const int kend = min(nk, kb0 + kFcChain);
        for (int kb = kb0; kb < kend; ++kb) {
            const int cur = kb & 1;
            if (kb + 1 < nk) fetch((kb + 1) * GK);
            const f4* as = reinterpret_cast<const f4*>(&As[cur][(msub * 32 + col) * GS + h * (GK / 2)]);
            const f4* bs = reinterpret_cast<const f4*>(&Bs[cur][(jsub * 32 + col) * GS + h * (GK / 2)]);
#pragma unroll
            for (int g = 0; g < GK / 8; ++g) {
                const f4 a = as[g], b = bs[g];
                acc = mfma(a.x, b.x, acc);
                acc = mfma(a.y, b.y, acc);
                acc = mfma(a.z, b.z, acc);
                acc = mfma(a.w, b.w, acc);
            }
            if (kb + 1 < nk) stash(cur ^ 1);
            __syncthreads();
        }
        tot += acc;
        acc = f16v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + msub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int j = j0 + jsub * 32 + col;
        if (m < M) {
            float v = tot[r] + bias[j];
            if (act) v = gelu(v);
            out[(int64_t)m * Nout + j] = v;
        }
    }
}

// ------------------------------------------------------------------------------ LayerNorm + sign
__global__ __launch_bounds__(256) void layernorm_sign_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ be, float* __restrict__ logits,
                                                             float* __restrict__ dec, int M, int N) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* r = x + m * N;
    float s = 0.0f;
    for (int i = lane; i < N; i += 64) s += r[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)N;
    float v = 0.0f;
    for (int i = lane; i < N; i += 64) {
        const float d = r[i] - mean;
        v += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const float rstd = 1.0f / sqrtf(v / (float)N + 1e-6f);
    for (int i = lane; i < N; i += 64) {
        const float y = (r[i] - mean) * rstd * g[i] + be[i];
        if (logits) logits[m * N + i] = y;
        if (dec) dec[m * N + i] = y > 0.0f ? 1.0f : (y < 0.0f ? -1.0f : 0.0f);
    }
}

}  // namespace conv
}  // namespace npd

// input4 (models.py:750, returned by convNet.forward): the (nb, N, C) activation after layers3 (+ residual) as
// the reference's channels-first (nb, C, N).  A 64 x 64 (position x channel) tile per workgroup through LDS,
// so both the reads (channels contiguous) and the writes (positions contiguous) are coalesced.
__global__ __launch_bounds__(256) void act_to_channels_first_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                    int N, int C) {
    __shared__ float t[64][65];
    const int64_t b = blockIdx.z;
    const int l0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const float* src = in + b * (int64_t)N * C;
    float* dst = out + b * (int64_t)N * C;
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int l = e >> 6, cc = e & 63;
        if (l0 + l < N && c0 + cc < C) t[l][cc] = src[(int64_t)(l0 + l) * C + c0 + cc];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int cc = e >> 6, l = e & 63;
        if (l0 + l < N && c0 + cc < C) dst[(int64_t)(c0 + cc) * N + l0 + l] = t[l][cc];
    }
}

namespace npd {
namespace conv {

// ------------------------------------------------------------------------------ host
// conv_layer_kernel's fp32 A operands; channel tiles padded to 64 so every (64-channel) block has two 32-row MFMA tiles
void pack_conv_f32(const float* w, LayerPlan& L, std::vector<float>& img) {
    const int co = L.cout, ci = L.cin, t32n = (co + 63) / 64 * 2;
    if (ci == 1) {
        // [t32][lane][4]: k-step s of lane half hh is tap 2s + hh (tap 7 = 0)
        L.woff = append_aligned(img, (size_t)t32n * 64 * 4);
        for (int t32 = 0; t32 < t32n; ++t32)
            for (int l = 0; l < 64; ++l)
                for (int s2 = 0; s2 < 4; ++s2) {
                    const int row = 32 * t32 + (l & 31), t = 2 * s2 + (l >> 5);
                    img[L.woff + ((int64_t)t32 * 64 + l) * 4 + s2] = (row < co && t < 7) ? w[(int64_t)row * 7 + t] : 0.0f;
                }
        return;
    }
    // [t32][tap][group][lane][4]: k-step 4g+e of tap t pairs channel 4g+e (half 0) with cin/2 + 4g+e
    const int ng = ci / 8;
    L.woff = append_aligned(img, (size_t)t32n * 7 * ng * 64 * 4);
    for (int t32 = 0; t32 < t32n; ++t32)
        for (int t = 0; t < 7; ++t)
            for (int g = 0; g < ng; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 4; ++e) {
                        const int row = 32 * t32 + (l & 31);
                        const int cc = (l >> 5) * (ci / 2) + 4 * g + e;
                        img[L.woff + ((((int64_t)t32 * 7 + t) * ng + g) * 64 + l) * 4 + e] =
                            row < co ? w[((int64_t)row * ci + cc) * 7 + t] : 0.0f;
                    }
}

int launch_conv_f32(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    const size_t lds = (size_t)(L.cin == 1 ? 4 : L.cin + 4) * (64 + 6 * L.dil) * 4;
    const dim3 grid(a.N / 64, (L.cout + 63) / 64, (unsigned)a.nb);
    const float *w = a.img + L.woff, *b = a.img + L.boff;
    if (L.cin == 1)
        return launch_lds<conv_layer_kernel<true>>("conv_layer_kernel launch", grid, 256, lds, s, a.in, a.out, a.res, w, b,
                                                   L.cin, L.cout, a.N, L.dil, L.res, a.am_out);
    return launch_lds<conv_layer_kernel<false>>("conv_layer_kernel launch", grid, 256, lds, s, a.in, a.out, a.res, w, b,
                                                L.cin, L.cout, a.N, L.dil, L.res, a.am_out);
}

int launch_fc_f32(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    const dim3 grid(L.cout / 64, (unsigned)((a.nb + 63) / 64));
    hipLaunchKernelGGL(fc_kernel, grid, dim3(256), 0, s, a.in, a.img + L.woff, a.img + L.boff, a.out, (int)a.nb, L.cin,
                       L.cout, L.res);
    return launch_check("fc_kernel launch");
}

int launch_channels_first(const float* in, float* out, int N, int C, int64_t nb, hipStream_t s) {
    hipLaunchKernelGGL(act_to_channels_first_kernel, dim3((N + 63) / 64, (C + 63) / 64, (unsigned)nb), dim3(256), 0, s, in,
                       out, N, C);
    return launch_check("tap transpose launch");
}

int launch_layernorm_sign(const float* x, const float* g, const float* be, float* logits, float* dec, int64_t M, int N,
                          hipStream_t s) {
    hipLaunchKernelGGL(layernorm_sign_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, g, be, logits, dec,
                       (int)M, N);
    return launch_check("layernorm launch");
}

}  // namespace conv
}  // namespace npd

// npd_gru_train.hip -- CRISP GRU training (RNN_decoder.decode(net, True, y, gt, tfr), rnn_all.py:422-512) on fused kernels.
//
//  gru_train_pack_kernel  the flat device weight vector -> the LDS images (the weights change every optimiser step, so
//                         the images are packed on the device: no host copy, no synchronisation)
//  gru_train_fwd_kernel   gru_decode_kernel's geometry (gate rows = MFMA rows, 32 codewords per wave = columns, 4 waves
//                         per workgroup, weights in LDS); per step and layer it also stores h', r, z, n and a_hn, and the
//                         value fed to the next step (teacher forcing: gt; student forcing: the sign of its own output)
//  gru_train_bwd_kernel   the recurrence backwards over the three transposed matrices in LDS; the gate gradients
//                         Delta are computed in accumulator layout, which is register for register the B operand of
//                         the transposed MFMAs; Delta goes to the scratch buffer
//  gru_train_contract_kernel / gru_train_reduce_kernel
//                         every weight gradient is a tall-skinny GEMM over the N B samples (fp32 MFMA, both operands
//                         read along their contiguous rows); the samples are split over workgroups into partial sums
//                         that a second pass adds in a fixed order -- no floating-point atomics, so two identical
//                         calls return the same bits
//
// The gates use expf / tanhf and a true division (not the decode kernels' v_exp_f32 / v_rcp_f32): gradients are held to
// a multiple of torch's own fp32 autograd error (tests/test_gru_train_gpu.py).
#include <new>

#include "npd_gru_train.hpp"

namespace npd {
namespace gru {

// ---------------------------------------------------------------------------------- image packing
struct TrainPackArgs {
    const float* w;
    float* img_f;
    float* wy;
    float* img_b;  // NULL: pack the forward images; else the backward image alone
    int N, F, L, onehot;
};

__device__ __forceinline__ int acc_row(int i, int hf) { return (i & 3) + 8 * (i >> 2) + 4 * hf; }

__global__ __launch_bounds__(256) void gru_train_pack_kernel(const TrainPackArgs a) {
    const int F = a.F, L = a.L, N = a.N;
    const int TT = 3 * F / 32, HT = F / 32, KG = F / 8, NG = L == 2 ? 3 : 1, KGB = 3 * F / 8;
    const TrainOff o = train_off(N, F, L, a.onehot);
    const float* mats[3] = {a.w + o.whh[0], a.w + o.wih[1], a.w + o.whh[1]};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t e0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.img_b) {
        const int gsz = HT * KGB * 256, nm = NG * gsz;
        for (int64_t e = e0; e < nm + HT * 32; e += stride) {
            float v;
            if (e < nm) {  // W^T[unit 32 t + (l & 31)][gate row hid_of(s, l >> 5)]
                const int g = (int)(e / gsz), r = (int)(e % gsz), t = r / (KGB * 256), r2 = r % (KGB * 256);
                const int s = 4 * (r2 >> 8) + (r2 & 3), l = (r2 >> 2) & 63;
                v = mats[g][(int64_t)hid_of(s, l >> 5) * F + 32 * t + (l & 31)];
            } else {
                const int r = (int)(e - nm);
                v = a.w[o.wlin + 32 * (r >> 5) + acc_row(r & 15, (r >> 4) & 1)];
            }
            a.img_b[e] = v;
        }
        return;
    }
    const int gsz = TT * KG * 256, nm = NG * gsz, nv = (4 * TT + 3 * HT) * 32;
    const int ng = N / 8, nwy = TT * ng * 256;
    const float* wih0 = a.w + o.wih[0];
    for (int64_t e = e0; e < (int64_t)nm + nv + nwy; e += stride) {
        if (e < nm) {  // fill_mats' order
            const int g = (int)(e / gsz), r = (int)(e % gsz), t = r / (KG * 256), r2 = r % (KG * 256);
            const int s = 4 * (r2 >> 8) + (r2 & 3), l = (r2 >> 2) & 63;
            a.img_f[e] = mats[g][(int64_t)(32 * t + (l & 31)) * F + hid_of(s, l >> 5)];
        } else if (e < nm + nv) {
            const int r = (int)(e - nm), v = r >> 5, rr = acc_row(r & 15, (r >> 4) & 1);
            float val = 0.0f;
            if (v < TT) {
                const int row = 32 * v + rr;
                val = a.w[o.bih[0] + row] + (row < 2 * F ? a.w[o.bhh[0] + row] : 0.0f);
            } else if (v < 2 * TT) {
                val = wih0[(int64_t)(32 * (v - TT) + rr) * o.Din + N];
            } else if (v < 3 * TT) {
                val = a.onehot ? wih0[(int64_t)(32 * (v - 2 * TT) + rr) * o.Din + N + 1] : 0.0f;
            } else if (v < 3 * TT + HT) {
                val = a.w[o.bhh[0] + 2 * F + 32 * (v - 3 * TT) + rr];
            } else if (v < 4 * TT + HT) {
                const int row = 32 * (v - 3 * TT - HT) + rr;
                if (L == 2) val = a.w[o.bih[1] + row] + (row < 2 * F ? a.w[o.bhh[1] + row] : 0.0f);
            } else if (v < 4 * TT + 2 * HT) {
                if (L == 2) val = a.w[o.bhh[1] + 2 * F + 32 * (v - 4 * TT - HT) + rr];
            } else {
                val = a.w[o.wlin + 32 * (v - 4 * TT - 2 * HT) + rr];
            }
            a.img_f[e] = val;
        } else {  // fill_wy's order
            const int r = (int)(e - nm - nv), t = r / (ng * 256), r2 = r % (ng * 256);
            const int s = 4 * (r2 >> 8) + (r2 & 3), l = (r2 >> 2) & 63;
            a.wy[r] = wih0[(int64_t)(32 * t + (l & 31)) * o.Din + s + (l >> 5) * (N / 2)];
        }
    }
}

// ---------------------------------------------------------------------------------- tiles in global memory
// A 32-unit tile j of one sample's F-vector at `p`, in accumulator layout: register i of lane half hf = unit
// 32 j + (i & 3) + 8 (i >> 2) + 4 hf, so registers 4q .. 4q + 3 are 16 contiguous bytes
__device__ __forceinline__ void store_tile(float* p, int j, int hf, const f16v& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f4*>(p + 32 * j + 8 * q + 4 * hf) = f4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
}
__device__ __forceinline__ f16v load_tile(const float* p, int j, int hf) {
    f16v v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f4 x = *reinterpret_cast<const f4*>(p + 32 * j + 8 * q + 4 * hf);
        v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
    }
    return v;
}
__device__ __forceinline__ f16v lds_vec(const float* smem, int off, int hf) {
    const f4* p = reinterpret_cast<const f4*>(smem + off + hf * 16);
    const f4 x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
    return f16v{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3],
                x2[0], x2[1], x2[2], x2[3], x3[0], x3[1], x3[2], x3[3]};
}

// PyTorch's GRU cell with the gates kept: r, z = sigmoid, n = tanh(a_in + r a_hn), h' = (h - n) z + n
__device__ __forceinline__ void train_update(f16v& h, const f16v& ar, const f16v& az, const f16v& ain, const f16v& ahn,
                                             f16v& r, f16v& z, f16v& n) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        r[i] = 1.0f / (1.0f + expf(-ar[i]));
        z[i] = 1.0f / (1.0f + expf(-az[i]));
        n[i] = tanhf(ain[i] + r[i] * ahn[i]);
        h[i] = (h[i] - n[i]) * z[i] + n[i];
    }
}

// ---------------------------------------------------------------------------------- forward
struct TrainFwdArgs {
    const float* img;
    const f4* wy;
    const float* w;   // flat weights (the Linear bias is read from it)
    const float* y;
    const float* gt;  // (B, N) in the step frame, or NULL (student forcing)
    float* out;       // (B, N) step frame: the logit where `writes` is set, else 1.0
    float* bits;      // (B, N) step frame: the value step ii hands to step ii + 1
    float* saved;
    int64_t B, blin_off;
    int N, onehot, student;
    uint32_t writes[kMaxWords];
};

template <int F, int L>
__global__ __launch_bounds__(64 * NPD_GRU_WPB) void gru_train_fwd_kernel(const TrainFwdArgs a) {
    using T = TGeo<F, L>;
    constexpr int TT = T::TT, HT = T::HT, KG = T::KG, WPB = NPD_GRU_WPB;
    extern __shared__ __attribute__((aligned(16))) f4 smem4[];
    const float* smem = reinterpret_cast<const float*>(smem4);
    {
        const f4* src = reinterpret_cast<const f4*>(a.img);
        for (int i = threadIdx.x; i < T::F_TOTAL / 4; i += blockDim.x) smem4[i] = src[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    const int N = a.N;
    const int64_t B = a.B, NBF = (int64_t)N * B * F;
    const int64_t ntiles = (B + 31) / 32;
    const float b_lin = a.w[a.blin_off];
    const f16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto vec = [&](int v) -> f16v { return lds_vec(smem, T::OFF_V + v * 32, half); };
    float* aux = a.saved + 5 * L * NBF;

    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < ntiles; tile += (int64_t)gridDim.x * WPB) {
        const int64_t cw = tile * 32 + col;
        const bool valid = cw < B;
        const int64_t cwc = valid ? cw : B - 1;  // loads only: an invalid lane stores nothing

        // P = W_ih0[:, :N] y + the layer-0 biases (constant over the steps)
        f16v P[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) P[t] = zero;
        {
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
#pragma unroll
        for (int t = 0; t < TT; ++t) P[t] += vec(T::V_B0 + t);

        f16v h0[HT], h1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            h0[t] = zero;
            h1[t] = zero;
        }
        float fed = 1.0f;  // step 0 is fed prev = +1

        for (int ii = 0; ii < N; ++ii) {
            // get_onehot (rnn_all.py:258-260): -1 and 0 -> column 0, +1 -> column 1; without onehot the raw value
            const float idx = fed > 0.0f ? 1.0f : 0.0f;
            const float xa = a.onehot ? 1.0f - idx : fed, xb = a.onehot ? idx : 0.0f;
            const int64_t smp = (int64_t)ii * B + cw;
            if (half == 0 && valid) {
                aux[smp * 3] = 1.0f;
                aux[smp * 3 + 1] = xa;
                aux[smp * 3 + 2] = xb;
            }
            // ================= layer 0
            {
                f16v arz[2 * HT], ain[HT], ahn[HT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) arz[t] = P[t] + xa * vec(T::V_XA + t) + xb * vec(T::V_XB + t);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    ain[j] = P[2 * HT + j] + xa * vec(T::V_XA + 2 * HT + j) + xb * vec(T::V_XB + 2 * HT + j);
                    ahn[j] = vec(T::V_HN0 + j);
                }
                gemm_chain<TT, KG, 2 * HT, HT>(smem4, 0, 0, lane, arz, h0);
                gemm_chain<TT, KG, HT, HT>(smem4, 0, 2 * HT, lane, ahn, h0);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    f16v r, z, n;
                    train_update(h0[j], arz[j], arz[HT + j], ain[j], ahn[j], r, z, n);
                    if (valid) {
                        float* p = a.saved + smp * F;
                        store_tile(p, j, half, h0[j]);
                        store_tile(p + NBF, j, half, r);
                        store_tile(p + 2 * NBF, j, half, z);
                        store_tile(p + 3 * NBF, j, half, n);
                        store_tile(p + 4 * NBF, j, half, ahn[j]);
                    }
                }
            }
            if constexpr (L == 2) {
                // ================= layer 1
                f16v arz[2 * HT], ain[HT], ahn[HT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) arz[t] = vec(T::V_B1 + t);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    ain[j] = vec(T::V_B1 + 2 * HT + j);
                    ahn[j] = vec(T::V_HN1 + j);
                }
                gemm_chain<TT, KG, 2 * HT, HT>(smem4, 1, 0, lane, arz, h0);
                gemm_chain<TT, KG, HT, HT>(smem4, 1, 2 * HT, lane, ain, h0);
                gemm_chain<TT, KG, 2 * HT, HT>(smem4, 2, 0, lane, arz, h1);
                gemm_chain<TT, KG, HT, HT>(smem4, 2, 2 * HT, lane, ahn, h1);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    f16v r, z, n;
                    train_update(h1[j], arz[j], arz[HT + j], ain[j], ahn[j], r, z, n);
                    if (valid) {
                        float* p = a.saved + 5 * NBF + smp * F;
                        store_tile(p, j, half, h1[j]);
                        store_tile(p + NBF, j, half, r);
                        store_tile(p + 2 * NBF, j, half, z);
                        store_tile(p + 3 * NBF, j, half, n);
                        store_tile(p + 4 * NBF, j, half, ahn[j]);
                    }
                }
            }
            // ================= Linear(F, 1) on the top layer
            float part = 0.0f;
#pragma unroll
            for (int j = 0; j < HT; ++j) {
                const f16v wl = vec(T::V_WL + j);
#pragma unroll
                for (int i = 0; i < 16; ++i) part = fmaf(wl[i], L == 2 ? h1[j][i] : h0[j][i], part);
            }
            const float out = part + __shfl_xor(part, 32, 64) + b_lin;
            const bool wr = (a.writes[ii >> 5] >> (ii & 31)) & 1u;
            const float dec = wr ? out : 1.0f;
            const float next = a.student ? sgnf(dec) : a.gt[cwc * N + ii];
            if (half == 0 && valid) {
                a.out[cw * N + ii] = dec;
                a.bits[cw * N + ii] = next;
            }
            fed = next;
        }
    }
}

// ---------------------------------------------------------------------------------- backward recurrence
struct TrainBwdArgs {
    const float* img;
    const float* gout;  // (B, N) step frame; 0 where the forward wrote no logit
    const float* saved;
    float* delta;       // scratch: L arrays [NB][4F]
    float* ge;          // scratch: [NB] grad_out, step-major
    int64_t B;
    int N;
};

template <int F, int L>
__global__ __launch_bounds__(64 * NPD_GRU_WPB) void gru_train_bwd_kernel(const TrainBwdArgs a) {
    using T = TGeo<F, L>;
    constexpr int TT = T::TT, HT = T::HT, KGB = T::KGB, WPB = NPD_GRU_WPB;
    extern __shared__ __attribute__((aligned(16))) f4 smem4[];
    const float* smem = reinterpret_cast<const float*>(smem4);
    {
        const f4* src = reinterpret_cast<const f4*>(a.img);
        for (int i = threadIdx.x; i < T::B_TOTAL / 4; i += blockDim.x) smem4[i] = src[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    const int N = a.N;
    const int64_t B = a.B, NBF = (int64_t)N * B * F;
    const int64_t ntiles = (B + 31) / 32;
    const f16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < ntiles; tile += (int64_t)gridDim.x * WPB) {
        const int64_t cw = tile * 32 + col;
        const bool valid = cw < B;
        // an invalid lane reads the last word's state but its grad_out is 0, so its column's dh and Delta are exactly
        // 0 throughout; MFMA columns do not mix, and it stores nothing
        const int64_t cwc = valid ? cw : B - 1;
        f16v dh[L][HT];
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
            for (int j = 0; j < HT; ++j) dh[l][j] = zero;

        for (int ii = N - 1; ii >= 0; --ii) {
            const int64_t smp = (int64_t)ii * B + cwc;
            const float g = valid ? a.gout[cwc * N + ii] : 0.0f;
            if (half == 0 && valid) a.ge[smp] = g;
#pragma unroll
            for (int j = 0; j < HT; ++j) dh[L - 1][j] += g * lds_vec(smem, T::B_OFF_WL + j * 32, half);
#pragma unroll
            for (int l = L - 1; l >= 0; --l) {
                f16v dhh[TT], dih[TT];  // [da_r, da_z, da_hn] and [da_r, da_z, da_in], HT tiles each
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    const float* p = a.saved + (int64_t)(5 * l) * NBF + smp * F;
                    const f16v r = load_tile(p + NBF, j, half), z = load_tile(p + 2 * NBF, j, half);
                    const f16v n = load_tile(p + 3 * NBF, j, half), ahn = load_tile(p + 4 * NBF, j, half);
                    const f16v hp = ii > 0 ? load_tile(p - B * F, j, half) : zero;
                    f16v dar, daz, dan, dahn;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float d = dh[l][j][i];
                        const float dn = d * (1.0f - z[i]);
                        const float dz = d * (hp[i] - n[i]);
                        dan[i] = dn * (1.0f - n[i] * n[i]);
                        dahn[i] = dan[i] * r[i];
                        dar[i] = dan[i] * ahn[i] * r[i] * (1.0f - r[i]);
                        daz[i] = dz * z[i] * (1.0f - z[i]);
                        dh[l][j][i] = d * z[i];
                    }
                    dhh[j] = dar; dhh[HT + j] = daz; dhh[2 * HT + j] = dahn;
                    dih[j] = dar; dih[HT + j] = daz; dih[2 * HT + j] = dan;
                    if (valid) {
                        float* q = a.delta + ((int64_t)l * N * B + smp) * (4 * F);
                        store_tile(q, j, half, dar);
                        store_tile(q + F, j, half, daz);
                        store_tile(q + 2 * F, j, half, dan);
                        store_tile(q + 3 * F, j, half, dahn);
                    }
                }
                // dh_prev = dh z + W_hh^T Delta_hh; layer 1 also hands W_ih1^T Delta_ih to layer 0's h' of this step
                gemm_chain<HT, KGB, HT, TT>(smem4, l == 0 ? 0 : 2, 0, lane, dh[l], dhh);
                if (l == 1) gemm_chain<HT, KGB, HT, TT>(smem4, 1, 0, lane, dh[0], dih);
            }
        }
    }
}

// ---------------------------------------------------------------------------------- weight-gradient contraction
// out (M x Nc) = sum over k < K of A[k][row(m)] Bm[k'][n]: row(m) = m, or (amapF > 0, the hidden-side rows [r, z, hn] of
// a [r, z, in, hn] Delta) m + amapF for m >= 2 amapF; k' = k, or k mod bmod (y, the same for every step)
struct TrainJob {
    const float* A;
    const float* Bm;
    int64_t K, bmod, out_off, part_off;
    int lda, ldb, M, Nc, amapF, ld_out;
};
struct TrainJobs {
    TrainJob j[kTrainMaxJobs];
    int n, P;
    int64_t total;  // floats per split
    float* part;
    float* gw;
};

__global__ __launch_bounds__(256) void gru_train_contract_kernel(const TrainJobs js) {
    const TrainJob& jb = js.j[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    int64_t chunk = (jb.K + js.P - 1) / js.P;
    chunk += chunk & 1;
    const int64_t k0 = (int64_t)blockIdx.x * chunk;
    const int64_t k1 = k0 + chunk < jb.K ? k0 + chunk : jb.K;
    const int nt = (jb.Nc + 31) / 32, tiles = ((jb.M + 31) / 32) * nt;
    float* part = js.part + (int64_t)blockIdx.x * js.total + jb.part_off;
    for (int tile = wave; tile < tiles; tile += 4) {
        const int m = 32 * (tile / nt) + col, n = 32 * (tile % nt) + col;
        const bool am_ok = m < jb.M, bn_ok = n < jb.Nc;
        const int am = jb.amapF > 0 && m >= 2 * jb.amapF ? m + jb.amapF : m;
        f16v acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int64_t kb = k0 + half;
        if (jb.bmod > 0) kb %= jb.bmod;
        for (int64_t k = k0 + half; k < k1 + half; k += 2) {  // every lane runs the same count; k >= k1 adds zeros
            const bool in = k < k1;
            const float av = am_ok && in ? jb.A[k * jb.lda + am] : 0.0f;
            const float bv = bn_ok && in ? jb.Bm[(jb.bmod > 0 ? kb : k) * jb.ldb + n] : 0.0f;
            acc = mfma(av, bv, acc);
            if (jb.bmod > 0) {
                kb += 2;  // bmod >= 1: at most two wraps
                if (kb >= jb.bmod) kb -= jb.bmod;
                if (kb >= jb.bmod) kb -= jb.bmod;
            }
        }
        if (bn_ok) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = 32 * (tile / nt) + acc_row(i, half);
                if (row < jb.M) part[(int64_t)row * jb.Nc + n] = acc[i];
            }
        }
    }
}

__global__ __launch_bounds__(256) void gru_train_reduce_kernel(const TrainJobs js) {
    const TrainJob& jb = js.j[blockIdx.y];
    const int cnt = jb.M * jb.Nc;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += gridDim.x * blockDim.x) {
        float s = 0.0f;
        for (int p = 0; p < js.P; ++p) s += js.part[(int64_t)p * js.total + jb.part_off + e];
        js.gw[jb.out_off + (int64_t)(e / jb.Nc) * jb.ld_out + e % jb.Nc] = s;
    }
}

static int train_grid(int64_t B) {
    return grid_for(((B + 31) / 32 + NPD_GRU_WPB - 1) / NPD_GRU_WPB, 1, device_cu_count());
}

static int pack(const npd_gru_train* g, const float* w, bool backward, hipStream_t s) {
    TrainPackArgs pa{w, g->img_f, g->wy, backward ? g->img_b : nullptr, g->N, g->F, g->layers, g->onehot};
    hipLaunchKernelGGL(gru_train_pack_kernel, dim3(64), dim3(256), 0, s, pa);
    return launch_check("gru_train_pack_kernel launch");
}

}  // namespace gru
}  // namespace npd

using namespace npd;

// ---------------------------------------------------------------------------------- C ABI
static bool train_shape_ok(int N, int F, int layers) {
    return N >= 8 && N <= kMaxN && N % 8 == 0 && (F == 32 || F == 64) && (layers == 1 || layers == 2);
}

extern "C" int npd_gru_train_create(int N, int F, int layers, int onehot, npd_gru_train** out) {
    NPD_ARG(out != nullptr, "npd_gru_train_create: out is NULL");
    *out = nullptr;
    NPD_ARG(N >= 8 && N <= kMaxN && N % 8 == 0, "npd_gru_train_create: N must be a multiple of 8 in [8, 256]");
    NPD_ARG(F == 32 || F == 64, "npd_gru_train_create: hidden size F must be 32 or 64 (128 .. 512 are a follow-up)");
    NPD_ARG(layers == 1 || layers == 2, "npd_gru_train_create: 1 or 2 layers supported");
    NPD_ARG(onehot == 0 || onehot == 1, "npd_gru_train_create: onehot must be 0 or 1");
    npd_gru_train* g = new (std::nothrow) npd_gru_train{};
    if (!g) return fail(NPD_ENOMEM, "npd_gru_train_create: out of memory");
    g->N = N; g->F = F; g->layers = layers; g->onehot = onehot;
    hipError_t e = hipGetDevice(&g->device);
    if (e == hipSuccess) e = hipMalloc(&g->img_f, gru::train_fwd_image_floats(F, layers) * 4);
    if (e == hipSuccess) e = hipMalloc(&g->wy, gru::train_wy_floats(N, F) * 4);
    if (e == hipSuccess) e = hipMalloc(&g->img_b, gru::train_bwd_image_floats(F, layers) * 4);
    if (e != hipSuccess) {
        npd_gru_train_destroy(g);
        return hip_fail(e, "npd_gru_train_create");
    }
    *out = g;
    return NPD_OK;
}

extern "C" int npd_gru_train_destroy(npd_gru_train* g) {
    NPD_ARG(g != nullptr, "npd_gru_train_destroy: handle is NULL");
    for (float* p : {g->img_f, g->wy, g->img_b})
        if (p) (void)hipFree(p);
    delete g;
    return NPD_OK;
}

extern "C" int npd_gru_train_workspace(const npd_gru_train* g, int64_t B, int64_t* saved_floats, int64_t* scratch_floats) {
    NPD_ARG(g != nullptr, "npd_gru_train_workspace: handle is NULL");
    NPD_ARG(saved_floats != nullptr && scratch_floats != nullptr, "npd_gru_train_workspace: an output is NULL");
    NPD_ARG(B >= 0 && B <= ((int64_t)1 << 31), "npd_gru_train_workspace: B must be in [0, 2^31]");
    *saved_floats = gru::train_saved_floats(g->N, g->F, g->layers, B);
    *scratch_floats = gru::train_scratch_floats(g->N, g->F, g->layers, g->onehot, B);
    return NPD_OK;
}

extern "C" int npd_gru_train_forward(npd_gru_train* g, const float* weights_dev, const float* y, const float* gt_or_null,
                                     const uint8_t* writes_logit, int student, float* out, float* bits, float* saved,
                                     int64_t B, void* stream) {
    NPD_ARG(g != nullptr, "npd_gru_train_forward: handle is NULL");
    NPD_ARG(weights_dev && y && writes_logit && out && bits && saved, "npd_gru_train_forward: an operand is NULL");
    NPD_ARG(student == 0 || student == 1, "npd_gru_train_forward: student must be 0 or 1");
    NPD_ARG(student || gt_or_null, "npd_gru_train_forward: teacher forcing needs gt");
    NPD_ARG(B >= 0 && B <= ((int64_t)1 << 31), "npd_gru_train_forward: B must be in [0, 2^31]");
    NPD_ARG(((uintptr_t)y | (uintptr_t)saved) % 16 == 0, "npd_gru_train_forward: y and saved must be 16-byte aligned");
    NPD_ARG(train_shape_ok(g->N, g->F, g->layers), "npd_gru_train_forward: bad handle");
    if (B == 0) return NPD_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc = gru::pack(g, weights_dev, false, s);
    if (rc != NPD_OK) return rc;
    gru::TrainFwdArgs a{};
    a.img = g->img_f; a.wy = reinterpret_cast<const gru::f4*>(g->wy); a.w = weights_dev; a.y = y; a.gt = gt_or_null;
    a.out = out; a.bits = bits; a.saved = saved; a.B = B;
    a.blin_off = gru::train_off(g->N, g->F, g->layers, g->onehot).blin;
    a.N = g->N; a.onehot = g->onehot; a.student = student;
    gru::info_mask(writes_logit, g->N, a.writes);
    const int grid = gru::train_grid(B);
    return gru::dispatch(gru::NarrowShapes{}, [&](auto f, auto l) {
        return gru::launch_lds<gru::gru_train_fwd_kernel<f.value, l.value>>(
            "gru_train_fwd_kernel launch", grid, 64 * NPD_GRU_WPB, (size_t)gru::TGeo<f.value, l.value>::F_TOTAL * 4, s, a);
    }, g->F, g->layers);
}

extern "C" int npd_gru_train_backward(npd_gru_train* g, const float* weights_dev, const float* y, const float* grad_out,
                                      const float* saved, float* scratch, float* grad_weights_dev, int64_t B,
                                      void* stream) {
    NPD_ARG(g != nullptr, "npd_gru_train_backward: handle is NULL");
    NPD_ARG(weights_dev && y && grad_out && saved && scratch && grad_weights_dev,
            "npd_gru_train_backward: an operand is NULL");
    NPD_ARG(B >= 0 && B <= ((int64_t)1 << 31), "npd_gru_train_backward: B must be in [0, 2^31]");
    NPD_ARG(((uintptr_t)saved | (uintptr_t)scratch) % 16 == 0,
            "npd_gru_train_backward: saved and scratch must be 16-byte aligned");
    NPD_ARG(train_shape_ok(g->N, g->F, g->layers), "npd_gru_train_backward: bad handle");
    hipStream_t s = (hipStream_t)stream;
    const int N = g->N, F = g->F, L = g->layers;
    const gru::TrainOff o = gru::train_off(N, F, L, g->onehot);
    if (B == 0) {  // no sample: every gradient is zero
        NPD_HIP(hipMemsetAsync(grad_weights_dev, 0, o.total * 4, s));
        return NPD_OK;
    }
    int rc = gru::pack(g, weights_dev, true, s);
    if (rc != NPD_OK) return rc;
    const int64_t NB = (int64_t)N * B, NBF = NB * F;
    float* delta = scratch;
    float* ge = scratch + NB * 4 * F * L;
    gru::TrainBwdArgs a{g->img_b, grad_out, saved, delta, ge, B, N};
    const int grid = gru::train_grid(B);
    rc = gru::dispatch(gru::NarrowShapes{}, [&](auto f, auto l) {
        return gru::launch_lds<gru::gru_train_bwd_kernel<f.value, l.value>>(
            "gru_train_bwd_kernel launch", grid, 64 * NPD_GRU_WPB, (size_t)gru::TGeo<f.value, l.value>::B_TOTAL * 4, s, a);
    }, F, L);
    if (rc != NPD_OK) return rc;

    gru::TrainJobs js{};
    js.P = gru::train_splits(NB);
    js.total = o.total;
    js.part = ge + NB;
    js.gw = grad_weights_dev;
    const float* aux = saved + 5 * L * NBF;
    int64_t poff = 0;
    auto add = [&](const float* A, int lda, int M, int amapF, const float* Bm, int ldb, int Nc, int64_t bmod, int64_t K,
                   int64_t out_off, int ld_out) {
        gru::TrainJob& j = js.j[js.n++];
        j.A = A; j.Bm = Bm; j.K = K; j.bmod = bmod; j.out_off = out_off; j.part_off = poff;
        j.lda = lda; j.ldb = ldb; j.M = M; j.Nc = Nc; j.amapF = amapF; j.ld_out = ld_out;
        poff += (int64_t)M * Nc;
    };
    for (int l = 0; l < L; ++l) {
        const float* D = delta + (int64_t)l * NB * 4 * F;
        const float* H = saved + (int64_t)(5 * l) * NBF;
        if (l == 0) {
            add(D, 4 * F, 3 * F, 0, y, N, N, B, NB, o.wih[0], o.Din);                            // dW_ih0[:, :N]
            add(D, 4 * F, 3 * F, 0, aux + 1, 3, g->onehot ? 2 : 1, 0, NB, o.wih[0] + N, o.Din);  // its bit column(s)
        } else {
            add(D, 4 * F, 3 * F, 0, saved, F, F, 0, NB, o.wih[1], F);                            // dW_ih1 = D_ih1 (x) h0'
        }
        add(D + B * 4 * F, 4 * F, 3 * F, F, H, F, F, 0, NB - B, o.whh[l], F);                    // dW_hh = D_hh (x) h_prev
        add(D, 4 * F, 3 * F, 0, aux, 3, 1, 0, NB, o.bih[l], 1);
        add(D, 4 * F, 3 * F, F, aux, 3, 1, 0, NB, o.bhh[l], 1);
    }
    add(ge, 1, 1, 0, saved + (int64_t)(5 * (L - 1)) * NBF, F, F, 0, NB, o.wlin, F);
    add(ge, 1, 1, 0, aux, 3, 1, 0, NB, o.blin, 1);
    if (poff != o.total) return fail(NPD_EINVAL, "npd_gru_train_backward: internal job table mismatch");
    hipLaunchKernelGGL(gru::gru_train_contract_kernel, dim3(js.P, js.n), dim3(256), 0, s, js);
    rc = launch_check("gru_train_contract_kernel launch");
    if (rc != NPD_OK) return rc;
    hipLaunchKernelGGL(gru::gru_train_reduce_kernel, dim3(16, js.n), dim3(256), 0, s, js);
    return launch_check("gru_train_reduce_kernel launch");
}

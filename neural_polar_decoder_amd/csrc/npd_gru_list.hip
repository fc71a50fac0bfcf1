// npd_gru_list.hip -- CRISP GRU list decoder (RNN_decoder.list_decode, y_input).
//
// Reference: rnn_all.py:563-664.  L partial decodings per received word stay alive; every live path runs one GRU step
// per position, forks at an information position into sign(out) (metric unchanged) and -sign(out) (metric + |out|),
// pruneLists keeps torch.topk(-metric, L) in ascending child order, and the survivor whose re-encoded word is nearest
// to y (first minimum) is the answer.  Frozen positions only advance the state: bit +1, no metric penalty.
//
// MI355X design: gru_decode_kernel's step (npd_gru.hip: weights in LDS, 4 waves, v_mfma_f32_32x32x2_f32, the state
// tiles are the next step's B operands) with another column map.  With Lp = L rounded up to 1, 2, 4 or 8, a wave's 32
// MFMA columns are 32 / Lp codewords x Lp path slots, column = cw * Lp + slot; Lp = 1 is gru_decode_kernel's map.
// Each column carries its path's metric and its N bits as bit words (1 = the bit is -1).
//
// While the list fills (2 ls <= L) slot s holds a copy of path s mod ls: all slots of a codeword start from the same
// y and zero state, so the copies are bit-identical and a fork only flips the bit of the slots whose new path index
// (s mod 2 ls) is >= ls: nothing moves.  Once 2 ls > L every information step chooses L of the 2 ls children
// (rank counting; npd_nth.hpp's statement of torch.topk when a tie straddles the L-th place), compacts them in
// ascending child index and gathers state, bits and metric from the parent column with ds_bpermute_b32 inside the
// lane half; the gather is skipped when no lane of the wave moves.
//
// This file also owns the C entry points of both list kernels; hidden 256 / 512 handles go to gru_wide_list_kernel
// (npd_gru_wide_list.hip: the same column map and procedure on the weight-streaming step).  npd_gru_list_decode_crc
// and npd_gru_list_decode_crc_mc run the CA instantiations: the same step loop, list_finish<true> as the epilogue.
#include <stdlib.h>
#include <string.h>

#include "npd_gru_list.hpp"

namespace npd {
namespace gru {

// CA: list_finish's CRC-aided / counting epilogue (npd_gru_list.hpp); the step loop is the same text in both
template <int F, int L, bool CA>
__global__ __launch_bounds__(64 * NPD_GRU_WPB) void gru_list_kernel(const ListArgs a) {
    constexpr int WPB = NPD_GRU_WPB;
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
    const int lpl = a.lp_log2, Lp = 1 << lpl;
    const int slot = col & (Lp - 1);
    const int base = lane - slot;  // this codeword's slot 0, in this lane half
    const int cpt = 32 >> lpl;     // codewords per wave tile
    const uint32_t gmask = (1u << Lp) - 1u;
    const int64_t ntiles = (a.B + cpt - 1) / cpt;
    const f16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto cvec = [&](int off) -> f16v {
        const f4* p = reinterpret_cast<const f4*>(smem + off + half * 16);
        const f4 x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
        return f16v{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3],
                    x2[0], x2[1], x2[2], x2[3], x3[0], x3[1], x3[2], x3[3]};
    };

    [[maybe_unused]] unsigned long long cnt[3] = {0ull, 0ull, 0ull};  // CA: this wave's error counts (wave-uniform)

    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < ntiles; tile += (int64_t)gridDim.x * WPB) {
        const int64_t cw = tile * cpt + (col >> lpl);
        const bool valid = cw < a.B;
        const int64_t cwc = valid ? cw : a.B - 1;

        // ---- P = W_ih0[:, :N] . Fy, once per column (the slots of a codeword compute the same P)
        f16v P[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) P[t] = zero;
        {
            const f4* yr = reinterpret_cast<const f4*>(a.fy + cwc * N + half * (N / 2));
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
        float xb = 1.0f;   // x_i of this path: onehot index of its previous bit (or its sign); +1 at step 0 / after frozen
        float met = 0.0f;  // path metric
        uint32_t bw[kMaxWords];  // the path's bits, bit i of word i / 32 set = position i decided -1
#pragma unroll
        for (int w = 0; w < kMaxWords; ++w) bw[w] = 0u;
        int ls = 1;  // live list size (the same for every codeword)

        for (int ii = 0; ii < N; ++ii) {
            const float xbe = half ? xb : 1.0f;  // extra k-step B operand: [1, x_i]
            // ================= layer 0 (as gru_decode_kernel)
            {
                f16v acc[TT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) acc[t] = P[t];
#pragma unroll
                for (int t = 2 * HT; t < TT; ++t) acc[t] = cvec(G::OFF_CV + (t - 2 * HT) * 32);
                gemm_chain<TT, KG, TT, HT>(smem4, 0, 0, lane, acc, h0);
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) acc[t] = mfma(smem[G::OFF_X + t * 64 + lane], xbe, acc[t]);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    const f16v ain = mfma(smem[G::OFF_IN + j * 64 + lane], xbe, P[2 * HT + j]);
                    gru_update<true>(h0[j], acc[j], acc[HT + j], ain, acc[2 * HT + j]);
                }
            }
            if constexpr (L == 2) {
                // ================= layer 1
                f16v acc1[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc1[t] = cvec(G::OFF_CV + (HT + t) * 32);
                gemm_chain<TT, KG, TT, HT>(smem4, 1, 0, lane, acc1, h0);
                f16v arz[2 * HT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) arz[t] = acc1[t];
                gemm_chain<TT, KG, 2 * HT, HT>(smem4, 2, 0, lane, arz, h1);
                f16v ahn[HT];
#pragma unroll
                for (int j = 0; j < HT; ++j) ahn[j] = cvec(G::OFF_CV + (HT + TT + j) * 32);
                gemm_chain<TT, KG, HT, HT>(smem4, 2, 2 * HT, lane, ahn, h1);
#pragma unroll
                for (int j = 0; j < HT; ++j) gru_update<true>(h1[j], arz[j], arz[HT + j], acc1[2 * HT + j], ahn[j]);
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
            const float out = part + __shfl_xor(part, 32, 64) + a.b_lin;

            const bool info = (a.info[ii >> 5] >> (ii & 31)) & 1u;
            if (!info) {  // frozen: only the state advances; the bit stays +1
                xb = 1.0f;
                continue;
            }
            // ================= information position: fork, prune, gather
            const float ao = fabsf(out);
            uint32_t neg = out < 0.0f ? 1u : 0u;  // the kept child's bit is sign(out) (an exact 0 counts as +1)
            bool flip;
            if (2 * ls <= a.L) {
                // filling: slot s already holds its parent (path s mod ls); its new path index is s mod 2 ls
                flip = (slot & (2 * ls - 1)) >= ls;
                if (flip) met += ao;
                ls *= 2;
            } else {
                // metric and bit always come from the parent; state and bit words only when some lane of the wave moves
                const int src = list_prune(met, neg, flip, ao, ls, a.L, lane, slot, base, gmask);
                if (__ballot(src != lane) != 0ull) {
#pragma unroll
                    for (int t = 0; t < HT; ++t)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            h0[t][i] = __shfl(h0[t][i], src, 64);
                            if constexpr (L == 2) h1[t][i] = __shfl(h1[t][i], src, 64);
                        }
#pragma unroll
                    for (int w = 0; w < kMaxWords; ++w)
                        if (32 * w < N) bw[w] = (uint32_t)__shfl((int)bw[w], src, 64);
                }
                ls = a.L;
            }
            neg ^= flip ? 1u : 0u;
#pragma unroll
            for (int w = 0; w < kMaxWords; ++w) bw[w] |= (w == (ii >> 5)) ? (neg << (ii & 31)) : 0u;
            xb = a.onehot ? (neg ? 0.0f : 1.0f) : (neg ? -1.0f : 1.0f);
        }

        // ================= epilogue: encode every path, distance to y, first minimum over the live slots
        if constexpr (CA)
            list_finish<true>(a, bw, met, ls, cw, cwc, valid, half, slot, base, cnt);
        else
            list_finish(a, bw, met, ls, cw, cwc, valid, half, slot, base);
    }
    if constexpr (CA) list_count_flush(a, cnt, lane);
}

template <int F, int L, bool CA>
static int launch_list(const ListArgs& a, hipStream_t s) {
    using G = Geo<F, L>;
    constexpr int WPB = NPD_GRU_WPB;
    auto kern = gru_list_kernel<F, L, CA>;
    const size_t lds = (size_t)G::TOTAL * 4;
    static bool attr = false;
    if (!attr) {
        NPD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
        attr = true;
    }
    const int cpt = 32 >> a.lp_log2;
    const int64_t tiles = (a.B + cpt - 1) / cpt;
    const int64_t wgs = (tiles + WPB - 1) / WPB;
    const int grid = grid_for(wgs, 1, device_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WPB), lds, s, a);
    return launch_check("gru_list_kernel launch");
}

}  // namespace gru
}  // namespace npd

using namespace npd;

// the handles the list kernels cover: fp32 GRU cells with a plain Linear head, on the LDS-resident kernel (F 32 or 64)
// or the weight-streaming one (F 256 or 512; F = 128 is not instantiated)
static bool list_handle_ok(const npd_gru* g) {
    return g->cell == 0 && g->precision == 0 && (g->F == 32 || g->F == 64 || g->F == 256 || g->F == 512) && g->ln == 0 &&
           g->hd == nullptr;
}

extern "C" int npd_gru_list_supported(const npd_gru* gru, const npd_code* code, int list_size) {
    NPD_ARG(gru != nullptr && code != nullptr, "npd_gru_list_supported: NULL handle");
    return (list_handle_ok(gru) && code->p.N == gru->N && list_size >= 1 && list_size <= 8) ? 1 : 0;
}

// The checks, the argument block and the launch that the three entry points share.  `a` arrives with the caller's output
// pointers, polynomial and counting fields; need_out: at least one of msg_hat and cand_msg must be given (the counting
// entry point needs neither).  ca: the CRC-aided / counting instantiations.
static int list_run(const char* who, const npd_gru* g, const npd_code* code, const float* y, const float* fy,
                    int list_size, gru::ListArgs a, bool need_out, bool ca, int64_t B, void* stream) {
    const std::string w(who);
    NPD_ARG(g != nullptr, w + ": gru is NULL");
    NPD_ARG(code != nullptr, w + ": code is NULL");
    NPD_ARG(B >= 0, w + ": B < 0");
    NPD_ARG(list_size >= 1 && list_size <= 8, w + ": list_size must be 1 .. 8");
    NPD_ARG(code->p.N == g->N, w + ": the code's N differs from the GRU handle's");
    if (a.crc_poly != 0u) {
        a.crc_c = crc_degree(a.crc_poly, code->p.K);
        NPD_ARG(a.crc_c > 0, w + ": crc_poly needs degree 1 .. 24 below K and bit 0 set");
    }
    if (!list_handle_ok(g))
        return fail(NPD_ENOTSUP, w + ": list decoding runs on the fp32 GRU kernels (GRU cell, precision 0, "
                                     "F 32, 64, 256 or 512, plain Linear head)");
    if (B == 0) return NPD_OK;
    NPD_ARG(!need_out || a.msg_hat != nullptr || a.cand_msg != nullptr, w + ": msg_hat and cand_msg both NULL");
    NPD_ARG(y != nullptr, w + ": y is NULL");
    if (fy == nullptr) fy = y;
    NPD_ARG(((uintptr_t)y & 15) == 0 && ((uintptr_t)fy & 15) == 0, w + ": y and fy must be 16-byte aligned");
    NPD_ARG(B <= (int64_t)1 << 40, w + ": B too large");
    a.img = g->img;
    a.wy = reinterpret_cast<const gru::f4*>(g->wy);
    a.y = y;
    a.fy = fy;
    a.B = B;
    a.N = g->N;
    a.K = code->p.K;
    a.L = list_size;
    a.lp_log2 = list_size <= 1 ? 0 : list_size <= 2 ? 1 : list_size <= 4 ? 2 : 3;
    a.onehot = g->onehot;
    a.pac = code->p.pac;
    a.b_lin = g->b_lin;
    a.tapmask = code->p.tapmask;
    a.smask = code->p.smask;
    for (int w2 = 0; w2 < kMaxWords; ++w2) a.info[w2] = 0;
    for (int i = 0; i < g->N; ++i)
        if (!((code->p.frozen[i >> 5] >> (i & 31)) & 1u)) a.info[i >> 5] |= 1u << (i & 31);
    hipStream_t s = (hipStream_t)stream;
    if (g->F > 64) return gru::launch_wide_list(g, a, ca, s);
    if (ca)
        return gru::dispatch(gru::NarrowShapes{},
                             [&](auto f, auto l) { return gru::launch_list<f.value, l.value, true>(a, s); }, g->F,
                             g->layers);
    return gru::dispatch(gru::NarrowShapes{},
                         [&](auto f, auto l) { return gru::launch_list<f.value, l.value, false>(a, s); }, g->F, g->layers);
}

extern "C" int npd_gru_list_decode(const npd_gru* g, const npd_code* code, const float* y, const float* fy,
                                   int list_size, float* msg_hat, int32_t* sel, float* cand_msg, float* cand_metric,
                                   int64_t B, void* stream) {
    gru::ListArgs a{};
    a.msg_hat = msg_hat;
    a.sel = sel;
    a.cand_msg = cand_msg;
    a.cand_metric = cand_metric;
    return list_run("npd_gru_list_decode", g, code, y, fy, list_size, a, true, false, B, stream);
}

extern "C" int npd_gru_list_decode_crc(const npd_gru* g, const npd_code* code, const float* y, const float* fy,
                                       int list_size, uint32_t crc_poly, float* msg_hat, int32_t* sel, int32_t* crc_ok,
                                       float* cand_msg, float* cand_metric, int32_t* cand_crc, int64_t B, void* stream) {
    NPD_ARG(crc_poly != 0u, "npd_gru_list_decode_crc: crc_poly needs degree 1 .. 24 below K and bit 0 set");
    gru::ListArgs a{};
    a.msg_hat = msg_hat;
    a.sel = sel;
    a.crc_ok = crc_ok;
    a.cand_msg = cand_msg;
    a.cand_metric = cand_metric;
    a.cand_crc = cand_crc;
    a.crc_poly = crc_poly;
    return list_run("npd_gru_list_decode_crc", g, code, y, fy, list_size, a, true, true, B, stream);
}

extern "C" int npd_gru_list_decode_crc_mc(const npd_gru* g, const npd_code* code, const float* y, const float* fy,
                                          int list_size, uint32_t crc_poly, float* msg_hat, uint64_t seed,
                                          uint64_t cw_offset, int64_t B, unsigned long long* counters, void* stream) {
    NPD_ARG(counters != nullptr, "npd_gru_list_decode_crc_mc: counters is NULL");
    gru::ListArgs a{};
    a.msg_hat = msg_hat;
    a.counters = counters;
    a.seed = seed;
    a.cw_offset = cw_offset;
    a.crc_poly = crc_poly;  // 0: plain selection, counted over all K bits
    return list_run("npd_gru_list_decode_crc_mc", g, code, y, fy, list_size, a, false, true, B, stream);
}

// npd_gru_list.hpp -- what the two GRU list kernels share (npd_gru_list.hip: gru_list_kernel, weights in LDS, F <= 64;
// npd_gru_wide_list.hip: gru_wide_list_kernel, weights streamed, F = 256 / 512): the launch arguments, the pruning
// order and the tie rule.  npd_gru_list.hip owns the C entry points and dispatches to launch_wide_list.
#pragma once

#include "npd_gru_host.hpp"
#include "npd_nth.hpp"

namespace npd {
namespace gru {

struct ListArgs {
    const float* img;
    const f4* wy;
    const float* y;    // (B, N) received words: final selection
    const float* fy;   // (B, N) GRU input
    float* msg_hat;    // (B, K) or NULL
    int32_t* sel;      // (B) or NULL
    float* cand_msg;   // (B, L, K) or NULL
    float* cand_metric;  // (B, L) or NULL
    int64_t B;
    int N, K, L, lp_log2;
    int onehot, pac;
    float b_lin;
    uint32_t tapmask, smask;
    uint32_t info[kMaxWords];
};

typedef float f8v __attribute__((ext_vector_type(8)));

// metric x beats metric y in pruneLists: torch.topk(-metric) with NaN as the largest value (nth::comp on the negated metrics)
__device__ __forceinline__ bool beats(float x, float y) { return (x != x && y == y) || (x < y); }

// survivors when a tie straddles the L-th place (rare): the reference's exact rule on the list order
// [keep_0 .. keep_{s-1}, flip_0 .. flip_{s-1}].  Vectors by value (VGPRs), the queue lives on this function's stack.
static __device__ __noinline__ uint32_t list_exact_mask(f8v km, f8v fm, int s, int L) {
    float v[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        v[t] = 0.0f;
        v[8 + t] = 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (t < s) {
            v[t] = -1.0f * km[t];
            v[s + t] = -1.0f * fm[t];
        }
    return nth::prune_mask(v, 2 * s, L);
}

// pruneLists for one codeword's slot group (2 ls > L): of the 2 ls children in list order -- c < ls keeps slot c's bit and
// metric, c >= ls flips slot c - ls's and adds ao = |out| -- the L that torch.topk(-metric) keeps, compacted in ascending
// child index.  Rank counting; list_exact_mask when a class of equivalent metrics straddles the L-th place.  Sets this
// slot's metric, kept-child bit `neg` (the parent's) and `flip`; returns the parent's lane (the lane itself for a dead
// slot).  slot = the lane's slot, base = the lane of the codeword's slot 0 in this lane half, gmask = (1 << Lp) - 1.
__device__ __forceinline__ int list_prune(float& met, uint32_t& neg, bool& flip, float ao, int ls, int L, int lane,
                                          int slot, int base, uint32_t gmask) {
    const float mk = met, mf = met + ao;
    f8v km, fm;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int sl = base + (t < ls ? t : 0);
        km[t] = __shfl(mk, sl, 64);
        fm[t] = __shfl(mf, sl, 64);
    }
    // rank counting for this slot's two children: nb candidates beat it, ne are equivalent (itself too)
    int nbk = 0, nek = 0, nbf = 0, nef = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < ls) {
            const bool b1 = beats(km[t], mk), e1 = !b1 && !beats(mk, km[t]);
            const bool b2 = beats(fm[t], mk), e2 = !b2 && !beats(mk, fm[t]);
            const bool b3 = beats(km[t], mf), e3 = !b3 && !beats(mf, km[t]);
            const bool b4 = beats(fm[t], mf), e4 = !b4 && !beats(mf, fm[t]);
            nbk += (int)b1 + (int)b2;
            nek += (int)e1 + (int)e2;
            nbf += (int)b3 + (int)b4;
            nef += (int)e3 + (int)e4;
        }
    }
    const bool mine = slot < ls;
    const bool sk = mine && nbk < L, sf = mine && nbf < L;
    // a class of equivalent metrics straddles the L-th place: the top-L set is not unique
    const bool amb = (sk && nbk + nek > L) || (sf && nbf + nef > L);
    const uint64_t bk = __ballot(sk), bf = __ballot(sf), ba = __ballot(amb);
    uint32_t mask = ((uint32_t)(bk >> base) & gmask) | (((uint32_t)(bf >> base) & gmask) << ls);
    if (((uint32_t)(ba >> base) & gmask) != 0u) mask = list_exact_mask(km, fm, ls, L);
    // slot j takes the j-th survivor in ascending child index
    int child = -1, cnt = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int bit = (int)((mask >> c) & 1u);
        if (bit && cnt == slot) child = c;
        cnt += bit;
    }
    const bool live = slot < L && child >= 0;
    flip = live && child >= ls;
    const int src = live ? base + (flip ? child - ls : child) : lane;
    const float pk = __shfl(mk, src, 64), pf = __shfl(mf, src, 64);
    met = flip ? pf : pk;
    neg = (uint32_t)__shfl((int)neg, src, 64);
    return src;
}

// The end of list_decode for one wave's columns: encode every path (bw: its bit words), fp32 distance to y, first
// minimum over the codeword's ls live slots, and the optional outputs (lane half 0 of the valid columns stores).
__device__ __forceinline__ void list_finish(const ListArgs& a, const uint32_t (&bw)[kMaxWords], float met, int ls,
                                            int64_t cw, int64_t cwc, bool valid, int half, int slot, int base) {
    const int N = a.N;
    uint32_t cd[kMaxWords];
#pragma unroll
    for (int w = 0; w < kMaxWords; ++w) cd[w] = bw[w];
    if (a.pac) {
        // rate-1 convolution (encode_kernel, npd_gen.hip): u_i = v_i xor parity(state & taps), state <- v
        uint32_t st = 0;
#pragma unroll
        for (int w = 0; w < kMaxWords; ++w)
            if (32 * w < N) {
                const uint32_t vin = bw[w];
                uint32_t uo = 0u;
                for (int b = 0; b < 32; ++b) {
                    const uint32_t vi = (vin >> b) & 1u;
                    uo |= (vi ^ ((uint32_t)__builtin_popcount(st & a.tapmask) & 1u)) << b;
                    st = ((st << 1) | vi) & a.smask;
                }
                const int rem = N - 32 * w;
                cd[w] = rem >= 32 ? uo : (uo & ((1u << rem) - 1u));
            }
    }
    // Plotkin butterfly over GF(2): x_i ^= x_{i+h} where bit h of i is clear (words past N are zero)
    {
        constexpr uint32_t km[5] = {0x55555555u, 0x33333333u, 0x0F0F0F0Fu, 0x00FF00FFu, 0x0000FFFFu};
#pragma unroll
        for (int s = 0; s < 5; ++s)
#pragma unroll
            for (int w = 0; w < kMaxWords; ++w) cd[w] ^= (cd[w] >> (1 << s)) & km[s];
#pragma unroll
        for (int hw = 1; hw < kMaxWords; hw <<= 1)
#pragma unroll
            for (int w = 0; w < kMaxWords; ++w)
                if ((w & hw) == 0) cd[w] ^= cd[w + hw];
    }
    // fp32 distance: each lane half sums 16 positions of every word
    float ds = 0.0f;
    {
        const float* yrow = a.y + cwc * N;
#pragma unroll
        for (int w = 0; w < kMaxWords; ++w)
            if (32 * w < N) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i0 = 32 * w + 16 * half + 4 * q;
                    if (i0 < N) {
                        const f4 yv = *reinterpret_cast<const f4*>(yrow + i0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float c = ((cd[w] >> (16 * half + 4 * q + e)) & 1u) ? -1.0f : 1.0f;
                            const float d = c - yv[e];
                            ds = fmaf(d, d, ds);
                        }
                    }
                }
            }
    }
    const float dist = ds + __shfl_xor(ds, 32, 64);
    float best = 0.0f;
    int bsel = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float dt = __shfl(dist, base + (t < ls ? t : 0), 64);
        if (t == 0 || (t < ls && dt < best)) {
            best = t == 0 ? dt : (dt < best ? dt : best);
            bsel = t;
        }
    }
    if (half == 0 && valid && slot < a.L) {
        const bool alive = slot < ls;
        const bool chosen = slot == bsel;
        if (a.cand_metric) a.cand_metric[cw * a.L + slot] = alive ? met : __builtin_inff();
        if (a.sel && chosen) a.sel[cw] = bsel;
        float* cm = a.cand_msg ? a.cand_msg + (cw * a.L + slot) * (int64_t)a.K : nullptr;
        float* mh = (a.msg_hat && chosen) ? a.msg_hat + cw * (int64_t)a.K : nullptr;
        int k = 0;
#pragma unroll
        for (int w = 0; w < kMaxWords; ++w)
            if (32 * w < N) {
                const uint32_t iw = a.info[w], vw = bw[w];
                for (int b = 0; b < 32; ++b)
                    if ((iw >> b) & 1u) {
                        const float v = ((vw >> b) & 1u) ? -1.0f : 1.0f;
                        if (cm) cm[k] = alive ? v : 0.0f;
                        if (mh) mh[k] = v;
                        ++k;
                    }
            }
    }
}

// npd_gru_wide_list.hip: F = 256 / 512, 1 or 2 layers
int launch_wide_list(const npd_gru* g, const ListArgs& a, hipStream_t s);

}  // namespace gru
}  // namespace npd

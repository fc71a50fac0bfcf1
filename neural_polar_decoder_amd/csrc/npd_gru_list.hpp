// npd_gru_list.hpp -- what the two GRU list kernels share (npd_gru_list.hip: gru_list_kernel, weights in LDS, F <= 64;
// npd_gru_wide_list.hip: gru_wide_list_kernel, weights streamed, F = 256 / 512): the launch arguments, the pruning
// order, the tie rule and the epilogue in its two modes (plain, and CRC-aided selection with fused error counting:
// include/npd.h, "CRC-aided CRISP GRU list decoding").  npd_gru_list.hip owns the C entry points and dispatches to
// launch_wide_list.
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
    // CRC-aided selection and fused counting (the CA instantiations only; npd_gru_list_decode_crc / _crc_mc)
    int32_t* crc_ok;    // (B) or NULL
    int32_t* cand_crc;  // (B, L) or NULL
    unsigned long long* counters;  // 3 device counters, or NULL: no counting
    uint64_t seed, cw_offset;      // Philox message stream of the words counted against
    uint32_t crc_poly;             // bit i = coefficient of x^i; 0 with crc_c = 0: plain selection
    int crc_c;                     // its degree
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

// remainder of a path's information bits (bw at the set bits of a.info, wave-uniform), read as a polynomial of degree
// K - 1: npd_scl.hpp's crc_divide recurrence on a register of crc_c bits plus the bit shifted out
__device__ __forceinline__ uint32_t list_crc_divide(const ListArgs& a, const uint32_t (&bw)[kMaxWords]) {
    uint32_t reg = 0u;
#pragma unroll
    for (int w = 0; w < kMaxWords; ++w)
        if (32 * w < a.N)
            for (uint32_t im = a.info[w]; im != 0u; im &= im - 1u) {
                reg = (reg << 1) | ((bw[w] >> __builtin_ctz(im)) & 1u);
                reg ^= a.crc_poly & (0u - ((reg >> a.crc_c) & 1u));
            }
    return reg;
}

// word q of the Philox message words (a select chain: no dynamically indexed register array)
__device__ __forceinline__ uint32_t list_pick_word(const uint32_t (&mw)[8], int q) {
    uint32_t w = mw[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) w = (q == i) ? mw[i] : w;
    return w;
}

// The end of list_decode for one wave's columns: encode every path (bw: its bit words), fp32 distance to y, first
// minimum over the codeword's ls live slots, and the optional outputs (lane half 0 of the valid columns stores).
// CA (npd_gru_list_decode_crc / _crc_mc; the CA = false instantiations compile to what they were): with a.crc_c > 0
// every column divides its own path's information bits, and when a ballot of the pass flags finds a passing path in
// the codeword's slot group the first minimum runs over the passing slots only; with a.counters the chosen column
// compares its first K - crc_c information bits with the Philox message words and the wave's sums go to cnt[0..2]
// (wave-uniform; the kernel adds them to a.counters once, after its last tile).
template <bool CA = false>
__device__ __forceinline__ void list_finish(const ListArgs& a, const uint32_t (&bw)[kMaxWords], float met, int ls,
                                            int64_t cw, int64_t cwc, bool valid, int half, int slot, int base,
                                            unsigned long long* cnt = nullptr) {
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
    [[maybe_unused]] uint32_t reg = 0u;
    [[maybe_unused]] bool anyp = false;
    if constexpr (!CA) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float dt = __shfl(dist, base + (t < ls ? t : 0), 64);
            if (t == 0 || (t < ls && dt < best)) {
                best = t == 0 ? dt : (dt < best ? dt : best);
                bsel = t;
            }
        }
    } else {
        // eligible slots of this codeword: the passing ones if any passes, else every live one (slot 0 is always live,
        // so with no passing path this is the plain scan, comparison for comparison)
        uint32_t emask = (1u << ls) - 1u;
        if (a.crc_c > 0) {
            reg = list_crc_divide(a, bw);
            const uint32_t pm = (uint32_t)(__ballot(slot < ls && reg == 0u) >> base) & emask;
            anyp = pm != 0u;
            emask = anyp ? pm : emask;
        }
        bool found = false;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float dt = __shfl(dist, base + (t < ls ? t : 0), 64);
            if (((emask >> t) & 1u) && (!found || dt < best)) {
                best = dt;
                bsel = t;
                found = true;
            }
        }
    }
    if (half == 0 && valid && slot < a.L) {
        const bool alive = slot < ls;
        const bool chosen = slot == bsel;
        if (a.cand_metric) a.cand_metric[cw * a.L + slot] = alive ? met : __builtin_inff();
        if (a.sel && chosen) a.sel[cw] = bsel;
        if constexpr (CA) {
            if (a.cand_crc) a.cand_crc[cw * a.L + slot] = alive ? (int32_t)reg : -1;
            if (a.crc_ok && chosen) a.crc_ok[cw] = anyp ? 1 : 0;
        }
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
    if constexpr (CA) {
        if (a.counters) {
            // message words of this column's codeword: Philox block 0 holds bits 0 .. 127, block 1 bits 128 .. 255
            const int kc = a.K - a.crc_c;
            uint32_t mw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
                if (blk * 128 < kc) {
                    const u32x4 o = philox_block(a.seed, kStreamMsg, a.cw_offset + (uint64_t)cwc, (uint32_t)blk);
                    mw[4 * blk + 0] = o.x;
                    mw[4 * blk + 1] = o.y;
                    mw[4 * blk + 2] = o.z;
                    mw[4 * blk + 3] = o.w;
                }
            uint32_t e = 0u, cur = mw[0];
            int k = 0;
#pragma unroll
            for (int w = 0; w < kMaxWords; ++w)
                if (32 * w < N)
                    for (uint32_t im = a.info[w]; im != 0u; im &= im - 1u) {
                        e += (k < kc) ? (((bw[w] >> __builtin_ctz(im)) ^ cur) & 1u) : 0u;
                        cur >>= 1;
                        ++k;
                        if ((k & 31) == 0) cur = list_pick_word(mw, k >> 5);
                    }
            const bool mine = half == 0 && valid && slot == bsel;
            e = mine ? e : 0u;
            cnt[0] += (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum_u32(e));
            cnt[1] += (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum_u32(e ? 1u : 0u));
            cnt[2] += (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum_u32((mine && !anyp) ? 1u : 0u));
        }
    }
}

// the wave's sums of list_finish<true>, added once: one atomic triple per wave (counters[2] only with a CRC)
__device__ __forceinline__ void list_count_flush(const ListArgs& a, const unsigned long long* cnt, int lane) {
    if (a.counters && lane == 0) {
        atomicAdd(a.counters + 0, cnt[0]);
        atomicAdd(a.counters + 1, cnt[1]);
        if (a.crc_c > 0) atomicAdd(a.counters + 2, cnt[2]);
    }
}

// npd_gru_wide_list.hip: F = 256 / 512, 1 or 2 layers
int launch_wide_list(const npd_gru* g, const ListArgs& a, bool ca, hipStream_t s);

}  // namespace gru
}  // namespace npd

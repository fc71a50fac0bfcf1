// npd_gru_split.hpp -- what the split 16-bit MFMA kernels share (gru_decode_bf_kernel in npd_gru_split.hip, gru16p_kernel
// in npd_gru_split16.hip): the split variants, the kernels' argument block and the host's 16-bit image pieces.
// precision 1 = bf16x3 split (a*b ~ ah*bh + ah*bl + al*bh, ~2^-16 relative per product),
// precision 2 = plain bf16 (fp32 accumulate).  v_mfma_f32_32x32x16_bf16: 16x the fp32 MFMA rate.
// precision 3 = fp16x3 split ("SPLIT 4" below): the same three products on v_mfma_f32_32x32x16_f16, whose
// 11-bit significands make hi + lo a 22-bit split (a*b to ~2^-21 relative: fp32-class, against bf16x3's
// 2^-16).  fp16's exponent range is handled by exact power-of-2 scaling: weights (and the y projection's
// weights) x 2^8 on the host, states and received words x 2^8 at the split, so every accumulator holds
// 2^16 x its value (biases / one-hot constants pre-scaled by 2^16, and the gate nonlinearities take the
// 2^-16 in their exp2 constants: all exact).  Then hi and lo stay normal fp16 for |w| >= 5e-4 and
// |h| >= 5e-4 (smaller terms contribute below 2^-33 absolute).
// Same orientation as the fp32 kernel: an h' accumulator tile converts register-for-register into
// the B fragments of the next step (registers 8s..8s+7 -> k-step s, cdna_hip_programming.md sec. 3).
// Bias / one-hot / previous-decision terms stay an exact fp32 k-step (v_mfma_f32_32x32x2_f32).
#pragma once

#include <string.h>

#include "npd_gru_host.hpp"

namespace npd {
namespace gru {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef _Float16 hf8 __attribute__((ext_vector_type(8)));

// SPLIT: 1 = bf16, 3 = bf16 hi + lo, 4 = fp16 hi + lo (scaled), 5 = fp16 hi + lo, unscaled, gate constants folded
// into the weights (16-codeword kernels only, see build_image16)
template <int SPLIT>
struct SplitT {
    static constexpr bool kLo = SPLIT >= 3;
    static constexpr bool kF16 = SPLIT >= 4;
    static constexpr bool kFold = SPLIT == 5;  // accumulators hold -log2(e) a (r, z rows) / -2 log2(e) a (n rows)
    using V = std::conditional_t<kF16, hf8, bf8>;
    using E = std::conditional_t<kF16, _Float16, __bf16>;
    static constexpr float kIn = SPLIT == 4 ? 256.0f : 1.0f;           // B-operand scale (states, y)
    static constexpr float kAcc = SPLIT == 4 ? 1.0f / 65536.0f : 1.0f;  // accumulator -> value
    // exp2 arguments of sigmoid(a) = 1 / (1 + 2^(c1 a)) and tanh(x) = 2 / (1 + 2^(c2 x)) - 1 from the accumulators
    static constexpr float kC1 = kFold ? 1.0f : -1.44269504088896340736f * kAcc;
    static constexpr float kC2 = kFold ? 1.0f : -2.88539008177792681472f * kAcc;
};

struct ArgsB {
    const float* img;
    const f4* wy;  // [TT][N/16][64] bf16x8 fragments (hi, then lo for SPLIT 3)
    const float* y;   // NULL: no y input (y_h0)
    const float* h0;  // NULL: zero initial state; else (B, F L) as Args::h0 (16-codeword kernel only)
    const float* gt;
    float* decoded;
    float* logits;
    int64_t B;
    int N;
    int rev;
    int onehot;
    float b_lin;
    int64_t wy_lo;  // offset (in f4) of the lo Wy image
    uint32_t info[kMaxWords];
    // sweep / count mode (gru16p_kernel only): y, decoded and logits are nseg segments of (B, N) back to back; with
    // counters != NULL the decision at every position jj of the mask cmp is compared with msg[cw][slot[jj]] and
    // counters[2 s], [2 s + 1] += bit / block errors of segment s (npd_gru_decode_count_sweep)
    const float* msg;
    unsigned long long* counters;
    int K;
    int nseg;
    uint32_t slotw[kMaxN / 4];  // byte jj & 3 of word jj >> 2 = slot of position jj (copied to the LDS step table)
    uint32_t cmp[kMaxWords];    // bit jj & 31 of word jj >> 5: position jj is compared (as info; all slot values are slots)
};

static uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_to_f(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// IEEE binary16, round to nearest even (finite inputs within the fp16 range; subnormals handled)
static uint16_t f16_rne(float f) {
    const _Float16 h = (_Float16)f;  // clang lowers the host conversion with round-to-nearest-even
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
static float f16_to_f(uint16_t b) {
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}
// 16-bit split of v: SPLIT 4 -> fp16 of v * 2^8; SPLIT 5 -> fp16 of v (lo may be subnormal); else bf16 of v
template <int SPLIT>
static void split16(float v, uint16_t& hi, uint16_t& lo) {
    if (SPLIT >= 4) {
        const float s = SPLIT == 4 ? v * 256.0f : v;
        hi = f16_rne(s);
        lo = f16_rne(s - f16_to_f(hi));
    } else {
        hi = bf16_rne(v);
        lo = bf16_rne(v - bf16_to_f(hi));
    }
}

// 16-bit y projection fragments of `tiles` row tiles of `rows` (32 or 16) gate rows: lane l holds row l % rows, and
// k-step q pairs its 8 elements with y[8 (64 / rows) q + 8 (l / rows) + j]; hi image, then lo (SPLIT >= 3).  fr(row) =
// the gate row's factor.  Returns the lo image's offset in 16-B fragments (ArgsB::wy_lo)
template <int SPLIT, typename Fr>
static int64_t fill_wy16(const float* wih0, int tiles, int rows, int N, int Din, Fr&& fr, std::vector<float>& wy) {
    const int kw = 8 * (64 / rows), nq = N / kw;
    const size_t per = (size_t)tiles * nq * 64 * 8;  // 16-bit elements per image
    wy.assign((per * (SPLIT >= 3 ? 2 : 1) + 1) / 2, 0.0f);
    uint16_t* w16 = reinterpret_cast<uint16_t*>(wy.data());
    for (int t = 0; t < tiles; ++t)
        for (int q = 0; q < nq; ++q)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int row = rows * t + l % rows;
                    const int k = kw * q + 8 * (l / rows) + j;
                    const size_t e = (((size_t)t * nq + q) * 64 + l) * 8 + j;
                    uint16_t hi, lo;
                    split16<SPLIT>(fr(row) * wih0[(size_t)row * Din + k], hi, lo);
                    w16[e] = hi;
                    if (SPLIT >= 3) w16[per + e] = lo;
                }
    return (int64_t)(per / 8);
}

// the kernels' arguments from the handle and the call's operands; img / wy: the 16-codeword kernel's where it exists
inline ArgsB make_args_b(const npd_gru* g, const Args& a) {
    ArgsB b{};
    b.img = g->img16 ? g->img16 : g->img;
    b.wy = reinterpret_cast<const f4*>(g->img16 ? g->wy16 : g->wy);
    b.wy_lo = g->img16 ? g->wy16_lo : g->wy_lo;
    b.y = a.y; b.h0 = a.h0; b.gt = a.gt; b.decoded = a.decoded; b.logits = a.logits; b.B = a.B; b.N = a.N;
    b.rev = a.rev; b.onehot = a.onehot; b.b_lin = a.b_lin;
    b.nseg = 1;
    memcpy(b.info, a.info, sizeof(b.info));
    return b;
}

// npd_gru_split16.hip: gru16p_kernel on the handle's SplitT variant (g->split16)
int launch_split16(const npd_gru* g, const ArgsB& b, hipStream_t s);

// SplitT variant of a handle's precision: 32-codeword kernels (fp16x3 scaled) / 16-codeword kernel (fp16x3 folded)
inline int split_of(int precision, bool k16) { return precision == 1 ? 3 : precision == 3 ? (k16 ? 5 : 4) : 1; }

}  // namespace gru
}  // namespace npd

// npd_ml.hip -- maximum-likelihood and bitwise-MAP decoding against the whole codebook on the fp16 MFMA.
//
//   npd_ml_decode  <- the eval loops' inline ML block (run_models.py:347-351, rnn_all.py:892-948 under --run_ML):
//                     idx = argmin_i ||y - c_i||^2 = argmax_i sum_j y_j c_i[j], decoded = all_message_bits[idx]
//   npd_map_decode <- PolarCode.bitwise_MAP (polar.py:879-899): per message bit, logsumexp of a.c_i over the codewords
//                     with the bit +1 minus the same over the codewords with the bit -1, a = (2/sigma^2) y
//
// Both are a GEMM of the received words against the +-1 codebook.  The codebook never exists in memory: the code is
// linear, so the sign mask of codeword i is the XOR of the generator rows g[b] over the set bits b of i, and on fp16
// +-1 values that XOR acts on the sign bits of an MFMA A fragment held in registers.
//
// Tiling (v_mfma_f32_16x16x32_f16, D = A B): A = 16 consecutive codewords (rows; row r of tile t is index 16 t + r),
// B = 16 received words (columns), k = code position.  Lane l holds A[row l & 15][k = 8 (l >> 4) + j], B[k][col l & 15]
// and D[row 4 (l >> 4) + reg][col l & 15].  A's fragment for tile t = base(row bits) ^ hi(t >> 6) ^ table[t & 63]:
// the 64-entry table of expanded sign masks is built once per workgroup in LDS (4 KB per k-step), the hi part changes
// every 64 tiles.
//
// Exactness: a received fp32 value, scaled by its word's power of two so that the largest magnitude lies in
// [2^14, 2^15), splits exactly into three fp16 planes (hi, mid, lo: 3 x 11 significand bits >= 24).  +-1 times an fp16
// value is exact, so the three MFMA products sum EXACT products in fp32; nothing is dropped (unlike the hi/lo weight
// splits of the GRU and conv kernels, which omit lo x lo).  The planes are accumulated lo, mid, hi: the partial sums of
// the first two are below 2^-10 of sum |y|, so the rounding error is that of the N-term hi sum.
//
// A workgroup is 4 waves that share WT word tiles; each wave sweeps a quarter of the codeword tiles and the four
// partial results meet in LDS.  Nothing is allocated and nothing but the outputs is written, so both entry points are
// a single kernel node under graph capture.
#include <math.h>

#include "npd_common.hpp"

namespace npd {
namespace ml {

typedef _Float16 hf8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kMaxK = 22;     // ML: 2^22 codewords
constexpr int kMaxKMap = 16;  // MAP: 2^16 codewords
constexpr float kLog2e = 1.44269504088896340736f;

struct MlParams {             // by value in the kernel arguments
    uint64_t g[kMaxK];        // g[b] = sign mask (bit j = position j is -1) of the codeword of index 1 << b; 0 for b >= K
    int N, K;
};

// 8 sign bits -> the sign bits of 8 fp16 values in 4 dwords (value 2p in the low half of dword p)
__device__ __forceinline__ void expand8(uint32_t byte, uint32_t out[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
        out[p] = (((byte >> (2 * p)) & 1u) << 15) | (((byte >> (2 * p + 1)) & 1u) << 31);
}

// XOR of g[b0 + j] over the set bits j < nb of `bits`
__device__ __forceinline__ uint64_t xor_rows(const MlParams& p, uint32_t bits, int b0, int nb) {
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < nb; ++j)
        if ((bits >> j) & 1u) m ^= p.g[b0 + j];
    return m;
}

__device__ __forceinline__ hf8 as_hf8(const uint32_t d[4]) {
    union { uint32_t u[4]; hf8 h; } c;
    c.u[0] = d[0]; c.u[1] = d[1]; c.u[2] = d[2]; c.u[3] = d[3];
    return c.h;
}

__device__ __forceinline__ bool better(float v2, uint32_t i2, float v1, uint32_t i1) {
    return v2 > v1 || (v2 == v1 && i2 < i1);
}

// The received words of this workgroup as MFMA B fragments: per word tile, k-step and plane (0 hi, 1 mid, 2 lo).
// wexp[w] = the exponent e of the word's largest magnitude (the planes hold y * 2^(14 - e)).
template <int KS, int WT>
__device__ __forceinline__ void load_words(const float* __restrict__ y, int64_t B, int N, int64_t word0, int lane,
                                           hf8 (&bf)[WT][KS][3], int (&wexp)[WT]) {
    const int col = lane & 15, quad = lane >> 4;
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const int64_t word = word0 + w * 16 + col;
        float v[KS][8];
        float amax = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k0 = 32 * ks + 8 * quad;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[ks][j] = (word < B && k0 + j < N) ? y[word * N + k0 + j] : 0.0f;
                amax = fmaxf(amax, fabsf(v[ks][j]));
            }
        }
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        int ef = (int)((fbits(amax) >> 23) & 0xFFu);
        if (ef == 0) ef = 1;          // zero / subnormal maximum: the smallest normal exponent
        if (ef == 255) ef = 254;      // non-finite input: no meaning, but no trap either
        const int e = ef - 127;
        wexp[w] = e;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            hf8 h, m, l;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float s = ldexpf(v[ks][j], 14 - e);
                const _Float16 hi = (_Float16)s;
                const float r1 = s - (float)hi;
                const _Float16 mid = (_Float16)r1;
                const float r2 = r1 - (float)mid;
                h[j] = hi;
                m[j] = mid;
                l[j] = (_Float16)r2;
            }
            bf[w][ks][0] = h;
            bf[w][ks][1] = m;
            bf[w][ks][2] = l;
        }
    }
}

// LDS table of the 64 low-tile masks: entry (ks, tl, quad) = the expanded sign bits of positions 32 ks + 8 quad .. + 7
// of XOR g[4 + b] over the bits b of tl
template <int KS>
__device__ __forceinline__ void build_table(const MlParams& p, uint4* TL) {
    for (int e = threadIdx.x; e < KS * 64 * 4; e += blockDim.x) {
        const int quad = e & 3, tl = (e >> 2) & 63, ks = e >> 8;
        const uint64_t m = xor_rows(p, (uint32_t)tl, 4, 6);
        uint32_t d[4];
        expand8((uint32_t)(m >> (32 * ks + 8 * quad)) & 0xFFu, d);
        TL[e] = make_uint4(d[0], d[1], d[2], d[3]);
    }
}

// One wave's sweep over codeword tiles [t0, t0 + Tw): epi(t, acc) sees the 16 x (16 WT) correlations of tile t
// (acc[w][reg] = word column l & 15 of tile w, codeword row 4 (l >> 4) + reg), in units of 2^(14 - e) per word.
template <int KS, int WT, class Epi>
__device__ __forceinline__ void codebook_sweep(const MlParams& p, const uint4* TL, const hf8 (&bf)[WT][KS][3],
                                               uint32_t t0, uint32_t Tw, int lane, Epi&& epi) {
    const int quad = lane >> 4;
    uint32_t arow[KS][4];
    {
        const uint64_t m = xor_rows(p, (uint32_t)(lane & 15), 0, 4);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            expand8((uint32_t)(m >> (32 * ks + 8 * quad)) & 0xFFu, arow[ks]);
#pragma unroll
            for (int i = 0; i < 4; ++i) arow[ks][i] ^= 0x3C003C00u;  // +1.0 | +1.0
        }
    }
    const uint32_t n = Tw < 64u ? Tw : 64u;
    for (uint32_t tb = t0; tb < t0 + Tw; tb += 64) {
        const uint64_t hm = xor_rows(p, tb >> 6, 10, kMaxK - 10);
        uint32_t ab[KS][4];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            expand8((uint32_t)(hm >> (32 * ks + 8 * quad)) & 0xFFu, ab[ks]);
#pragma unroll
            for (int i = 0; i < 4; ++i) ab[ks][i] ^= arow[ks][i];
        }
        const uint32_t tl0 = tb & 63u, thi = tb & ~63u;
        for (uint32_t tl = tl0; tl < tl0 + n; ++tl) {
            hf8 a[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 m = TL[(ks * 64 + tl) * 4 + quad];
                const uint32_t d[4] = {ab[ks][0] ^ m.x, ab[ks][1] ^ m.y, ab[ks][2] ^ m.z, ab[ks][3] ^ m.w};
                a[ks] = as_hf8(d);
            }
            f4 acc[WT];
#pragma unroll
            for (int w = 0; w < WT; ++w) acc[w] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int pl = 2; pl >= 0; --pl)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int w = 0; w < WT; ++w)
                        acc[w] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks], bf[w][ks][pl], acc[w], 0, 0, 0);
            epi(thi + tl, acc);
        }
    }
}

// The ML sweep of one workgroup: every thread with threadIdx.x < 16 WT returns (value, index) of its word
// (word tile threadIdx.x >> 4, column threadIdx.x & 15); value is in units of 2^(14 - e).  sv / si: 4 x 16 WT each.
template <int KS, int WT>
__device__ __forceinline__ void ml_sweep(const MlParams& p, const uint4* TL, const hf8 (&bf)[WT][KS][3], float* sv,
                                         uint32_t* si, float& best_v, uint32_t& best_i) {
    const int lane = threadIdx.x & 63, quad = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform: tile indices stay scalar
    const uint32_t T = p.K > 4 ? 1u << (p.K - 4) : 1u;          // codeword tiles
    const uint32_t nvalid = p.K >= 4 ? 16u : 1u << p.K;         // rows of the only tile that are codewords
    const uint32_t Tw = T >= 4 ? T / 4 : T;                     // tiles per sweeping wave
    const bool sweeps = T >= 4 || wave == 0;
    float bv[WT][4];
    uint32_t bt[WT][4];
#pragma unroll
    for (int w = 0; w < WT; ++w)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bv[w][r] = -INFINITY;
            bt[w][r] = 0u;
        }
    if (sweeps)
        codebook_sweep<KS, WT>(p, TL, bf, wave * Tw, Tw, lane, [&](uint32_t t, const f4 (&acc)[WT]) {
#pragma unroll
            for (int w = 0; w < WT; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool up = acc[w][r] > bv[w][r];     // strict: the first (smallest) tile keeps a tie
                    bv[w][r] = up ? acc[w][r] : bv[w][r];
                    bt[w][r] = up ? t : bt[w][r];
                }
        });
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        float v = -INFINITY;
        uint32_t i = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = 4u * quad + r;
            const bool ok = sweeps && row < nvalid;           // padding rows of a K < 4 tile never win
            const float vr = ok ? bv[w][r] : -INFINITY;
            const uint32_t ir = ok ? (bt[w][r] << 4) | row : 0u;
            if (better(vr, ir, v, i)) { v = vr; i = ir; }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float v2 = __shfl_xor(v, o, 64);
            const uint32_t i2 = (uint32_t)__shfl_xor((int)i, o, 64);
            if (better(v2, i2, v, i)) { v = v2; i = i2; }
        }
        if (quad == 0) {
            sv[wave * 16 * WT + w * 16 + lane] = v;
            si[wave * 16 * WT + w * 16 + lane] = i;
        }
    }
    __syncthreads();
    best_v = -INFINITY;
    best_i = 0u;
    if (threadIdx.x < 16 * WT) {
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            const float v2 = sv[wv * 16 * WT + threadIdx.x];
            const uint32_t i2 = si[wv * 16 * WT + threadIdx.x];
            if (better(v2, i2, best_v, best_i)) { best_v = v2; best_i = i2; }
        }
    }
}

// ---------------------------------------------------------------------------------- ML
template <int KS, int WT>
__global__ __launch_bounds__(256) void ml_decode_kernel(const MlParams p, const float* __restrict__ y,
                                                        float* __restrict__ msg_hat, int32_t* __restrict__ idx,
                                                        float* __restrict__ metric, int64_t B) {
    __shared__ uint4 TL[KS * 64 * 4];
    __shared__ float sv[4 * 16 * WT];
    __shared__ uint32_t si[4 * 16 * WT];
    const int lane = threadIdx.x & 63;
    const int64_t word0 = (int64_t)blockIdx.x * (16 * WT);
    build_table<KS>(p, TL);
    hf8 bf[WT][KS][3];
    int wexp[WT];
    load_words<KS, WT>(y, B, p.N, word0, lane, bf, wexp);
    __syncthreads();
    float bv;
    uint32_t bi;
    ml_sweep<KS, WT>(p, TL, bf, sv, si, bv, bi);
    const int64_t word = word0 + threadIdx.x;
    if (threadIdx.x < 16 * WT && word < B) {
        if (idx) idx[word] = (int32_t)bi;
        if (metric) {
            // the winner's correlation, re-summed in fp64 from y (N terms once per word)
            const uint64_t m = xor_rows(p, bi, 0, kMaxK);
            double s = 0.0;
            for (int j = 0; j < p.N; ++j) {
                const double v = (double)y[word * p.N + j];
                s += ((m >> j) & 1ull) ? -v : v;
            }
            metric[word] = (float)s;
        }
        if (msg_hat)
            for (int k = 0; k < p.K; ++k) msg_hat[word * p.K + k] = ((bi >> (p.K - 1 - k)) & 1u) ? -1.0f : 1.0f;
    }
}

// ---------------------------------------------------------------------------------- bitwise MAP
// Sweep 1 = the ML sweep (the word's largest correlation, the logsumexp shift).  Sweep 2 recomputes the same
// correlations (bit for bit: the same MFMAs) and adds exp(a.c_i - max) into, per message bit, the sum of its class.
// A term is 2^frac on v_exp_f32 scaled by 2^floor in fp64, so the class that does not hold the ML codeword keeps its
// value down to 2^-1000 of the other (an LLR of ~690 nats) instead of flushing at fp32's 2^-126 (87 nats, which
// Polar(64,12) passes at 4 dB).  Bits 0-1 of the index are the accumulator register, bits 2-3 the lane's quad (settled
// in the final reduction), bits >= 4 are uniform over a tile and summed under scalar control (below).  One word tile
// per workgroup is what the entry point launches: the sweep is VALU- and fp64-bound, a second tile amortises nothing.
template <int KS, int WT>
__global__ __launch_bounds__(256) void map_decode_kernel(const MlParams p, const float* __restrict__ y,
                                                         float llr_scale, float* __restrict__ msg_hat,
                                                         float* __restrict__ llr, int64_t B) {
    constexpr int NT = kMaxKMap - 4;                 // tile-uniform index bits
    __shared__ uint4 TL[KS * 64 * 4];
    __shared__ float sv[4 * 16 * WT];
    __shared__ uint32_t si[4 * 16 * WT];
    __shared__ float smax[16 * WT];
    __shared__ double dred[4][16 * WT][2 * kMaxKMap];
    const int lane = threadIdx.x & 63, quad = lane >> 4, col = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t word0 = (int64_t)blockIdx.x * (16 * WT);
    const int K = p.K;
    build_table<KS>(p, TL);
    hf8 bf[WT][KS][3];
    int wexp[WT];
    load_words<KS, WT>(y, B, p.N, word0, lane, bf, wexp);
    __syncthreads();
    float bv;
    uint32_t bi;
    ml_sweep<KS, WT>(p, TL, bf, sv, si, bv, bi);
    if (threadIdx.x < 16 * WT) smax[threadIdx.x] = bv;
    __syncthreads();

    const uint32_t T = K > 4 ? 1u << (K - 4) : 1u;
    const uint32_t nvalid = K >= 4 ? 16u : 1u << K;
    const uint32_t Tw = T >= 4 ? T / 4 : T;
    const bool sweeps = T >= 4 || wave == 0;
    float fw[WT], cw[WT][4];
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        fw[w] = ldexpf(llr_scale * kLog2e, wexp[w] - 14);   // log2-units per accumulator unit
#pragma unroll
        for (int r = 0; r < 4; ++r)                         // padding rows of a K < 4 tile: floored to a weight of 2^-1000
            cw[w][r] = 4u * quad + r < nvalid ? -(smax[w * 16 + col] * fw[w]) : -INFINITY;
    }
    // D[w][r]: this lane's sum per accumulator register (index bits 0-1).  Tile bits j < m = log2(Tw) vary inside the
    // wave's range and are summed as a binary counter over the tile index: when bit j of t is 0 the sum of the
    // finished 2^j-tile block waits in H[j]; when it is 1 the finished block goes to S1[j], its waiting left sibling
    // to S0[j], and their sum carries to level j + 1 -- two levels per tile on average instead of one add per bit.
    // Tile bits >= m are constant over the wave's range and take its total at the end.
    int m = 0;
    while ((1u << m) < Tw) ++m;
    const uint32_t t0 = (uint32_t)wave * Tw;
    double D[WT][4], S0[WT][NT], S1[WT][NT], H[WT][NT];
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        D[w][0] = D[w][1] = D[w][2] = D[w][3] = 0.0;
#pragma unroll
        for (int j = 0; j < NT; ++j) S0[w][j] = S1[w][j] = H[w][j] = 0.0;
    }
    if (sweeps)
        codebook_sweep<KS, WT>(p, TL, bf, t0, Tw, lane, [&](uint32_t t, const f4 (&acc)[WT]) {
            double carry[WT];
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                double d[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x = fmaf(acc[w][r], fw[w], cw[w][r]);
                    x = fmaxf(x, -1000.0f);                      // also turns a NaN into the floor
                    x = fminf(x, 64.0f);
                    const float fl = floorf(x);
                    const float e2 = __builtin_amdgcn_exp2f(x - fl);
                    d[r] = ldexp((double)e2, (int)fl);
                    D[w][r] += d[r];
                }
                carry[w] = (d[0] + d[1]) + (d[2] + d[3]);
            }
            bool open = true;
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (open && j < m) {
                    if ((t >> j) & 1u) {
#pragma unroll
                        for (int w = 0; w < WT; ++w) {
                            S1[w][j] += carry[w];
                            S0[w][j] += H[w][j];
                            carry[w] += H[w][j];
                        }
                    } else {
#pragma unroll
                        for (int w = 0; w < WT; ++w) H[w][j] = carry[w];
                        open = false;
                    }
                }
        });
    // per index bit b and class v: this lane's sum, summed over the four quads, then over the four waves
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const double tot = (D[w][0] + D[w][1]) + (D[w][2] + D[w][3]);
#pragma unroll
        for (int b = 0; b < kMaxKMap; ++b)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                double x;
                if (b == 0) x = v ? D[w][1] + D[w][3] : D[w][0] + D[w][2];
                else if (b == 1) x = v ? D[w][2] + D[w][3] : D[w][0] + D[w][1];
                else if (b == 2) x = (quad & 1) == v ? tot : 0.0;
                else if (b == 3) x = (quad >> 1) == v ? tot : 0.0;
                else if (b - 4 < m) x = v ? S1[w][b - 4] : S0[w][b - 4];
                else x = (int)((t0 >> (b - 4)) & 1u) == v ? tot : 0.0;
                x += __shfl_xor(x, 16, 64);
                x += __shfl_xor(x, 32, 64);
                if (quad == 0) dred[wave][w * 16 + col][2 * b + v] = x;
            }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * WT * K; e += blockDim.x) {
        const int wd = e / K, k = e % K, b = K - 1 - k;
        const int64_t word = word0 + wd;
        if (word >= B) continue;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            s0 += dred[wv][wd][2 * b];
            s1 += dred[wv][wd][2 * b + 1];
        }
        const float L = (float)(log(s0) - log(s1));
        if (llr) llr[word * K + k] = L;
        if (msg_hat) msg_hat[word * K + k] = L >= 0.0f ? 1.0f : -1.0f;
    }
}

// ---------------------------------------------------------------------------------- host
// Generator rows over GF(2): row k = the codeword (bit j = position j is -1) of the message with -1 in column k only.
// Polar: u[info[k]] = 1, butterfly.  PAC: rate profile, u_i = v_i ^ parity(state & taps) with state <- v
// (pac_code.py:181-208), rate-1 butterfly.
static uint64_t generator_row(const CodeParams& c, int k) {
    const int N = c.N;
    uint64_t v = 1ull << c.info[k], u = v;
    if (c.pac) {
        u = 0;
        uint32_t st = 0;
        for (int i = 0; i < N; ++i) {
            const uint32_t vi = (uint32_t)(v >> i) & 1u;
            const uint32_t par = (uint32_t)__builtin_popcount(st & c.tapmask) & 1u;
            u |= (uint64_t)(vi ^ par) << i;
            st = ((st << 1) | vi) & c.smask;
        }
    }
    for (int h = 1; h < N; h <<= 1) {
        uint64_t msk = 0;
        for (int i = 0; i < N; ++i)
            if (((i / h) & 1) == 0) msk |= 1ull << i;
        u ^= (u >> h) & msk;
    }
    return u;
}

static bool supported(const CodeParams& c, int map) {
    const int N = c.N, K = c.K;
    if (!(N == 8 || N == 16 || N == 32 || N == 64)) return false;
    return K >= 1 && K <= N && K <= (map ? kMaxKMap : kMaxK);
}

static MlParams make_params(const CodeParams& c) {
    MlParams p{};
    p.N = c.N;
    p.K = c.K;
    for (int b = 0; b < c.K; ++b) p.g[b] = generator_row(c, c.K - 1 - b);  // index bit b = message column K-1-b
    return p;
}

template <int KS, int WT>
static int launch_ml(const MlParams& p, const float* y, float* msg_hat, int32_t* idx, float* metric, int64_t B,
                     hipStream_t s) {
    const int64_t blocks = (B + 16 * WT - 1) / (16 * WT);
    hipLaunchKernelGGL((ml_decode_kernel<KS, WT>), dim3((unsigned)blocks), dim3(256), 0, s, p, y, msg_hat, idx, metric, B);
    return launch_check("ml_decode_kernel launch");
}

template <int KS, int WT>
static int launch_map(const MlParams& p, const float* y, float llr_scale, float* msg_hat, float* llr, int64_t B,
                      hipStream_t s) {
    const int64_t blocks = (B + 16 * WT - 1) / (16 * WT);
    hipLaunchKernelGGL((map_decode_kernel<KS, WT>), dim3((unsigned)blocks), dim3(256), 0, s, p, y, llr_scale, msg_hat, llr,
                       B);
    return launch_check("map_decode_kernel launch");
}

}  // namespace ml
}  // namespace npd

using namespace npd;

extern "C" int npd_ml_supported(const npd_code* code, int map) {
    NPD_ARG(code != nullptr, "npd_ml_supported: code is NULL");
    return ml::supported(code->p, map) ? 1 : 0;
}

extern "C" int npd_ml_decode(const npd_code* code, const float* y, float* msg_hat, int32_t* idx, float* metric,
                             int64_t B, void* stream) {
    NPD_ARG(code != nullptr, "npd_ml_decode: code is NULL");
    NPD_ARG(B >= 0, "npd_ml_decode: B < 0");
    if (!ml::supported(code->p, 0))
        return fail(NPD_ENOTSUP, "npd_ml_decode: needs N in {8, 16, 32, 64} and 1 <= K <= 22");
    NPD_ARG(msg_hat != nullptr || idx != nullptr || metric != nullptr, "npd_ml_decode: no output requested");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr, "npd_ml_decode: y is NULL");
    NPD_ARG(B <= (int64_t)0x7fffffff * 16, "npd_ml_decode: B too large for one call");
    const ml::MlParams p = ml::make_params(code->p);
    hipStream_t s = (hipStream_t)stream;
    // word tiles per workgroup: as many as still leave every CU several workgroups
    const int64_t fill = (int64_t)device_cu_count() * 4;
    const int wt = B >= fill * 64 ? 4 : (B >= fill * 32 ? 2 : 1);
    if (p.N == 64) {
        if (wt == 4) return ml::launch_ml<2, 4>(p, y, msg_hat, idx, metric, B, s);
        if (wt == 2) return ml::launch_ml<2, 2>(p, y, msg_hat, idx, metric, B, s);
        return ml::launch_ml<2, 1>(p, y, msg_hat, idx, metric, B, s);
    }
    if (wt == 4) return ml::launch_ml<1, 4>(p, y, msg_hat, idx, metric, B, s);
    if (wt == 2) return ml::launch_ml<1, 2>(p, y, msg_hat, idx, metric, B, s);
    return ml::launch_ml<1, 1>(p, y, msg_hat, idx, metric, B, s);
}

extern "C" int npd_map_decode(const npd_code* code, const float* y, float llr_scale, float* msg_hat, float* llr,
                              int64_t B, void* stream) {
    NPD_ARG(code != nullptr, "npd_map_decode: code is NULL");
    NPD_ARG(B >= 0, "npd_map_decode: B < 0");
    if (!ml::supported(code->p, 1))
        return fail(NPD_ENOTSUP, "npd_map_decode: needs N in {8, 16, 32, 64} and 1 <= K <= 16");
    NPD_ARG(msg_hat != nullptr || llr != nullptr, "npd_map_decode: no output requested");
    NPD_ARG(llr_scale >= 0.0f && llr_scale <= 3.0e38f, "npd_map_decode: llr_scale must be finite and >= 0");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr, "npd_map_decode: y is NULL");
    NPD_ARG(B <= (int64_t)0x7fffffff * 16, "npd_map_decode: B too large for one call");
    const ml::MlParams p = ml::make_params(code->p);
    hipStream_t s = (hipStream_t)stream;
    // one word tile per workgroup: the sweep is bound by the VALU and fp64 work per correlation, which a second word
    // tile does not amortise (measured: 9.5 vs 9.5 ms at (32,16), 0.92 vs 1.64 ms at (64,12), 2^18 words)
    if (p.N == 64) return ml::launch_map<2, 1>(p, y, llr_scale, msg_hat, llr, B, s);
    return ml::launch_map<1, 1>(p, y, llr_scale, msg_hat, llr, B, s);
}

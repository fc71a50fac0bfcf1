// npd_scl.hpp -- SC-List decoding kernels (PolarCode.scl_decode, polar.py:793-876, use_CRC=False), shared by
// npd_scl.hip (the Polar instantiations and the C ABI), npd_scl_pac.hip (the PAC instantiations) and, for lists of
// 9 .. 32 paths, npd_scl_wide.hip / npd_scl_pac_wide.hip (G = 16 and 32, on the iterative LDS kernel at every N).
// The CRC-aided selection (use_CRC=True, polar.py:849-866; template flag CRC, see "CRC-aided selection" below) is a
// second epilogue of the same kernels, instantiated in npd_scl_crc.hip / _pac / _wide / _pac_wide.
//
// Layout: a list of L paths per codeword lives in G = pow2ceil(L) adjacent lanes, one path per lane,
// so 64/G codewords share a wave.  At N <= 64 and L <= 8 every lane runs the same compile-time-unrolled min-sum SC schedule
// as npd_sc_fast.hip on its own path state (LLRs of each level and partial sums in VGPRs); the
// channel LLRs are identical for the whole group and never move.
//
// At an information leaf the group's 2s candidates (s = current list size) are, in the reference's
// list order, [keep_0 .. keep_{s-1}, flip_0 .. flip_{s-1}] with metrics m_j and fl32(m_j + |l_j|)
// (polar.py:830-843).  When 2s > L the survivors are torch.topk's choice (polar.py:777-791): if no
// metric tie straddles the L-th place the survivor set is unique and is found by rank counting (two
// ballots); otherwise the group runs the exact std::nth_element statement of npd_nth.hpp.  Survivors
// keep list order.  Lane j then takes its candidate's parent state through ds_bpermute -- only the
// values that are still live after this leaf (known at compile time from the leaf index), never the
// channel level.
//
// The final choice is the reference's ML step (polar.py:868-874): each path's codeword
// (encode_plotkin of its decisions, computed on sign/zero bit masks) is compared with y in fp32 and the
// first minimum wins.  The leaf LLRs of the chosen path (scl_decode's first output) equal a genie SC
// pass with gt = the chosen u_hat; the host wrapper runs npd_sc_decode for that when asked.
//
// PAC (template flag PAC, selected with if constexpr: the Polar instantiations compile to what they were):
// the same list decoder with pac_sc_decode's leaf step (pac_code.py:534-573).  Each path also carries its
// convolution state, the last len(g_array)-1 values of v_hat as a bit mask under smask (bit t = v_{i-1-t} is
// -1), initially 0 (all +1); u0 = conv1bTrans(+1, state) = (-1)^parity(state & tapmask).  A frozen leaf
// decides u = u0 (v = +1, the state shifts in a 0) and pays |l| unless sign(l) == u0; an information leaf
// forks on u = +-sign(l) exactly as Polar does and advances the state with v = u * u0, or leaves it alone
// when l == 0 (u = v = 0).  The state is one more value fetched from the source lane on a path switch.
// v_hat is needed only for the chosen path (msg_hat, the fused counts): it is recovered there from u_hat by the
// inverse convolution (v_i = u_i * u0, no state advance where u_i = 0), position by position (pac_unconv_word) or,
// at N <= 64 when no decision is 0, as a polynomial division on the whole word (pac_unconv_fast).
#pragma once
#include "npd_common.hpp"
#include "npd_nth.hpp"
#include "npd_sc_prim.hpp"

namespace npd {
namespace scl {

struct Args {
    const float* y;
    float* msg;                    // (B,K) or null
    float* uhat;                   // (B,N) or null
    unsigned long long* counters;  // {bit errors, block errors} (CRC: and {words no path passed for}) or null
    uint64_t seed;
    uint64_t cw_offset;
    int64_t B;
    int64_t ntiles;
    float scale;
    int L;
    uint32_t count;
    uint32_t crc_poly;             // CRC: the polynomial (bit i = coefficient of x^i) and its degree
    int crc_c;
    int32_t* crc_ok;               // CRC: (B) or null
};

typedef float f4 __attribute__((ext_vector_type(4)));

// value of lane (group base + T) for every lane of a G-lane group
template <int G, int T>
__device__ __forceinline__ float gb(float x, int src_lane) {
    if constexpr (G == 1) {
        return x;
    } else if constexpr (G == 2) {
        constexpr int ctl = T | (T << 2) | ((2 + T) << 4) | ((2 + T) << 6);
        return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), ctl, 0xF, 0xF, false));
    } else if constexpr (G == 4) {
        constexpr int ctl = T * 0x55;
        return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), ctl, 0xF, 0xF, false));
    } else {
        return __shfl(x, src_lane, 64);
    }
}

template <int N, int G>
struct Lane {
    static constexpr int W = (N + 31) / 32;
    float lv[2 * N];   // level d at lv[2^d .. 2^(d+1)); channel level at lv[N .. 2N)
    float beta[N];     // partial sums
    float m;           // path metric (polar.py:803)
    uint32_t sm[W];    // decision sign bits by position (u = -1)
    uint32_t zm[W];    // decision zero bits by position (u = 0, from sign(0))
    uint32_t fz[W];    // frozen bits (re-materialised per tile)
    int base;          // lane id of the group's first lane
    int j;             // index within the group (= list slot)
    uint32_t slot;     // wave-uniform: information bits decided so far
    int L;
    uint32_t st;       // PAC: convolution state (bit t set iff v_{i-1-t} = -1)
    uint32_t tap, smk; // PAC: wave-uniform CodeParams::tapmask / smask
};

// PAC: sign bit of u0 = conv1bTrans(+1, state) (pac_code.py:188-193)
__device__ __forceinline__ uint32_t pac_par(uint32_t st, uint32_t tap) {
    return (uint32_t)__builtin_popcount(st & tap) & 1u;
}

// PAC: sign bits of v_hat for one 32-bit word of u_hat (sign bits sw, zero bits zw; nbits positions), the inverse
// convolution run position by position: v_i = u_i * u0, and a zero decision leaves the state alone.  Branch-free
// (a select per position, unrolled, keeps one lane mask per position live in SGPRs: 164 SGPR spills at N = 64).
__device__ __forceinline__ uint32_t pac_unconv_word(uint32_t sw, uint32_t zw, int nbits, uint32_t& st, uint32_t tap,
                                                    uint32_t smk) {
    uint32_t vw = 0u;
#pragma unroll 8
    for (int b = 0; b < nbits; ++b) {
        const uint32_t negv = ((sw >> b) & 1u) ^ pac_par(st, tap);
        vw |= negv << b;
        const uint32_t sh = ((st << 1) | negv) & smk;
        st ^= (st ^ sh) & (((zw >> b) & 1u) - 1u);
    }
    return vw;
}

// PAC, N <= 64, no zero decision: v = u / g in GF(2)[D] mod D^N with g(D) = 1 + sum over taps t of D^(t+1).
// g^N = g(D^N) = 1 mod D^N, so 1 / g = g^(N-1) = g(D) g(D^2) g(D^4) ... g(D^(N/2)): log2(N) stages of one shifted
// xor per tap on the whole word (bit i = position i; bits at and above N are never read).
template <int N>
__device__ __forceinline__ uint64_t pac_unconv_fast(uint64_t x, uint32_t tap) {
#pragma unroll
    for (int k = 0; k < log2c<N>(); ++k) {
        uint64_t acc = x;
        for (uint32_t m = tap; m != 0u; m &= m - 1u) {  // wave-uniform
            const int sh = (__builtin_ctz(m) + 1) << k;
            if (sh < 64) acc ^= x << sh;
        }
        x = acc;
    }
    return x;
}

// ---------------------------------------------------------------------------------- CRC-aided selection
// Template flag CRC (npd_scl_decode_crc, instantiated in npd_scl_crc*.hip; the CRC = false instantiations compile to
// what they were): the distance step is replaced by a CRC over every surviving path's K information decisions
// (Polar: u_hat, PAC: v_hat, so every live lane runs the inverse convolution, not only the winner).  The
// information positions of a word are the set bits of ~frozen[w], a wave-uniform mask: the division needs no
// info[] loads and no per-bit LDS reads.  The register is c bits wide plus the bit shifted out: polar.py:738-748's
// division, MSB first, zero initial value, no reflection, no final XOR.

// information positions among the NB positions that word w holds (wave-uniform)
template <int NB>
__device__ __forceinline__ uint32_t info_word(const CodeParams& p, int w) {
    uint32_t iw = ~p.frozen[w];
    if constexpr (NB < 32) iw &= (1u << NB) - 1u;
    return iw;
}

// remainder of the path's information bits (sign words vs, bit 1 = symbol -1) read as a polynomial of degree K - 1
template <int W, int NB>
__device__ __forceinline__ uint32_t crc_divide(const uint32_t (&vs)[W], const CodeParams& p, uint32_t poly, int c) {
    uint32_t reg = 0u;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t word = vs[w];
        for (uint32_t im = info_word<NB>(p, w); im != 0u; im &= im - 1u) {
            reg = (reg << 1) | ((word >> __builtin_ctz(im)) & 1u);
            reg ^= poly & (0u - ((reg >> c) & 1u));
        }
    }
    return reg;
}

// The list slot chosen for one group of G lanes: the passing path of smallest metric, or, when no path of the group
// passes (decided from a ballot of the pass flags, not from the key), the live path of smallest metric; the
// (value, index) butterfly of the ML step, so the first in list order wins a tie.
template <int G>
__device__ __forceinline__ int crc_choose(float m, bool pass, bool live, int j, int base, bool& any) {
    const unsigned long long bal = __ballot(pass);
    const unsigned long long gm = G >= 64 ? ~0ull : ((1ull << G) - 1ull);
    any = ((bal >> base) & gm) != 0ull;
    float bd = (any ? pass : live) ? m : __builtin_inff();
    int bi = j;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        const float od = __shfl_xor(bd, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (od < bd || (od == bd && oi < bi)) {
            bd = od;
            bi = oi;
        }
    }
    return bi;
}

// word q of the Philox message words (a select chain: no dynamically indexed register array)
template <int MW>
__device__ __forceinline__ uint32_t pick_word(const uint32_t (&mw)[MW], int q) {
    uint32_t w = mw[0];
#pragma unroll
    for (int t = 1; t < MW; ++t) w = (q == t) ? mw[t] : w;
    return w;
}

// The winner's lane: msg_hat row (K values, the CRC columns included) from the sign words vs and zero words zs at the
// information positions in order, and the errors of the first kc = K - c of them against the Philox message words.
template <int W, int NB, int MW>
__device__ __forceinline__ uint32_t crc_emit(const uint32_t (&vs)[W], const uint32_t (&zs)[W], const CodeParams& p,
                                             float* mrow, const uint32_t (&mw)[MW], int kc) {
    uint32_t e = 0u, cur = 0u;
    int k = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        for (uint32_t im = info_word<NB>(p, w); im != 0u; im &= im - 1u) {
            const int b = __builtin_ctz(im);
            if ((k & 31) == 0) cur = pick_word<MW>(mw, k >> 5);
            const uint32_t sb = (vs[w] >> b) & 1u, zb = (zs[w] >> b) & 1u;
            if (mrow) mrow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
            e += k < kc ? ((sb ^ (cur & 1u)) | zb) : 0u;
            cur >>= 1;
            ++k;
        }
    }
    return e;
}

// first position whose partial sum is still read after leaf I: the start of the highest ancestor that
// still needs its left block for a g-update, or that will combine partial sums (spine nodes skip it)
template <int N, int I>
constexpr int beta_live_start() {
    constexpr int n = log2c<N>();
    for (int D = n; D >= 1; --D) {
        const int S0 = (I >> D) << D;
        const int h = 1 << (D - 1);
        const bool inleft = (I - S0) < h;
        const bool spine = S0 + (1 << D) == N;
        if (inleft || !spine) return S0;
    }
    return I;
}

template <int N, int G, int I, int D>
__device__ __forceinline__ void copy_levels(Lane<N, G>& c, int src) {
    if constexpr (D >= 1) {
        if constexpr (((I >> (D - 1)) & 1) == 0) {  // I in the left child of its level-D ancestor: input live
#pragma unroll
            for (int k = (1 << D); k < (2 << D); ++k) c.lv[k] = __shfl(c.lv[k], src, 64);
        }
        copy_levels<N, G, I, D - 1>(c, src);
    }
}

template <int N, int G, int I>
__device__ __forceinline__ void copy_live(Lane<N, G>& c, int src) {
    constexpr int n = log2c<N>();
    copy_levels<N, G, I, n - 1>(c, src);
    constexpr int b0 = beta_live_start<N, I>();
#pragma unroll
    for (int k = b0; k < I; ++k) c.beta[k] = __shfl(c.beta[k], src, 64);
#pragma unroll
    for (int w = 0; w <= (I >> 5); ++w) {
        c.sm[w] = (uint32_t)__shfl((int)c.sm[w], src, 64);
        c.zm[w] = (uint32_t)__shfl((int)c.zm[w], src, 64);
    }
}

// survivors of pruneLists for one group when a metric tie straddles the L-th place (rare): exact rule
// km / fm arrive as 8-wide vectors (VGPRs): arrays passed by reference would live in scratch, stored at
// every information leaf whether or not the tie path is taken
typedef float f8v __attribute__((ext_vector_type(8)));
template <int G>
__device__ __noinline__ uint32_t exact_mask(f8v km, f8v fm, int s, int L) {
    float negm[16];
#pragma unroll
    for (int t = 0; t < G; ++t) {
        negm[t] = -1.0f * km[t];
        negm[G + t] = -1.0f * fm[t];
    }
    // list order is [keep_0..keep_{s-1}, flip_0..flip_{s-1}]: compact when s < G
    float v[16];
    for (int c2 = 0; c2 < s; ++c2) {
        v[c2] = negm[c2];
        v[s + c2] = negm[G + c2];
    }
    return nth::prune_mask(v, 2 * s, L);
}

// Surviving candidates of one group at an information leaf (pruneLists, polar.py:777-791), as a mask over
// the list order [keep_0 .. keep_{s-1}, flip_0 .. flip_{s-1}]; m = this lane's path metric, a = |LLR|.
template <int G>
__device__ __forceinline__ uint32_t list_select(float m, float a, int j, int bl, int s, int L) {
    if (2 * s <= L) return (1u << (2 * s)) - 1u;
    float km[G], fm[G];
    km[0] = gb<G, 0>(m, bl + 0);
    fm[0] = km[0] + gb<G, 0>(a, bl + 0);
    if constexpr (G > 1) {
        km[1] = gb<G, 1>(m, bl + 1);
        fm[1] = km[1] + gb<G, 1>(a, bl + 1);
    }
    if constexpr (G > 2) {
        km[2] = gb<G, 2>(m, bl + 2);
        fm[2] = km[2] + gb<G, 2>(a, bl + 2);
        km[3] = gb<G, 3>(m, bl + 3);
        fm[3] = km[3] + gb<G, 3>(a, bl + 3);
    }
    if constexpr (G > 4) {
#pragma unroll
        for (int t = 4; t < G; ++t) {
            km[t] = __shfl(m, bl + t, 64);
            fm[t] = km[t] + __shfl(a, bl + t, 64);
        }
    }
    const float vk = m, vf = m + a;
    int ltk = 0, lek = 0, ltf = 0, lef = 0;
#pragma unroll
    for (int t = 0; t < G; ++t) {
        if (t < s) {
            ltk += (km[t] < vk) + (fm[t] < vk);
            lek += (km[t] <= vk) + (fm[t] <= vk);
            ltf += (km[t] < vf) + (fm[t] < vf);
            lef += (km[t] <= vf) + (fm[t] <= vf);
        }
    }
    const bool act = j < s;
    const bool sk = act && ltk < L;
    const bool sf = act && ltf < L;
    const bool st = act && ((ltk < L && lek > L) || (ltf < L && lef > L));
    const unsigned long long bk = __ballot(sk), bf = __ballot(sf), bs = __ballot(st);
    const uint32_t lowm = (1u << s) - 1u;
    uint32_t msel = ((uint32_t)(bk >> bl) & lowm) | (((uint32_t)(bf >> bl) & lowm) << s);
    if (bs) {
        const bool mine = ((uint32_t)(bs >> bl) & ((G >= 32) ? 0xFFFFFFFFu : ((1u << G) - 1u))) != 0u;
        if (mine) {
            f8v kv = {}, fv = {};
#pragma unroll
            for (int t = 0; t < G; ++t) {
                kv[t] = km[t];
                fv[t] = fm[t];
            }
            msel = exact_mask<G>(kv, fv, s, L);
        }
    }
    return msel;
}

template <bool PAC, int N, int G, int I>
__device__ __forceinline__ void info_leaf(Lane<N, G>& c, float l, int lane) {
    const float a = __builtin_fabsf(l);
    const int L = c.L;
    const uint32_t slot = c.slot;
    const int s = slot >= 3u ? L : ((1 << slot) < L ? (1 << slot) : L);
    const uint32_t msel = list_select<G>(c.m, a, c.j, c.base, s, L);
    // list slot j takes the j-th surviving candidate (list order)
    uint32_t mm = msel;
#pragma unroll
    for (int t = 0; t < G - 1; ++t)
        if (t < c.j) mm &= mm - 1u;
    const int cidx = mm ? __builtin_ctz(mm) : c.j;
    const bool flip = mm ? (cidx >= s) : false;
    const int srcj = flip ? cidx - s : (mm ? cidx : c.j);
    float u;
    if constexpr (G == 1) {
        u = sgn_bits(l);
        if (flip) {
            u = -u;
            c.m = c.m + a;
        }
    } else {
        const int src = c.base + srcj;
        const float ls = __shfl(l, src, 64);
        const float ms = __shfl(c.m, src, 64);
        copy_live<N, G, I>(c, src);
        if constexpr (PAC) c.st = (uint32_t)__shfl((int)c.st, src, 64);
        u = sgn_bits(ls);
        if (flip) u = -u;
        c.m = flip ? ms + __builtin_fabsf(ls) : ms;
    }
    if constexpr (PAC) {
        // v = u * u0 enters the state; u = 0 (from l = 0) leaves it alone (pac_code.py:553-568)
        const uint32_t negv = (u < 0.0f ? 1u : 0u) ^ pac_par(c.st, c.tap);
        const uint32_t sh = ((c.st << 1) | negv) & c.smk;
        c.st = (u == 0.0f) ? c.st : sh;
    }
    c.beta[I] = u;
    c.sm[I >> 5] |= (u < 0.0f ? 1u : 0u) << (I & 31);
    c.zm[I >> 5] |= (u == 0.0f ? 1u : 0u) << (I & 31);
    c.slot = slot + 1u;
    (void)lane;
}

template <bool PAC, int N, int G, int I>
__device__ __forceinline__ void leaf(Lane<N, G>& c, float l, int lane) {
    const bool frozen = (c.fz[I >> 5] >> (I & 31)) & 1u;
    if (frozen) {
        if constexpr (PAC) {
            // u = u0, v = +1 (pac_code.py:545-551); the metric pays |l| unless sign(l) == u0 (sign(0) = 0 never is)
            const uint32_t par = pac_par(c.st, c.tap);
            const bool match = (l != 0.0f) && ((fbits(l) >> 31) == par);
            c.m = c.m + (match ? 0.0f : __builtin_fabsf(l));
            c.beta[I] = bitsf(0x3f800000u | (par << 31));
            c.sm[I >> 5] |= par << (I & 31);
            c.st = (c.st << 1) & c.smk;
        } else {
            const float pen = (l > 0.0f) ? 0.0f : __builtin_fabsf(l);  // |l| * (sign(l) != 1), polar.py:814
            c.m = c.m + pen;
            c.beta[I] = 1.0f;
        }
    } else {
        info_leaf<PAC, N, G, I>(c, l, lane);
    }
}

template <bool PAC, int N, int G, int D, int S0>
__device__ __forceinline__ void node(Lane<N, G>& c, int lane) {
    if constexpr (D == 0) {
        leaf<PAC, N, G, S0>(c, c.lv[1], lane);
    } else {
        constexpr int h = 1 << (D - 1);
#pragma unroll
        for (int j = 0; j < h; ++j) c.lv[h + j] = f_minsum_fmin(c.lv[2 * h + j], c.lv[3 * h + j]);
        node<PAC, N, G, D - 1, S0>(c, lane);
#pragma unroll
        for (int j = 0; j < h; ++j) c.lv[h + j] = c.beta[S0 + j] * c.lv[2 * h + j] + c.lv[3 * h + j];
        node<PAC, N, G, D - 1, S0 + h>(c, lane);
        if constexpr (S0 + (1 << D) < N) {  // nodes on the right spine never feed a g-update
#pragma unroll
            for (int j = 0; j < h; ++j) c.beta[S0 + j] = c.beta[S0 + j] * c.beta[S0 + h + j];
        }
    }
}

template <int N, int G, bool PAC, bool CRC = false>
__global__ __launch_bounds__(64) void scl_kernel(const CodeParams p, const Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int n = log2c<N>();
    constexpr int C = N / 4;      // 16-B chunks per row
    constexpr int T = 64 / G;     // codewords per wave tile
    constexpr int W = (N + 31) / 32;
    const int lane = threadIdx.x;
    const f4* y4 = reinterpret_cast<const f4*>(a.y);
    const int64_t last4 = a.B * C - 1;
    const int K = p.K;

    Lane<N, G> c;
    c.j = lane & (G - 1);
    c.base = lane - c.j;
    c.L = a.L;
    const int r = lane / G;       // row of this lane's codeword in the tile
    const int sw = swz<C>(r);
    const int s_final = K >= 3 ? a.L : ((1 << K) < a.L ? (1 << K) : a.L);

    uint32_t err_bits = 0, err_blocks = 0;
    [[maybe_unused]] uint32_t err_crc = 0;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t row0 = t * T;
        // ---- stage the tile's received words in LDS (coalesced), swizzled rows
        __syncthreads();
        for (int i = lane; i < T * C; i += 64) {
            const int rr = i / C, cc = i % C;
            int64_t gi = row0 * C + i;
            gi = gi < last4 ? gi : last4;
            *reinterpret_cast<f4*>(lds + 16 * (rr * C + (cc ^ swz<C>(rr)))) = y4[gi];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const f4 v = *reinterpret_cast<const f4*>(lds + 16 * (r * C + (q ^ sw)));
            c.lv[N + 4 * q + 0] = rmul(a.scale, v.x);
            c.lv[N + 4 * q + 1] = rmul(a.scale, v.y);
            c.lv[N + 4 * q + 2] = rmul(a.scale, v.z);
            c.lv[N + 4 * q + 3] = rmul(a.scale, v.w);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint32_t fw = p.frozen[w];
            asm volatile("" : "+s"(fw));
            c.fz[w] = fw;
            c.sm[w] = 0u;
            c.zm[w] = 0u;
        }
        c.m = 0.0f;
        c.slot = 0u;
        if constexpr (PAC) {
            c.st = 0u;
            c.tap = p.tapmask;
            c.smk = p.smask;
        }
        node<PAC, N, G, n, 0>(c, lane);

        if constexpr (CRC) {
            // ---- CRC-aided choice (polar.py:860-866): every live lane divides its own information decisions
            uint32_t vs[W], zs[W];
            uint32_t zany = 0u;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                vs[w] = PAC ? 0u : c.sm[w];
                zs[w] = c.zm[w];
                zany |= c.zm[w];  // zero decisions arise at information leaves only
            }
            if constexpr (PAC) {
                if (zany == 0u) {
                    const uint64_t u64 = (uint64_t)c.sm[0] | (W > 1 ? (uint64_t)c.sm[W - 1] << 32 : 0ull);
                    const uint64_t v64 = pac_unconv_fast<N>(u64, p.tapmask);
                    vs[0] = (uint32_t)v64;
                    if constexpr (W > 1) vs[W - 1] = (uint32_t)(v64 >> 32);
                } else {
                    uint32_t st = 0u;
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        vs[w] = pac_unconv_word(c.sm[w], c.zm[w], N < 32 ? N : 32, st, p.tapmask, p.smask);
                }
            }
            const uint32_t reg = crc_divide<W, (N < 32 ? N : 32)>(vs, p, a.crc_poly, a.crc_c);
            const bool live = c.j < s_final;
            bool anyp;
            const int bi = crc_choose<G>(c.m, live && reg == 0u && zany == 0u, live, c.j, c.base, anyp);
            const int64_t cwc = row0 + r;
            if (c.j == bi && cwc < a.B) {
                uint32_t mw[4] = {0u, 0u, 0u, 0u};
                if (a.count) {
                    const u32x4 o = philox_block(a.seed, kStreamMsg, a.cw_offset + (uint64_t)cwc, 0u);
                    mw[0] = o.x;
                    mw[1] = o.y;
                    mw[2] = o.z;
                    mw[3] = o.w;
                }
                const uint32_t e = crc_emit<W, (N < 32 ? N : 32), 4>(vs, zs, p, a.msg ? a.msg + cwc * K : nullptr, mw,
                                                                     K - a.crc_c);
                if (a.uhat) {
                    float* urow = a.uhat + cwc * N;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        const uint32_t sb = (c.sm[k >> 5] >> (k & 31)) & 1u, zb = (c.zm[k >> 5] >> (k & 31)) & 1u;
                        urow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                    }
                }
                if (a.crc_ok) a.crc_ok[cwc] = anyp ? 1 : 0;
                err_bits += e;
                err_blocks += e ? 1u : 0u;
                err_crc += anyp ? 0u : 1u;
            }
            continue;
        }

        // ---- ML choice (polar.py:868-874): codeword of each path from its decision bits
        uint32_t S[W], Z[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            S[w] = c.sm[w];
            Z[w] = c.zm[w];
        }
        constexpr uint32_t kLow[5] = {0x55555555u, 0x33333333u, 0x0F0F0F0Fu, 0x00FF00FFu, 0x0000FFFFu};
#pragma unroll
        for (int d = 0; d < (n < 5 ? n : 5); ++d) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                S[w] ^= (S[w] >> (1 << d)) & kLow[d];
                Z[w] |= (Z[w] >> (1 << d)) & kLow[d];
            }
        }
        if constexpr (n == 6) {
            S[0] ^= S[1];
            Z[0] |= Z[1];
        }
        float dist = 0.0f;
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const f4 v = *reinterpret_cast<const f4*>(lds + 16 * (r * C + (q ^ sw)));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * q + e;
                const uint32_t sb = (S[k >> 5] >> (k & 31)) & 1u, zb = (Z[k >> 5] >> (k & 31)) & 1u;
                const float cv = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                const float dd = cv - v[e];
                dist = dist + rmul(dd, dd);
            }
        }
        float bd = c.j < s_final ? dist : __builtin_inff();
        int bi = c.j;
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            const float od = __shfl_xor(bd, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < bd || (od == bd && oi < bi)) {
                bd = od;
                bi = oi;
            }
        }
        const int64_t cw = row0 + r;
        if (c.j == bi && cw < a.B) {
            uint32_t e = 0;
            uint32_t mw[4] = {0u, 0u, 0u, 0u};
            if (a.count) {
                const u32x4 o = philox_block(a.seed, kStreamMsg, a.cw_offset + (uint64_t)cw, 0u);
                mw[0] = o.x;
                mw[1] = o.y;
                mw[2] = o.z;
                mw[3] = o.w;
            }
            float* mrow = a.msg ? a.msg + cw * K : nullptr;
            // message bits: the decisions themselves (Polar) or v_hat, the inverse convolution of u_hat (PAC)
            uint32_t vs[W];
#pragma unroll
            for (int w = 0; w < W; ++w) vs[w] = PAC ? 0u : c.sm[w];
            if constexpr (PAC) {
                uint32_t zany = 0u;
#pragma unroll
                for (int w = 0; w < W; ++w) zany |= c.zm[w];
                if (zany == 0u) {
                    const uint64_t u64 = (uint64_t)c.sm[0] | (W > 1 ? (uint64_t)c.sm[W - 1] << 32 : 0ull);
                    const uint64_t v64 = pac_unconv_fast<N>(u64, p.tapmask);
                    vs[0] = (uint32_t)v64;
                    if constexpr (W > 1) vs[W - 1] = (uint32_t)(v64 >> 32);
                } else {  // a zero decision (l == 0 at an information leaf) does not advance the state
                    uint32_t st = 0u;
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        vs[w] = pac_unconv_word(c.sm[w], c.zm[w], N < 32 ? N : 32, st, p.tapmask, p.smask);
                }
            }
            for (int k = 0; k < K; ++k) {
                const int pos = p.info[k];
                const uint32_t sw0 = W > 1 && pos >= 32 ? vs[W - 1] : vs[0];
                const uint32_t zw0 = W > 1 && pos >= 32 ? c.zm[W - 1] : c.zm[0];
                const uint32_t sb = (sw0 >> (pos & 31)) & 1u, zb = (zw0 >> (pos & 31)) & 1u;
                if (mrow) mrow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                e += ((sb ^ ((mw[k >> 5] >> (k & 31)) & 1u)) | zb);
            }
            if (a.uhat) {
                float* urow = a.uhat + cw * N;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const uint32_t sb = (c.sm[k >> 5] >> (k & 31)) & 1u, zb = (c.zm[k >> 5] >> (k & 31)) & 1u;
                    urow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                }
            }
            err_bits += e;
            err_blocks += e ? 1u : 0u;
        }
    }
    if (a.count) {
        const uint32_t eb = wave_sum_u32(err_bits);
        const uint32_t bl = wave_sum_u32(err_blocks);
        if (lane == 0) {
            atomicAdd(a.counters + 0, (unsigned long long)eb);
            atomicAdd(a.counters + 1, (unsigned long long)bl);
        }
        if constexpr (CRC) {
            const uint32_t cf = wave_sum_u32(err_crc);
            if (lane == 0) atomicAdd(a.counters + 2, (unsigned long long)cf);
        }
    }
}

template <int N, int G, bool PAC, bool CRC = false>
static int launch(const CodeParams& p, Args a, hipStream_t s) {
    constexpr int T = 64 / G;
    const size_t lds = (size_t)T * N * 4;
    a.ntiles = (a.B + T - 1) / T;
    auto kern = scl_kernel<N, G, PAC, CRC>;
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 64, lds) != hipSuccess || occ <= 0) {
        (void)hipGetLastError();
        occ = 1;
    }
    const int grid = grid_for(a.ntiles, occ, device_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, s, p, a);
    return launch_check("scl_kernel launch");
}

template <int N, bool PAC, bool CRC = false>
static int launch_n(const CodeParams& p, const Args& a, hipStream_t s) {
    if (a.L == 1) return launch<N, 1, PAC, CRC>(p, a, s);
    if (a.L == 2) return launch<N, 2, PAC, CRC>(p, a, s);
    if (a.L <= 4) return launch<N, 4, PAC, CRC>(p, a, s);
    return launch<N, 8, PAC, CRC>(p, a, s);
}

// ---------------------------------------------------------------------------------- N >= 128
// The register file cannot hold a path's N-1 internal LLRs at N >= 128 (and a compile-time-unrolled tree
// that large would not fit the instruction cache), so each lane's path state lives in LDS,
// lane-interleaved (element e of lane q at dword e*64 + q: every wave access is bank-conflict free) and
// the SC schedule is walked iteratively (leaf i: one g step at level ctz(i), f steps down to the leaf,
// partial-sum combines for the nodes finished at i).  Per lane:
//   LLR level d = 1..n-1 (2^d values) at rows [2^d - 2, 2^(d+1) - 2); level 0 is a register;
//   bit rows: beta sign | beta zero | decision (u < 0) | decision (u == 0), W = N/32 words each.
// Partial sums are values in {+-1, +-0}: the float sign bit and a zero flag reproduce the reference's
// fp32 products exactly (sign bits XOR, zero flags OR).  The channel level is never stored: the two
// root steps read y through L1/L2 (the G lanes of a codeword read the same row).
// At an information leaf a lane whose slot takes another path's state copies only the LLR levels still
// read later (level D iff leaf i is in the left child of its level-D node) and the bit rows; all lanes
// of the wave read element e before any lane writes it (one instruction stream), so copies between
// lanes of a group need no double buffer.
// N = 256: the top internal level (n-1, the root's two children, 128 values) is not stored but recomputed from y
// (L1/L2) and the path's own partial-sum bits at the four steps that read it (leaves 0, N/4, N/2, 3N/4): 158
// rows = 40 KB of LDS per wave instead of 73 KB, so four waves (one per SIMD) fit a CU instead of two; a path
// switch then never copies that level either.
// Lists of 9 .. 32 paths (G = 16 or 32 lanes per codeword, 4 or 2 codewords per wave) run on this iterative form at
// every N, 8 .. 64 included: a tree unrolled over 64 leaves with a 32-wide selection at each would be several times
// the instruction cache, and here the selection exists once.  What is wider than at G <= 8:
//   the live list size is min(2^min(slot, 5), L), the final one min(2^K, L);
//   the survivor mask has 2s <= 64 bits (one ballot holds it) and list slot j finds its candidate, the j-th set
//   bit, by a popcount bisection (nth_bit64) instead of j clear-lowest-bit steps;
//   rank counting reads the group's 2G candidate metrics from two LDS rows that every lane parks its own pair in
//   (G/2 broadcast 16-byte reads per lane) instead of 2G ds_bpermute;
//   the exact tie rule (rare, out of line) reads the same two rows and keeps its 64 (value, index) pairs in scratch.
template <int N>
struct LdsRows {
    static constexpr int n = log2c<N>();
    static constexpr int W = N >= 32 ? N / 32 : 1;
    static constexpr bool kTopRec = N >= 256;
    static constexpr int kLv = kTopRec ? N / 2 - 2 : N - 2;  // LLR rows (levels 1 .. n-1, or 1 .. n-2)
    static constexpr int kBS = kLv;          // beta sign words
    static constexpr int kBZ = kLv + W;      // beta zero words
    static constexpr int kDS = kLv + 2 * W;  // decision sign words
    static constexpr int kDZ = kLv + 3 * W;  // decision zero words
    static constexpr int kRows = kLv + 4 * W;
    static constexpr int kPark = kRows;      // G >= 16 only: keep metrics | flip metrics, one dword per lane each
    static constexpr int kRowsWide = kRows + 2;
};

// position of the k-th set bit of m (k = 0 is the lowest), or 64 when m has at most k bits set
__device__ __forceinline__ int nth_bit64(uint64_t m, int k) {
    if (k >= __builtin_popcountll(m)) return 64;
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const int cnt = __builtin_popcountll((m >> pos) & ((1ull << w) - 1ull));
        if (k >= cnt) {
            k -= cnt;
            pos += w;
        }
    }
    return pos;
}

// exact_mask for up to 32 paths: the group's metrics are read from the parked rows (PK[lane] keep, PK[64 + lane]
// flip), so nothing is handed over in registers and the common path stores nothing for it
__device__ __noinline__ uint64_t exact_mask64(const float* PK, int bl, int s, int L) {
    float v[64];
    for (int c2 = 0; c2 < s; ++c2) {
        v[c2] = -1.0f * PK[bl + c2];
        v[s + c2] = -1.0f * PK[kWave + bl + c2];
    }
    return nth::prune_mask64(v, 2 * s, L);
}

// list_select for G = 16 / 32: the survivors over [keep_0 .. keep_{s-1}, flip_0 .. flip_{s-1}] as a 64-bit mask
template <int G>
__device__ __forceinline__ uint64_t list_select_wide(float* PK, float m, float a, int j, int bl, int lane, int s,
                                                     int L) {
    static_assert(G == 16 || G == 32, "wide lists take 16 or 32 lanes");
    if (2 * s <= L) return (1ull << (2 * s)) - 1ull;  // 2s <= 32
    const float vk = m, vf = m + a;
    int ltk = 0, lek = 0, ltf = 0, lef = 0;
    PK[lane] = vk;
    PK[kWave + lane] = vf;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < G / 4; ++q) {
        if (4 * q < s) {  // wave-uniform
            const f4 k4 = *reinterpret_cast<const f4*>(PK + bl + 4 * q);
            const f4 f4v = *reinterpret_cast<const f4*>(PK + kWave + bl + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (4 * q + e < s) {
                    ltk += (k4[e] < vk) + (f4v[e] < vk);
                    lek += (k4[e] <= vk) + (f4v[e] <= vk);
                    ltf += (k4[e] < vf) + (f4v[e] < vf);
                    lef += (k4[e] <= vf) + (f4v[e] <= vf);
                }
            }
        }
    }
    const bool act = j < s;
    const bool sk = act && ltk < L;
    const bool sf = act && ltf < L;
    const bool st = act && ((ltk < L && lek > L) || (ltf < L && lef > L));
    const unsigned long long bk = __ballot(sk), bf = __ballot(sf), bs = __ballot(st);
    const uint64_t lowm = (1ull << s) - 1ull;  // s <= 32
    uint64_t msel = ((bk >> bl) & lowm) | (((bf >> bl) & lowm) << s);
    if (bs) {
        const bool mine = ((bs >> bl) & ((1ull << G) - 1ull)) != 0ull;
        if (mine) msel = exact_mask64(PK, bl, s, L);
        __builtin_amdgcn_wave_barrier();
    }
    return msel;
}

__device__ __forceinline__ float beta_val(uint32_t sw, uint32_t zw, int b) {
    return bitsf((((sw >> b) & 1u) << 31) | (((zw >> b) & 1u) ? 0u : 0x3f800000u));
}

// level n-1 of the tree (the root's left child if !right, else its right child), elements x .. x+3 of one
// lane's path: f / g on the channel LLRs (polar.py:805-866 via updateLLR), g with the path's partial sums of
// the root's left half (sign / zero bit words BS / BZ, positions 0 .. N/2-1)
template <int N>
__device__ __forceinline__ f4 top4(const f4* y4, float scale, int x, bool right, const uint32_t* BW, int rowBS,
                                   int rowBZ, int lane) {
    const f4 u = y4[x >> 2], v = y4[(x + N / 2) >> 2];
    f4 o;
    if (!right) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f_minsum_fmin(rmul(scale, u[e]), rmul(scale, v[e]));
    } else {
        const uint32_t sw = BW[(rowBS + (x >> 5)) * kWave + lane], zw = BW[(rowBZ + (x >> 5)) * kWave + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = beta_val(sw, zw, (x + e) & 31) * rmul(scale, u[e]) + rmul(scale, v[e]);
    }
    return o;
}

// PAC: the convolution state is one VGPR per lane (no LDS row: the N = 256 kernel keeps its 158 rows and its four
// waves per CU); after the last leaf the beta sign rows are dead, and the chosen path writes v_hat's sign words there.
template <int N, int G, bool PAC, bool CRC = false>
__global__ __launch_bounds__(64) void scl_lds_kernel(const CodeParams p, const Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    using R = LdsRows<N>;
    constexpr int n = R::n;
    constexpr int W = R::W;
    constexpr int T = 64 / G;
    const int lane = threadIdx.x;
    float* const LV = reinterpret_cast<float*>(lds_raw);
    uint32_t* const BW = reinterpret_cast<uint32_t*>(lds_raw);
#define LVL(row) LV[(row) * kWave + lane]
#define BWL(row) BW[(row) * kWave + lane]
    const int K = p.K;
    const int L = a.L;
    const int j = lane & (G - 1);
    const int base = lane - j;
    const int r = lane / G;
    const int s_final = K >= (G > 8 ? 5 : 3) ? L : ((1 << K) < L ? (1 << K) : L);

    uint32_t err_bits = 0, err_blocks = 0;
    [[maybe_unused]] uint32_t err_crc = 0;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t cw = t * T + r;
        const int64_t cwc = cw < a.B ? cw : a.B - 1;
        const float* yr = a.y + cwc * N;
        const f4* y4 = reinterpret_cast<const f4*>(yr);
#pragma unroll
        for (int w = 0; w < 4 * W; ++w) BWL(R::kBS + w) = 0u;
        float m = 0.0f;
        uint32_t slot = 0;
        uint32_t st = 0u;  // PAC: convolution state (bit t set iff v_{i-1-t} = -1)

        for (int i = 0; i < N; ++i) {
            int d;  // level the f chain starts from
            if (R::kTopRec && (i & (N / 4 - 1)) == 0) {
                // level n-2 from the recomputed level n-1: f at leaves 0 and N/2 (left children), g at N/4 and 3N/4
                constexpr int h2 = N / 4;
                const bool right = i >= N / 2;
                const bool gstep = (i & (N / 2 - 1)) != 0;
                const int s0 = i - h2;  // g: the left sibling's partial sums are bits s0 .. s0 + h2 - 1
                for (int q = 0; q < h2 / 4; ++q) {
                    const f4 A = top4<N>(y4, a.scale, 4 * q, right, BW, R::kBS, R::kBZ, lane);
                    const f4 Bv = top4<N>(y4, a.scale, 4 * q + h2, right, BW, R::kBS, R::kBZ, lane);
                    if (!gstep) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) LVL(h2 - 2 + 4 * q + e) = f_minsum_fmin(A[e], Bv[e]);
                    } else {
                        const int q0 = s0 + 4 * q;
                        const uint32_t sw = BWL(R::kBS + (q0 >> 5)), zw = BWL(R::kBZ + (q0 >> 5));
#pragma unroll
                        for (int e = 0; e < 4; ++e) LVL(h2 - 2 + 4 * q + e) = beta_val(sw, zw, (q0 + e) & 31) * A[e] + Bv[e];
                    }
                }
                d = n - 2;
            } else if (i == 0) {  // left child of the root: f on the channel LLRs
                constexpr int h = N / 2;
                for (int q = 0; q < h / 4; ++q) {
                    const f4 u = y4[q], v = y4[q + h / 4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) LVL(h - 2 + 4 * q + e) = f_minsum_fmin(rmul(a.scale, u[e]), rmul(a.scale, v[e]));
                }
                d = n - 1;
            } else {  // right child of the node of 2^(k+1) leaves starting at i - 2^k
                const int k = __builtin_ctz((unsigned)i);
                const int h = 1 << k;
                const int s0 = i - h;
                if (k == 0) {
                    d = 0;
                } else if (k + 1 == n) {  // right child of the root: g on the channel LLRs
                    for (int q = 0; q < h / 4; ++q) {
                        const uint32_t sw = BWL(R::kBS + (q >> 3)), zw = BWL(R::kBZ + (q >> 3));
                        const f4 u = y4[q], v = y4[q + h / 4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float b = beta_val(sw, zw, (4 * q + e) & 31);
                            LVL(h - 2 + 4 * q + e) = b * rmul(a.scale, u[e]) + rmul(a.scale, v[e]);
                        }
                    }
                    d = k;
                } else {
                    for (int j0 = 0; j0 < h; j0 += 32) {
                        const int q0 = s0 + j0;
                        const uint32_t sw = BWL(R::kBS + (q0 >> 5)) >> (q0 & 31);
                        const uint32_t zw = BWL(R::kBZ + (q0 >> 5)) >> (q0 & 31);
                        const int hw = h < 32 ? h : 32;
                        for (int jj = 0; jj < hw; ++jj) {
                            const float b = beta_val(sw, zw, jj);
                            LVL(h - 2 + j0 + jj) = b * LVL(2 * h - 2 + j0 + jj) + LVL(2 * h - 2 + h + j0 + jj);
                        }
                    }
                    d = k;
                }
            }
            for (int dd = d - 1; dd >= 1; --dd) {  // left children down to level 1
                const int h = 1 << dd;
                for (int jj = 0; jj < h; ++jj) LVL(h - 2 + jj) = f_minsum_fmin(LVL(2 * h - 2 + jj), LVL(2 * h - 2 + h + jj));
            }
            float l;
            if (d == 0) {  // leaf i is a right child: g from level 1 with the left sibling's decision
                const uint32_t sw = BWL(R::kBS + ((i - 1) >> 5)), zw = BWL(R::kBZ + ((i - 1) >> 5));
                l = beta_val(sw, zw, (i - 1) & 31) * LVL(0) + LVL(1);
            } else {
                l = f_minsum_fmin(LVL(0), LVL(1));
            }

            // ---- leaf (polar.py:805-866)
            const bool frozen = (p.frozen[i >> 5] >> (i & 31)) & 1u;
            const int wi = i >> 5;
            const uint32_t bi = 1u << (i & 31);
            if (frozen) {
                if constexpr (PAC) {
                    // u = u0, v = +1 (pac_code.py:545-551); the metric pays |l| unless sign(l) == u0
                    const uint32_t par = pac_par(st, p.tapmask);
                    const bool match = (l != 0.0f) && ((fbits(l) >> 31) == par);
                    m = m + (match ? 0.0f : __builtin_fabsf(l));
                    if (par) {
                        BWL(R::kBS + wi) |= bi;
                        BWL(R::kDS + wi) |= bi;
                    }
                    st = (st << 1) & p.smask;
                } else {
                    m = m + ((l > 0.0f) ? 0.0f : __builtin_fabsf(l));  // |l| * (sign(l) != 1), polar.py:814
                    // u = +1: beta sign/zero bits stay clear
                }
            } else {
                const float av = __builtin_fabsf(l);
                const int s = slot >= (G > 8 ? 5u : 3u) ? L : ((1 << slot) < L ? (1 << slot) : L);
                float u;
                if constexpr (G > 8) {
                    const uint64_t msel = list_select_wide<G>(LV + R::kPark * kWave, m, av, j, base, lane, s, L);
                    // list slot j takes the j-th surviving candidate (list order); a slot past the last keeps itself
                    const int cidx = nth_bit64(msel, j);
                    const bool flip = cidx < 64 && cidx >= s;
                    const int srcj = flip ? cidx - s : (cidx < 64 ? cidx : j);
                    const int src = base + srcj;
                    const float ls = __shfl(l, src, 64);
                    const float ms = __shfl(m, src, 64);
                    if constexpr (PAC) st = (uint32_t)__shfl((int)st, src, 64);
                    if (src != lane) {
                        for (int D = 1; D < (R::kTopRec ? n - 1 : n); ++D) {
                            if ((i >> (D - 1)) & 1) continue;
                            const int b0 = (1 << D) - 2;
                            for (int e = 0; e < (1 << D); ++e) LV[(b0 + e) * kWave + lane] = LV[(b0 + e) * kWave + src];
                        }
#pragma unroll
                        for (int w = 0; w < 4 * W; ++w) BW[(R::kBS + w) * kWave + lane] = BW[(R::kBS + w) * kWave + src];
                    }
                    u = sgn_bits(ls);
                    if (flip) u = -u;
                    m = flip ? ms + __builtin_fabsf(ls) : ms;
                } else if constexpr (G == 1) {
                    u = sgn_bits(l);  // L = 1: plain SC with the metric tracked (pruning keeps the smaller one)
                    const uint32_t msel = list_select<G>(m, av, j, base, s, L);
                    if (!(msel & 1u)) {
                        u = -u;
                        m = m + av;
                    }
                } else {
                    const uint32_t msel = list_select<G>(m, av, j, base, s, L);
                    uint32_t mm = msel;
#pragma unroll
                    for (int q = 0; q < G - 1; ++q)
                        if (q < j) mm &= mm - 1u;
                    const int cidx = mm ? __builtin_ctz(mm) : j;
                    const bool flip = mm ? (cidx >= s) : false;
                    const int srcj = flip ? cidx - s : (mm ? cidx : j);
                    const int src = base + srcj;
                    const float ls = __shfl(l, src, 64);
                    const float ms = __shfl(m, src, 64);
                    if constexpr (PAC) st = (uint32_t)__shfl((int)st, src, 64);
                    if (src != lane) {
                        // live LLR levels: D in 1..n-1 with leaf i in the left child of its level-D node
                        for (int D = 1; D < (R::kTopRec ? n - 1 : n); ++D) {
                            if ((i >> (D - 1)) & 1) continue;
                            const int b0 = (1 << D) - 2;
                            for (int e = 0; e < (1 << D); ++e) LV[(b0 + e) * kWave + lane] = LV[(b0 + e) * kWave + src];
                        }
#pragma unroll
                        for (int w = 0; w < 4 * W; ++w) BW[(R::kBS + w) * kWave + lane] = BW[(R::kBS + w) * kWave + src];
                    }
                    u = sgn_bits(ls);
                    if (flip) u = -u;
                    m = flip ? ms + __builtin_fabsf(ls) : ms;
                }
                if constexpr (PAC) {
                    // v = u * u0 enters the state; u = 0 (from l = 0) leaves it alone (pac_code.py:553-568)
                    const uint32_t negv = (u < 0.0f ? 1u : 0u) ^ pac_par(st, p.tapmask);
                    const uint32_t sh = ((st << 1) | negv) & p.smask;
                    st = (u == 0.0f) ? st : sh;
                }
                if (fbits(u) >> 31) BWL(R::kBS + wi) |= bi;
                if (u == 0.0f) BWL(R::kBZ + wi) |= bi;
                if (u < 0.0f) BWL(R::kDS + wi) |= bi;
                if (u == 0.0f) BWL(R::kDZ + wi) |= bi;
                slot = slot + 1u;
            }
            // ---- partial sums of the nodes whose right child ends at leaf i (the right spine is never read)
            if (i != N - 1) {
                for (int l2 = 0; (i >> l2) & 1; ++l2) {
                    const int h = 1 << l2;
                    const int s0 = i + 1 - 2 * h;
                    if (h < 32) {
                        const int w = s0 >> 5, o = s0 & 31;
                        const uint32_t lowm = (1u << h) - 1u;
                        uint32_t sw = BWL(R::kBS + w), zw = BWL(R::kBZ + w);
                        sw ^= ((sw >> (o + h)) & lowm) << o;
                        zw |= ((zw >> (o + h)) & lowm) << o;
                        BWL(R::kBS + w) = sw;
                        BWL(R::kBZ + w) = zw;
                    } else {
                        const int w0 = s0 >> 5, hw = h >> 5;
                        for (int q = 0; q < hw; ++q) {
                            BWL(R::kBS + w0 + q) ^= BWL(R::kBS + w0 + hw + q);
                            BWL(R::kBZ + w0 + q) |= BWL(R::kBZ + w0 + hw + q);
                        }
                    }
                }
            }
        }

        if constexpr (CRC) {
            // ---- CRC-aided choice (polar.py:860-866): every live lane divides its own information decisions
            uint32_t us[W], vs[W], zs[W];
            uint32_t zany = 0u;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                us[w] = BWL(R::kDS + w);
                zs[w] = BWL(R::kDZ + w);
                vs[w] = us[w];
                zany |= zs[w];  // zero decisions arise at information leaves only
            }
            if constexpr (PAC) {
                uint32_t cs = 0u;
#pragma unroll
                for (int w = 0; w < W; ++w) vs[w] = pac_unconv_word(us[w], zs[w], 32, cs, p.tapmask, p.smask);
            }
            const uint32_t reg = crc_divide<W, (N < 32 ? N : 32)>(vs, p, a.crc_poly, a.crc_c);
            const bool live = j < s_final;
            bool anyp;
            const int bj = crc_choose<G>(m, live && reg == 0u && zany == 0u, live, j, base, anyp);
            if (j == bj && cw < a.B) {
                uint32_t mw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                if (a.count) {
#pragma unroll
                    for (int blk = 0; blk < 2; ++blk) {
                        if (blk * 128 < K) {
                            const u32x4 o = philox_block(a.seed, kStreamMsg, a.cw_offset + (uint64_t)cw, (uint32_t)blk);
                            mw[4 * blk + 0] = o.x;
                            mw[4 * blk + 1] = o.y;
                            mw[4 * blk + 2] = o.z;
                            mw[4 * blk + 3] = o.w;
                        }
                    }
                }
                const uint32_t e = crc_emit<W, (N < 32 ? N : 32), 8>(vs, zs, p, a.msg ? a.msg + cw * K : nullptr, mw,
                                                                     K - a.crc_c);
                if (a.uhat) {
                    float* urow = a.uhat + cw * N;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        const uint32_t sb = (us[k >> 5] >> (k & 31)) & 1u, zb = (zs[k >> 5] >> (k & 31)) & 1u;
                        urow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                    }
                }
                if (a.crc_ok) a.crc_ok[cw] = anyp ? 1 : 0;
                err_bits += e;
                err_blocks += e ? 1u : 0u;
                err_crc += anyp ? 0u : 1u;
            }
            continue;
        }

        // ---- ML choice (polar.py:868-874): codeword of each path from its decision bits
        uint32_t S[W], Z[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            S[w] = BWL(R::kDS + w);
            Z[w] = BWL(R::kDZ + w);
        }
        constexpr uint32_t kLow[5] = {0x55555555u, 0x33333333u, 0x0F0F0F0Fu, 0x00FF00FFu, 0x0000FFFFu};
#pragma unroll
        for (int dd = 0; dd < 5; ++dd) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                S[w] ^= (S[w] >> (1 << dd)) & kLow[dd];
                Z[w] |= (Z[w] >> (1 << dd)) & kLow[dd];
            }
        }
#pragma unroll
        for (int dd = 5; dd < n; ++dd) {
            const int st = 1 << (dd - 5);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if ((w & st) == 0) {
                    S[w] ^= S[w + st];
                    Z[w] |= Z[w + st];
                }
            }
        }
        float dist = 0.0f;
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f4 v = y4[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * q + e;
                const uint32_t sb = (S[k >> 5] >> (k & 31)) & 1u, zb = (Z[k >> 5] >> (k & 31)) & 1u;
                const float cv = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                const float dd = cv - v[e];
                dist = dist + rmul(dd, dd);
            }
        }
        float bd = j < s_final ? dist : __builtin_inff();
        int bj = j;
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            const float od = __shfl_xor(bd, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (od < bd || (od == bd && oj < bj)) {
                bd = od;
                bj = oj;
            }
        }
        if (j == bj && cw < a.B) {
            uint32_t e = 0;
            uint32_t mw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            if (a.count) {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    if (blk * 128 < K) {
                        const u32x4 o = philox_block(a.seed, kStreamMsg, a.cw_offset + (uint64_t)cw, (uint32_t)blk);
                        mw[4 * blk + 0] = o.x;
                        mw[4 * blk + 1] = o.y;
                        mw[4 * blk + 2] = o.z;
                        mw[4 * blk + 3] = o.w;
                    }
                }
            }
            float* mrow = a.msg ? a.msg + cw * K : nullptr;
            // message bits: the decisions themselves (Polar) or v_hat, the inverse convolution of u_hat (PAC),
            // whose sign words go to the beta sign rows (dead after the last leaf)
            constexpr int kMS = PAC ? R::kBS : R::kDS;
            if constexpr (PAC) {
                uint32_t cs = 0u;
                for (int w = 0; w < W; ++w)
                    BWL(R::kBS + w) = pac_unconv_word(BWL(R::kDS + w), BWL(R::kDZ + w), 32, cs, p.tapmask, p.smask);
            }
            for (int k = 0; k < K; ++k) {
                const int pos = p.info[k];
                const uint32_t sb = (BWL(kMS + (pos >> 5)) >> (pos & 31)) & 1u;
                const uint32_t zb = (BWL(R::kDZ + (pos >> 5)) >> (pos & 31)) & 1u;
                if (mrow) mrow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                e += ((sb ^ ((mw[k >> 5] >> (k & 31)) & 1u)) | zb);
            }
            if (a.uhat) {
                float* urow = a.uhat + cw * N;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const uint32_t sb = (BWL(R::kDS + (k >> 5)) >> (k & 31)) & 1u;
                    const uint32_t zb = (BWL(R::kDZ + (k >> 5)) >> (k & 31)) & 1u;
                    urow[k] = zb ? 0.0f : (sb ? -1.0f : 1.0f);
                }
            }
            err_bits += e;
            err_blocks += e ? 1u : 0u;
        }
    }
#undef LVL
#undef BWL
    if (a.count) {
        const uint32_t eb = wave_sum_u32(err_bits);
        const uint32_t bl = wave_sum_u32(err_blocks);
        if (lane == 0) {
            atomicAdd(a.counters + 0, (unsigned long long)eb);
            atomicAdd(a.counters + 1, (unsigned long long)bl);
        }
        if constexpr (CRC) {
            const uint32_t cf = wave_sum_u32(err_crc);
            if (lane == 0) atomicAdd(a.counters + 2, (unsigned long long)cf);
        }
    }
}

template <int N, int G, bool PAC, bool CRC = false>
static int launch_lds(const CodeParams& p, Args a, hipStream_t s) {
    constexpr int T = 64 / G;
    const size_t lds = (size_t)(G > 8 ? LdsRows<N>::kRowsWide : LdsRows<N>::kRows) * kWave * sizeof(float);
    a.ntiles = (a.B + T - 1) / T;
    auto kern = scl_lds_kernel<N, G, PAC, CRC>;
    static bool attr_set = false;  // benign race (idempotent)
    if (!attr_set && lds > 65536) {
        NPD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
        attr_set = true;
    }
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 64, lds) != hipSuccess || occ <= 0) {
        (void)hipGetLastError();
        occ = 1;
    }
    const int grid = grid_for(a.ntiles, occ, device_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, s, p, a);
    return launch_check("scl_lds_kernel launch");
}

template <int N, bool PAC, bool CRC = false>
static int launch_lds_n(const CodeParams& p, const Args& a, hipStream_t s) {
    if (a.L == 1) return launch_lds<N, 1, PAC, CRC>(p, a, s);
    if (a.L == 2) return launch_lds<N, 2, PAC, CRC>(p, a, s);
    if (a.L <= 4) return launch_lds<N, 4, PAC, CRC>(p, a, s);
    return launch_lds<N, 8, PAC, CRC>(p, a, s);
}

// the kernel for p.N (8 .. 256, checked by the caller) and a.L (1 .. 8; larger lists go to dispatch_wide)
template <bool PAC, bool CRC = false>
static int dispatch(const CodeParams& p, const Args& a, hipStream_t s) {
    switch (p.N) {
        case 8: return launch_n<8, PAC, CRC>(p, a, s);
        case 16: return launch_n<16, PAC, CRC>(p, a, s);
        case 32: return launch_n<32, PAC, CRC>(p, a, s);
        case 64: return launch_n<64, PAC, CRC>(p, a, s);
        case 128: return launch_lds_n<128, PAC, CRC>(p, a, s);
        default: return launch_lds_n<256, PAC, CRC>(p, a, s);
    }
}

// the kernel for p.N (8 .. 256) and a.L (9 .. 32): G = 16 up to 16 paths, G = 32 above
template <int N, bool PAC, bool CRC = false>
static int launch_wide_n(const CodeParams& p, const Args& a, hipStream_t s) {
    if (a.L <= 16) return launch_lds<N, 16, PAC, CRC>(p, a, s);
    return launch_lds<N, 32, PAC, CRC>(p, a, s);
}

template <bool PAC, bool CRC = false>
static int dispatch_wide(const CodeParams& p, const Args& a, hipStream_t s) {
    switch (p.N) {
        case 8: return launch_wide_n<8, PAC, CRC>(p, a, s);
        case 16: return launch_wide_n<16, PAC, CRC>(p, a, s);
        case 32: return launch_wide_n<32, PAC, CRC>(p, a, s);
        case 64: return launch_wide_n<64, PAC, CRC>(p, a, s);
        case 128: return launch_wide_n<128, PAC, CRC>(p, a, s);
        default: return launch_wide_n<256, PAC, CRC>(p, a, s);
    }
}

// npd_scl_pac.hip: the PAC instantiations (arguments already checked by run())
int run_pac(const CodeParams& p, const Args& a, hipStream_t s);
// npd_scl_wide.hip / npd_scl_pac_wide.hip: list sizes 9 .. 32, Polar / PAC
int run_wide(const CodeParams& p, const Args& a, hipStream_t s);
int run_pac_wide(const CodeParams& p, const Args& a, hipStream_t s);
// npd_scl_crc_pac.hip / npd_scl_crc_wide.hip / npd_scl_crc_pac_wide.hip: the CRC-aided instantiations other than
// Polar with 1 .. 8 paths (those are in npd_scl_crc.hip, with the C ABI)
int run_crc_pac(const CodeParams& p, const Args& a, hipStream_t s);
int run_crc_wide(const CodeParams& p, const Args& a, hipStream_t s);
int run_crc_pac_wide(const CodeParams& p, const Args& a, hipStream_t s);

}  // namespace scl
}  // namespace npd

// npd_gru_split.hip -- the split 16-bit MFMA paths on 32-codeword waves (gru_decode_bf_kernel: F <= 64, precisions 1-3;
// the design is described in npd_gru_split.hpp).  F = 64 x 2 with N % 32 == 0 runs npd_gru_split16.hip instead.
#include "npd_gru_split.hpp"

namespace npd {
namespace gru {

template <int F, int L, int SPLIT>
struct GeoB {
    static constexpr int TT = 3 * F / 32, HT = F / 32, KB = F / 16;
    static constexpr int NG = (L == 2) ? 3 : 1;
    static constexpr int IMG = NG * TT * KB * 64 * 4;  // floats: one 16-B bf16x8 fragment per lane per step
    static constexpr int NS = SPLIT >= 3 ? 2 : 1;      // hi (+ lo) images
    static constexpr int OFF_X = NS * IMG;
    static constexpr int OFF_IN = OFF_X + NG * TT * 64;
    static constexpr int OFF_WL = OFF_IN + HT * 64;
    static constexpr int TOTAL = OFF_WL + 2 * HT * 16;
};

__device__ __forceinline__ f16v mfma16(const bf8& a, const bf8& b, const f16v& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f16v mfma16(const hf8& a, const hf8& b, const f16v& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// the gate pre-activations arrive as ACC x their value (ACC a power of 2): folded into the exp2 constants
template <int SPLIT>
__device__ __forceinline__ void gru_update_fast(f16v& h, const f16v& ar, const f16v& az, const f16v& ain,
                                                const f16v& ahn) {
    constexpr float c1 = SplitT<SPLIT>::kC1, c2 = SplitT<SPLIT>::kC2;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(c1 * ar[i]));
        const float z = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(c1 * az[i]));
        const float x = ain[i] + ahn[i] * r;
        const float nn = fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(c2 * x)), -1.0f);
        h[i] = (h[i] - nn) * z + nn;
    }
}

// split the state tiles into 16-bit B fragments (hi and, for SPLIT 3 / 4, lo)
template <int HT, int SPLIT>
__device__ __forceinline__ void to_frags(const f16v (&h)[HT], typename SplitT<SPLIT>::V (&hi)[2 * HT],
                                         typename SplitT<SPLIT>::V (&lo)[2 * HT]) {
    using S = SplitT<SPLIT>;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = h[t][8 * s + j] * S::kIn;
                const typename S::E b = (typename S::E)v;
                hi[2 * t + s][j] = b;
                if (S::kLo) lo[2 * t + s][j] = (typename S::E)(v - (float)b);
            }
}

template <int TT, int KB, int NT, int SPLIT, int IMG>
__device__ __forceinline__ void gemm_bf(const f4* __restrict__ smem4, int g, int t0, int lane, f16v (&acc)[NT],
                                        const typename SplitT<SPLIT>::V (&hi)[KB],
                                        const typename SplitT<SPLIT>::V (&lo)[KB]) {
    using V = typename SplitT<SPLIT>::V;
#pragma unroll
    for (int q = 0; q < KB; ++q) {
        V ah[NT], al[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const f4 v = smem4[((g * TT + t0 + t) * KB + q) * 64 + lane];
            ah[t] = __builtin_bit_cast(V, v);
            if (SplitT<SPLIT>::kLo)
                al[t] = __builtin_bit_cast(V, smem4[IMG / 4 + ((g * TT + t0 + t) * KB + q) * 64 + lane]);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = mfma16(ah[t], hi[q], acc[t]);
            if (SplitT<SPLIT>::kLo) {
                acc[t] = mfma16(ah[t], lo[q], acc[t]);
                acc[t] = mfma16(al[t], hi[q], acc[t]);
            }
        }
    }
}

template <int F, int L, int SPLIT>
__global__ __launch_bounds__(64 * NPD_GRU_BF_WPB) void gru_decode_bf_kernel(const ArgsB a) {
    using G = GeoB<F, L, SPLIT>;
    using S = SplitT<SPLIT>;
    using V = typename S::V;
    using E = typename S::E;
    constexpr int TT = G::TT, HT = G::HT, KB = G::KB, IMG = G::IMG;
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
    const int64_t ntiles = (a.B + 31) / 32;
    const f16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float one_or_zero = half ? 0.0f : 1.0f;

    for (int64_t tile = (int64_t)blockIdx.x * NPD_GRU_BF_WPB + wave; tile < ntiles;
         tile += (int64_t)gridDim.x * NPD_GRU_BF_WPB) {
        const int64_t cw = tile * 32 + col;
        const bool valid = cw < a.B;
        const int64_t cwc = valid ? cw : a.B - 1;
        // ---- P = W_ih0[:, :N] . y ; k-step q covers y[16q + 8*half .. +7]
        f16v P[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) P[t] = zero;
        {
            const float* yr = a.y + cwc * N;
            const int nq = N / 16;
            for (int q = 0; q < nq; ++q) {
                const f4 y0 = *reinterpret_cast<const f4*>(yr + 16 * q + 8 * half);
                const f4 y1 = *reinterpret_cast<const f4*>(yr + 16 * q + 8 * half + 4);
                V yh, yl;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = (j < 4 ? y0[j] : y1[j - 4]) * S::kIn;
                    yh[j] = (E)v;
                    if (S::kLo) yl[j] = (E)(v - (float)yh[j]);
                }
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    const V wh = __builtin_bit_cast(V, a.wy[(t * nq + q) * 64 + lane]);
                    P[t] = mfma16(wh, yh, P[t]);
                    if (S::kLo) {
                        const V wl = __builtin_bit_cast(V, a.wy[a.wy_lo + (t * nq + q) * 64 + lane]);
                        P[t] = mfma16(wh, yl, P[t]);
                        P[t] = mfma16(wl, yh, P[t]);
                    }
                }
            }
        }
        f16v h0[HT], h1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            h0[t] = zero;
            h1[t] = zero;
        }
        float xb = 1.0f;
        // B fragments of h0: split once per update, used by layer 1 of this step and layer 0 of the next
        V fh[KB], fl[KB];
        to_frags<HT, SPLIT>(h0, fh, fl);
        for (int ii = 0; ii < N; ++ii) {
            const int jj = a.rev ? N - 1 - ii : ii;
            const float xbe = half ? xb : 1.0f;
            {
                f16v acc[TT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) acc[t] = P[t];
#pragma unroll
                for (int t = 2 * HT; t < TT; ++t) acc[t] = zero;
                gemm_bf<TT, KB, TT, SPLIT, IMG>(smem4, 0, 0, lane, acc, fh, fl);
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t] = mfma(smem[G::OFF_X + t * 64 + lane], xbe, acc[t]);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    const f16v ain = mfma(smem[G::OFF_IN + j * 64 + lane], xbe, P[2 * HT + j]);
                    gru_update_fast<SPLIT>(h0[j], acc[j], acc[HT + j], ain, acc[2 * HT + j]);
                }
            }
            if constexpr (L == 1) to_frags<HT, SPLIT>(h0, fh, fl);
            if constexpr (L == 2) {
                V gh[KB], gl[KB];
                to_frags<HT, SPLIT>(h0, fh, fl);
                to_frags<HT, SPLIT>(h1, gh, gl);
                f16v acc1[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc1[t] = zero;
                gemm_bf<TT, KB, TT, SPLIT, IMG>(smem4, 1, 0, lane, acc1, fh, fl);
#pragma unroll
                for (int t = 0; t < TT; ++t) acc1[t] = mfma(smem[G::OFF_X + (TT + t) * 64 + lane], one_or_zero, acc1[t]);
                f16v arz[2 * HT];
#pragma unroll
                for (int t = 0; t < 2 * HT; ++t) arz[t] = acc1[t];
                gemm_bf<TT, KB, 2 * HT, SPLIT, IMG>(smem4, 2, 0, lane, arz, gh, gl);
                f16v ahn[HT];
#pragma unroll
                for (int j = 0; j < HT; ++j) ahn[j] = zero;
                gemm_bf<TT, KB, HT, SPLIT, IMG>(smem4, 2, 2 * HT, lane, ahn, gh, gl);
#pragma unroll
                for (int j = 0; j < HT; ++j) {
                    ahn[j] = mfma(smem[G::OFF_X + (2 * TT + 2 * HT + j) * 64 + lane], one_or_zero, ahn[j]);
                    gru_update_fast<SPLIT>(h1[j], arz[j], arz[HT + j], acc1[2 * HT + j], ahn[j]);
                }
            }
            float part = 0.0f;
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    part += smem[G::OFF_WL + (half * HT + t) * 16 + i] * (L == 2 ? h1[t][i] : h0[t][i]);
            const float out = part + __shfl_xor(part, 32, 64) + a.b_lin;
            const bool info = (a.info[jj >> 5] >> (jj & 31)) & 1u;
            float d;
            if (info) d = out > 0.0f ? 1.0f : (out < 0.0f ? -1.0f : 0.0f);
            else d = a.gt ? a.gt[cwc * N + jj] : 1.0f;
            if (half == 0 && valid) {
                a.decoded[cw * N + jj] = d;
                if (a.logits) a.logits[cw * N + ii] = out;
            }
            const float sd = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            xb = a.onehot ? (sd > 0.0f ? 1.0f : 0.0f) : sd;
        }
    }
}

// img: fp32 image of GeoB (bf16 fragments stored as raw bytes inside the float array)
template <int F, int L, int SPLIT>
static void build_image_bf(const float* W, int N, int onehot, std::vector<float>& img, std::vector<float>& wy,
                           float& b_lin, int64_t& wy_lo) {
    using GB = GeoB<F, L, SPLIT>;
    using G32 = Geo<F, L>;
    constexpr int TT = GB::TT, HT = GB::HT, KB = GB::KB;
    // reuse the fp32 builder for the extra / input / linear constants
    std::vector<float> img32, wy32;
    build_image(F, L, W, N, onehot, false, img32, wy32, b_lin);
    img.assign(GB::TOTAL, 0.0f);
    const int Din = N + (onehot ? 2 : 1);
    const Weights u = unpack_weights(W, 3, F, L, Din);
    uint16_t* u16 = reinterpret_cast<uint16_t*>(img.data());
    for (int g = 0; g < GB::NG; ++g)
        for (int t = 0; t < TT; ++t)
            for (int q = 0; q < KB; ++q)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int row = 32 * t + (l & 31), hh = l >> 5;
                        const int th = q >> 1, s = q & 1;
                        const int colk = 32 * th + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3);
                        const float v = u.mats[g][(size_t)row * F + colk];
                        uint16_t hi, lo;
                        split16<SPLIT>(v, hi, lo);
                        const size_t e = ((((size_t)(g * TT + t) * KB + q) * 64 + l) * 8 + j);
                        u16[e] = hi;
                        if (SPLIT >= 3) u16[(size_t)GB::IMG * 2 + e] = lo;
                    }
    // the [1, x] k-step constants enter the accumulators directly: x 2^16 for the scaled fp16 split
    const float kc = SPLIT == 4 ? 65536.0f : 1.0f;
    for (int i = 0; i < GB::NG * TT * 64; ++i) img[GB::OFF_X + i] = img32[G32::OFF_X + i] * kc;
    for (int i = 0; i < HT * 64; ++i) img[GB::OFF_IN + i] = img32[G32::OFF_IN + i] * kc;
    for (int i = 0; i < 2 * HT * 16; ++i) img[GB::OFF_WL + i] = img32[G32::OFF_WL + i];
    // y projection fragments: k-step q pairs lanes' y[16q + 8h + j]
    wy_lo = fill_wy16<SPLIT>(u.wih[0], TT, 32, N, Din, [](int) { return 1.0f; }, wy);
}

// fn(IC<F>, IC<L>, IC<SPLIT>) for a split handle's shape and precision
template <typename Fn>
static int dispatch_bf(const npd_gru& g, Fn&& fn) {
    return dispatch(NarrowShapes{}, [&](auto f, auto l) {
        return dispatch(Combos<Combo<3>, Combo<4>, Combo<1>>{}, [&](auto sp) { return fn(f, l, sp); },
                        split_of(g.precision, false));
    }, g.F, g.layers);
}

void build_image_split(npd_gru& g, const float* W, HostImages& im) {
    dispatch_bf(g, [&](auto f, auto l, auto sp) {
        build_image_bf<f.value, l.value, sp.value>(W, g.N, g.onehot, im.img, im.wy, g.b_lin, g.wy_lo);
    });
}

int launch_split(const npd_gru* g, const Args& a, hipStream_t s) {
    const ArgsB b = make_args_b(g, a);
    if (g->img16) return launch_split16(g, b, s);
    const int grid = grid_for(((b.B + 31) / 32 + NPD_GRU_BF_WPB - 1) / NPD_GRU_BF_WPB, 1, device_cu_count());
    return dispatch_bf(*g, [&](auto f, auto l, auto sp) {
        return launch_lds<gru_decode_bf_kernel<f.value, l.value, sp.value>>(
            "gru_decode_bf_kernel launch", grid, 64 * NPD_GRU_BF_WPB,
            (size_t)GeoB<f.value, l.value, sp.value>::TOTAL * 4, s, b);
    });
}

}  // namespace gru
}  // namespace npd

// npd_conv_slab.hip -- conv model, fp16x3: the slab kernel for the layer widths the weight-stationary kernels do not
// take (cin 72 and up other than 128).
#include <type_traits>

#include "npd_conv_host.hpp"

namespace npd {
namespace conv {

// ------------------------------------------------------------------------------ conv layer, fp16x3
// precision 3 (cin > 1): the same implicit GEMM on v_mfma_f32_32x32x16_f16 with hi + lo fp16 operands, three
// products per multiply (hi.hi + hi.lo + lo.hi), fp32 accumulation -- 16 channels of one tap per MFMA triple instead
// of 8 fp32 MFMAs of 2 channels: 96 against 512 MFMA cycles per tap-group.  32x32x16 operand map (lane l, r = l&31,
// h = l>>5): A[row r][k = 8h + j], B[k = 8h + j][col r], j = 0..7; k-step s of tap t covers channels 16s + k.
// The slab is split once when staged: LDS holds a hi plane and a lo plane of fp16 rows [position][channel] of stride
// CSH = cin16 + 8 (cin16 = cin rounded up to 16, the pad channels zero), so a B fragment (8 channels) is one
// ds_read_b128 per plane.  Each wave owns 32 output channels x P position tiles: an A fragment pair (global, 2 x 16 B)
// feeds P MFMA triples, which divides the weight stream by P.  Block: 2 (co) x 2 (position) waves, 64 P positions.
// Epilogue (registers 4q..4q+3 = 4 consecutive channels, as conv_layer_kernel) after the exact descale 2^-(SW+SA).
template <int P>
__global__ __launch_bounds__(256) void conv_layer_split_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               const float* __restrict__ res, const f4* __restrict__ wimg,
                                                               const float* __restrict__ bias, int cin, int cout, int N,
                                                               int dil, int do_res, int sw,
                                                               const uint32_t* __restrict__ amax_in,
                                                               uint32_t* __restrict__ amax_out) {
    extern __shared__ __attribute__((aligned(16))) _Float16 slab16[];
    const int sa = split_sa(amax_in);
    const float sa_scale = __builtin_ldexpf(1.0f, sa), descale = __builtin_ldexpf(1.0f, -(sw + sa));
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    constexpr int PT = 64 * P;  // positions per block
    const int l0 = blockIdx.x * PT;
    const int64_t b = blockIdx.z;
    const int halo = 3 * dil;
    const int W = PT + 2 * halo;
    const int cin16 = (cin + 15) & ~15;
    const int CSH = cin16 + 8;
    _Float16* const hiP = slab16;
    _Float16* const loP = slab16 + (size_t)W * CSH;
    {
        // stage + split: 4 channels per element (cin is a multiple of 8), pad channels of each row zeroed
        const int c4n = cin >> 2, c4p = cin16 >> 2;
        const f4* inb = reinterpret_cast<const f4*>(in + b * (int64_t)N * cin);
        for (int e = tid; e < W * c4p; e += 256) {
            const int p = e / c4p, c4 = e - p * c4p;
            const int l = l0 - halo + p;
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if (c4 < c4n && l >= 0 && l < N) v = inb[(int64_t)l * c4n + c4];
            hf4 hi, lo;  // written out, not split4(): with the helper P = 2's registers are allocated differently
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = v[j] * sa_scale;
                hi[j] = (_Float16)x;
                lo[j] = (_Float16)(x - (float)hi[j]);
            }
            *reinterpret_cast<hf4*>(hiP + p * CSH + 4 * c4) = hi;
            *reinterpret_cast<hf4*>(loP + p * CSH + 4 * c4) = lo;
        }
    }
    __syncthreads();
    const int co_sub = wave & 1, pos_sub = wave >> 1;
    const int co_t32 = blockIdx.y * 2 + co_sub;  // 32-channel tile index
    const int ng = cin16 >> 4;                   // 16-channel k-steps per tap
    f16v acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = f16v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // A fragments: [t32][tap][s][part][lane] 16 B
    const f4* wq = wimg + (int64_t)co_t32 * 7 * ng * 128 + lane;
    f4 whn = wq[0], wln = wq[64];
    const int pbase = pos_sub * 32 * P + col;  // this lane's position column within the block, tile 0
    float amx = 0.0f;
    for (int t = 0; t < 7; ++t) {
        for (int g = 0; g < ng; ++g) {
            const hf8 ah = __builtin_bit_cast(hf8, whn), al = __builtin_bit_cast(hf8, wln);
            const int nxt = t * ng + g + 1;
            if (nxt < 7 * ng) {
                whn = wq[(int64_t)nxt * 128];
                wln = wq[(int64_t)nxt * 128 + 64];
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int off = (pbase + 32 * p + dil * t) * CSH + 16 * g + 8 * h;
                const hf8 bh = *reinterpret_cast<const hf8*>(hiP + off);
                const hf8 bl = *reinterpret_cast<const hf8*>(loP + off);
                acc[p] = mfma16(ah, bh, acc[p]);
                acc[p] = mfma16(ah, bl, acc[p]);
                acc[p] = mfma16(al, bh, acc[p]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int l = l0 + pos_sub * 32 * P + 32 * p + col;
        if (l >= N) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = co_t32 * 32 + 8 * q + 4 * h;
            if (co < cout) {
                const int64_t o = (b * N + l) * (int64_t)cout + co;
                const f4 bb = *reinterpret_cast<const f4*>(bias + co);
                f4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = gelu(fmaf(acc[p][4 * q + e], descale, bb[e]));
                if (do_res) {
                    const f4 rv = *reinterpret_cast<const f4*>(res + o);
                    v += rv;
                }
                *reinterpret_cast<f4*>(out + o) = v;
                amx = fmaxf(amx, amax4(v));
            }
        }
    }
    if (amax_out != nullptr) publish_amax(amax_out, amx);
}

// ------------------------------------------------------------------------------ host
int launch_conv_slab(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    const int P = L.q;
    const dim3 grid((a.N + 64 * P - 1) / (64 * P), (L.cout + 63) / 64, (unsigned)a.nb);
    auto go = [&](auto p) {
        return launch_lds<conv_layer_split_kernel<decltype(p)::value>>(
            "conv_layer_split_kernel launch", grid, 256, slab_lds_bytes(L.cin, P, L.dil), s, a.in, a.out, a.res,
            reinterpret_cast<const f4*>(a.img + L.woff), a.img + L.boff, L.cin, L.cout, a.N, L.dil, L.res, L.sw, a.am_in,
            a.am_out);
    };
    if (P == 1) return go(std::integral_constant<int, 1>{});
    if (P == 2) return go(std::integral_constant<int, 2>{});
    return fail(NPD_ENOTSUP, "npd_conv: no conv_layer_split_kernel for this plan");
}

}  // namespace conv
}  // namespace npd

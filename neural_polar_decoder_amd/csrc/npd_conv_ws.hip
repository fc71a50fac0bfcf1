// npd_conv_ws.hip -- conv model, fp16x3: the weight-stationary kernels, conv_split_ws_kernel on 32-row MFMA tiles (cin <=
// 56 other than 32) and conv_ws16_kernel on 16-row tiles (cin 32, 64, 128).
#include "npd_conv_host.hpp"

namespace npd {
namespace conv {

// ------------------------------------------------------------------------------ conv layer, fp16x3, weight-stationary
// The same products as conv_layer_split_kernel, reorganised so that nothing but activations streams: a persistent
// block (one per CU) keeps its waves' weight slices in registers for the whole layer and walks (codeword, 64 Q-position
// chunk) items.  NW waves = 2 (32 output channels each) x KS channel parts x NW / 2 / KS position parts; a wave holds
// 32 channels x 7 taps x NG / KS 16-channel groups, hi and lo (56 NG / KS VGPRs).  Every instantiation in use has
// NW = 4: KS = 1 for cin <= 48 (NG 1 .. 3), and KS = 2 at NG = 4 (cin 56; cin 64 runs on conv_ws16_kernel), two blocks
// per CU, whose two channel parts of a tile hand each other their partial sums through LDS for the tile's finishing
// wave to add.  (The 8-wave KS = 4 form ran the 128-channel layer until conv_ws16_kernel<4, 1, 8, 2> took it.)  The
// next item's slab (positions plus the dilation halo, all channels, fp32) is fetched into registers before the current
// item's MFMAs and split into the other half of a double-buffered fp16 hi / lo LDS slab after them, so HBM reads
// overlap the matrix work and no weight fragment is re-read.  Dilation <= 4 (conv_spec) bounds the halo at 12.
template <int NG, int Q, int KS, int NW>
__global__ __launch_bounds__(64 * NW, (NW == 4 && KS == 2) ? 2 : 1) void conv_split_ws_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                const float* __restrict__ res,
                                                                const f4* __restrict__ wimg,
                                                                const float* __restrict__ bias, int cin, int cout,
                                                                int N, int dil, int do_res, int sw,
                                                                const uint32_t* __restrict__ amax_in,
                                                                uint32_t* __restrict__ amax_out, int64_t nb, int nslices) {
    extern __shared__ __attribute__((aligned(16))) _Float16 slab16[];
    const int sa = split_sa(amax_in);
    const float sa_scale = __builtin_ldexpf(1.0f, sa), descale = __builtin_ldexpf(1.0f, -(sw + sa));
    float amx = 0.0f;
    constexpr int NT = 64 * NW;
    constexpr int PT = 64 * Q;        // positions per item (2 Q tiles of 32)
    constexpr int C4P = 4 * NG;       // float4 channel groups per staged row (pad channels zero)
    constexpr int CSH = 16 * NG + 8;  // fp16 row stride of the LDS slab
    constexpr int MAXE = ((PT + 24) * C4P + NT - 1) / NT;
    constexpr int NGW = NG / KS;      // channel groups per wave
    constexpr int PS = NW / 2 / KS;   // position parts
    constexpr int TPW = 2 * Q / PS;   // 32-position tiles per wave
    static_assert(NG % KS == 0 && (NW / 2) % KS == 0 && (2 * Q) % PS == 0, "wave decomposition");
    // partial-sum slots per wave: KS = 2 with 2 tiles hands over exactly one (slot 0), else slot = tile
    constexpr int RS = (KS == 2 && TPW == 2) ? 1 : TPW;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int co_sub = wave & 1, rest = wave >> 1;
    const int kp = rest % KS, pp = rest / KS;
    const int g0 = kp * NGW;
    const int halo = 3 * dil;
    const int W = PT + 2 * halo;
    const int plane = W * CSH;
    const int c4n = cin >> 2;
    const int slice = blockIdx.x % nslices;
    const int co_t32 = slice * 2 + co_sub;
    hf8 ah[7][NGW], al[7][NGW];
    {
        const f4* wq = wimg + (int64_t)co_t32 * 7 * NG * 128 + lane;
#pragma unroll
        for (int t = 0; t < 7; ++t)
#pragma unroll
            for (int g = 0; g < NGW; ++g) {
                ah[t][g] = __builtin_bit_cast(hf8, wq[(t * NG + g0 + g) * 128]);
                al[t][g] = __builtin_bit_cast(hf8, wq[(t * NG + g0 + g) * 128 + 64]);
            }
    }
    // KS > 1: partial sums of the channel parts, [wave][tile][register][lane]
    float* const red = reinterpret_cast<float*>(slab16 + (size_t)4 * plane);
    const int chunks = N / PT;
    const int64_t items = nb * chunks;
    const int64_t stride = gridDim.x / nslices;
    int64_t item = blockIdx.x / nslices;
    f4 pre[MAXE];
    auto fetch = [&](int64_t it) {
        const int64_t b = it / chunks;
        const int l0 = (int)(it - b * chunks) * PT;
        const f4* inb = reinterpret_cast<const f4*>(in + b * (int64_t)N * cin);
#pragma unroll
        for (int e = 0; e < MAXE; ++e) {
            const int idx = tid + NT * e;
            const int p = idx / C4P, c4 = idx - p * C4P;
            const int l = l0 - halo + p;
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if (p < W && c4 < c4n && l >= 0 && l < N) v = inb[(int64_t)l * c4n + c4];
            pre[e] = v;
        }
    };
    auto stash = [&](int buf) {
        _Float16* const hiP = slab16 + (size_t)buf * 2 * plane;
#pragma unroll
        for (int e = 0; e < MAXE; ++e) {
            const int idx = tid + NT * e;
            const int p = idx / C4P, c4 = idx - p * C4P;
            if (p < W) {
                hf4 hi, lo;
                split4(pre[e], sa_scale, hi, lo);
                *reinterpret_cast<hf4*>(hiP + p * CSH + 4 * c4) = hi;
                *reinterpret_cast<hf4*>(hiP + plane + p * CSH + 4 * c4) = lo;
            }
        }
    };
    if (item < items) {
        fetch(item);
        stash(0);
    }
    __syncthreads();
    int buf = 0;
    const int tbase = pp * 32 * TPW + col;  // this lane's position column of its first tile within the item
    // KS = 2, two tiles per wave (the 64-channel layers): each wave finishes tile kp; its residual quads are loaded
    // before the MFMAs (one item of HBM latency hidden) instead of in the epilogue (measured +18 % on residual layers)
    constexpr bool PRE_RES = KS == 2 && TPW == 2;
    for (; item < items; item += stride) {
        const int64_t nxt = item + stride;
        if (nxt < items) fetch(nxt);
        f4 resq[4];
        if constexpr (PRE_RES) {
            if (do_res) {
                const int64_t b = item / chunks;
                const int l = (int)(item - b * chunks) * PT + tbase + 32 * kp;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int co = co_t32 * 32 + 8 * r4 + 4 * h;
                    if (co < cout) resq[r4] = *reinterpret_cast<const f4*>(res + (b * N + l) * (int64_t)cout + co);
                }
            }
        }
        const _Float16* const hiP = slab16 + (size_t)buf * 2 * plane;
        const _Float16* const loP = hiP + plane;
        f16v acc[TPW];
#pragma unroll
        for (int q = 0; q < TPW; ++q)
            acc[q] = f16v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 7; ++t)
#pragma unroll
            for (int g = 0; g < NGW; ++g)
#pragma unroll
                for (int q = 0; q < TPW; ++q) {
                    const int off = (tbase + 32 * q + dil * t) * CSH + 16 * (g0 + g) + 8 * h;
                    const hf8 bh = *reinterpret_cast<const hf8*>(hiP + off);
                    const hf8 bl = *reinterpret_cast<const hf8*>(loP + off);
                    acc[q] = mfma16(ah[t][g], bh, acc[q]);
                    acc[q] = mfma16(ah[t][g], bl, acc[q]);
                    acc[q] = mfma16(al[t][g], bh, acc[q]);
                }
        // tile q of the (co_sub, pp) group is finished by channel part q % KS
        if constexpr (KS > 1) {
#pragma unroll
            for (int q = 0; q < TPW; ++q)
                if (q % KS != kp)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((wave * RS + (RS == 1 ? 0 : q)) * 16 + r) * 64 + lane] = acc[q][r];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < TPW; ++q)
                if (q % KS == kp)
#pragma unroll
                    for (int k = 1; k < KS; ++k) {
                        const int other = co_sub + 2 * ((kp + k) % KS + KS * pp);
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            acc[q][r] += red[((other * RS + (RS == 1 ? 0 : q)) * 16 + r) * 64 + lane];
                    }
        }
        const int64_t b = item / chunks;
        const int l0 = (int)(item - b * chunks) * PT;
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            if (q % KS != kp) continue;
            const int l = l0 + tbase + 32 * q;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int co = co_t32 * 32 + 8 * r4 + 4 * h;
                if (co < cout) {
                    const int64_t o = (b * N + l) * (int64_t)cout + co;
                    const f4 bb = *reinterpret_cast<const f4*>(bias + co);
                    f4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu(fmaf(acc[q][4 * r4 + e], descale, bb[e]));
                    if (do_res) {
                        if constexpr (PRE_RES) v += resq[r4];
                        else v += *reinterpret_cast<const f4*>(res + o);
                    }
                    *reinterpret_cast<f4*>(out + o) = v;
                    amx = fmaxf(amx, amax4(v));
                }
            }
        }
        if (nxt < items) stash(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (amax_out != nullptr) publish_amax(amax_out, amx);
}

// LDS bytes of conv_split_ws_kernel: two slab buffers (hi + lo planes) and, for KS > 1, the partial-sum exchange
// (KS = 2, Q = 1: each of the 4 waves hands over one 32 x 32 tile)
static size_t ws_lds_bytes(int ng, int Q, int ks, int dil) {
    const size_t slabs = (size_t)2 * 2 * (64 * Q + 6 * dil) * (16 * ng + 8) * 2;
    return slabs + (ks > 1 ? (size_t)4 * 16 * 64 * 4 : 0);
}

// ------------------------------------------------------------------------------ conv layer, fp16x3, 16-row tiles
// cin = 32 KB (KB = 1, 2, 4): the weight-stationary kernel on v_mfma_f32_16x16x32_f16.  A 16-row tile of output
// channels needs 7 taps x KB K blocks x (hi, lo) A fragments = 56 KB registers per wave (112 at cin 64), so at cin <= 64
// each wave holds ALL input channels of its 16 output channels -- no channel parts, no partial-sum exchange through LDS
// and no second barrier, which is what held conv_split_ws_kernel's 64-channel layers at ~0.4 of the MFMA rate (its
// 32-row tiles need 224 registers for all 64 channels, hence the 2 parts).  8 waves = 4 x 16 output channels (a
// 64-channel slice) x 2 position halves of a 64 Q-position item (TPW = 2 Q 16-position tiles per wave); at cin 128
// (KP = 2) the two halves are channel parts instead, each finishing half of the item's tiles with the other's 16-B
// partial sums from LDS.  16x16x32 operand map (lane l = 16 g + c): A[row c][k 8g + j], B[k 8g + j][col c],
// D[row 4g + i][col c]; k of K block kb = channel 32 kb + k, so a B fragment is 8 channels of one slab row: one
// ds_read_b128 per plane from the double-buffered hi / lo slab, and the accumulator's 4 registers are 4 consecutive
// channels of one position (16-B epilogue stores).  The next item's slab is fetched into registers before the MFMAs
// and split into the other buffer after them, the residual of this item before them; one barrier per item (two with
// channel parts).
__device__ __forceinline__ f4 mfma16x32(const hf8& a, const hf8& b, const f4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// Settled A/B choices: waves per block (8: one block per CU; 4: two), 128-position items where N allows (the plan's
// Q = 2) and the slab row pad -- measured 234 us (8 waves, Q = 2) / 245 us (4 waves, Q = 1) / 253 us (8 waves, Q = 2,
// CIN + 8 rows) per 64-channel layer per 4096 codewords.  The 128-channel layer runs here as <4, 1, 8, 2>, not on
// conv_split_ws_kernel's former 8-wave, 4-part form.
constexpr int kWs16Waves = 8;
constexpr int kWs16Pad = 16;
template <int KB, int Q, int NW, int KP>
__global__ __launch_bounds__(64 * NW, 8 / NW) void conv_ws16_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           const float* __restrict__ res, const f4* __restrict__ wimg,
                                                           const float* __restrict__ bias, int cout, int N, int dil,
                                                           int do_res, int sw, const uint32_t* __restrict__ amax_in,
                                                           uint32_t* __restrict__ amax_out, int64_t nb, int nslices) {
    extern __shared__ __attribute__((aligned(16))) _Float16 slab16[];
    constexpr int NT = 64 * NW;
    constexpr int CIN = 32 * KB;
    constexpr int PT = 64 * Q;        // positions per item
    constexpr int C4P = CIN / 4;      // float4 channel groups per staged row
    // fp16 row stride of the LDS slab: CIN + 16 halfs.  A B fragment read (lane 16 g + c: row c, channels 8 g ..) puts
    // rows c at c * CSH / 8 16-B units and g at +g units; with CIN + 8 (36 / 20 dwords) ds_read_b128's lane groups
    // {0-3, 12-15, 20-27}, ... collided 2-way (PMC: SQ_LDS_BANK_CONFLICT 0.48 of SQ_LDS_IDX_ACTIVE), with CIN + 16
    // (40 / 24 dwords) every group hits 16 distinct units
    constexpr int CSH = CIN + kWs16Pad;
    constexpr int MAXE = ((PT + 24) * C4P + NT - 1) / NT;
    constexpr int PP = NW / 4 / KP;   // position parts
    constexpr int TPW = 4 * Q / PP;   // 16-position tiles per wave
    constexpr int KBW = KB / KP;      // K blocks (32 input channels) per wave
    static_assert((NW == 4 || NW == 8) && PP >= 1 && KB % KP == 0 && TPW % KP == 0, "wave decomposition");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, col = lane & 15;
    const int co16 = wave & 3, kp = (wave >> 2) % KP, pp = (wave >> 2) / KP;
    const int halo = 3 * dil;
    const int W = PT + 2 * halo;
    const int plane = W * CSH;
    const int slice = blockIdx.x % nslices;
    const int t16 = slice * 4 + co16;  // 16-channel output tile
    const int sa = split_sa(amax_in);
    const float sa_scale = __builtin_ldexpf(1.0f, sa), descale = __builtin_ldexpf(1.0f, -(sw + sa));
    hf8 ah[7][KBW], al[7][KBW];
    {
        const f4* wq = wimg + (int64_t)t16 * 7 * KB * 128 + lane;
#pragma unroll
        for (int t = 0; t < 7; ++t)
#pragma unroll
            for (int kb = 0; kb < KBW; ++kb) {
                ah[t][kb] = __builtin_bit_cast(hf8, wq[(t * KB + kp * KBW + kb) * 128]);
                al[t][kb] = __builtin_bit_cast(hf8, wq[(t * KB + kp * KBW + kb) * 128 + 64]);
            }
    }
    // KP = 2: the two channel parts of a 16-channel tile each finish half of its TPW position tiles, taking the other
    // part's partial sums (one 16-B accumulator per lane and tile) from LDS behind the slab
    f4* const red = reinterpret_cast<f4*>(slab16 + (size_t)4 * (PT + 24) * CSH);
    auto fin = [&](int q) { return q * KP / TPW == kp; };
    const int chunks = N / PT;
    const int items = (int)nb * chunks;
    const int stride = gridDim.x / nslices;
    int item = blockIdx.x / nslices;
    f4 pre[MAXE];
    auto fetch = [&](int it) {
        const int b = it / chunks;
        const int l0 = (it - b * chunks) * PT;
        const f4* inb = reinterpret_cast<const f4*>(in + (int64_t)b * N * CIN);
#pragma unroll
        for (int e = 0; e < MAXE; ++e) {
            const int idx = tid + NT * e;
            const int p = idx / C4P, c4 = idx - p * C4P;
            const int l = l0 - halo + p;
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if (p < W && l >= 0 && l < N) v = inb[(int64_t)l * C4P + c4];
            pre[e] = v;
        }
    };
    auto stash = [&](int buf) {
        _Float16* const hiP = slab16 + (size_t)buf * 2 * plane;
#pragma unroll
        for (int e = 0; e < MAXE; ++e) {
            const int idx = tid + NT * e;
            const int p = idx / C4P, c4 = idx - p * C4P;
            if (p < W) {
                hf4 hi, lo;
                split4(pre[e], sa_scale, hi, lo);
                *reinterpret_cast<hf4*>(hiP + p * CSH + 4 * c4) = hi;
                *reinterpret_cast<hf4*>(hiP + plane + p * CSH + 4 * c4) = lo;
            }
        }
    };
    if (item < items) {
        fetch(item);
        stash(0);
    }
    __syncthreads();
    int buf = 0;
    const int tbase = pp * 16 * TPW + col;  // this lane's position column of its first tile within the item
    const int co = t16 * 16 + 4 * g;        // the lane's 4 output channels
    const bool co_ok = co < cout;
    const f4 bb = co_ok ? *reinterpret_cast<const f4*>(bias + co) : f4{0.f, 0.f, 0.f, 0.f};
    float amx = 0.0f;
    for (; item < items; item += stride) {
        const int nxt = item + stride;
        if (nxt < items) fetch(nxt);
        const int b = item / chunks;
        const int64_t row0 = (int64_t)b * N + (item - b * chunks) * PT + tbase;  // output row of tile 0
        f4 resv[TPW];
        if (do_res && co_ok) {
#pragma unroll
            for (int q = 0; q < TPW; ++q)
                if (fin(q)) resv[q] = *reinterpret_cast<const f4*>(res + (row0 + 16 * q) * cout + co);
        }
        const _Float16* const hiP = slab16 + (size_t)buf * 2 * plane;
        const _Float16* const loP = hiP + plane;
        f4 acc[TPW];
#pragma unroll
        for (int q = 0; q < TPW; ++q) acc[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 7; ++t)
#pragma unroll
            for (int kb = 0; kb < KBW; ++kb)
#pragma unroll
                for (int q = 0; q < TPW; ++q) {
                    const int off = (tbase + 16 * q + dil * t) * CSH + 32 * (kp * KBW + kb) + 8 * g;
                    const hf8 bh = *reinterpret_cast<const hf8*>(hiP + off);
                    const hf8 bl = *reinterpret_cast<const hf8*>(loP + off);
                    acc[q] = mfma16x32(ah[t][kb], bh, acc[q]);
                    acc[q] = mfma16x32(ah[t][kb], bl, acc[q]);
                    acc[q] = mfma16x32(al[t][kb], bh, acc[q]);
                }
        if constexpr (KP > 1) {
            const int slot = (co16 * PP + pp) * KP;
#pragma unroll
            for (int q = 0; q < TPW; ++q)
                if (!fin(q)) red[((slot + kp) * TPW + q) * 64 + lane] = acc[q];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < TPW; ++q)
                if (fin(q))
#pragma unroll
                    for (int o = 1; o < KP; ++o) acc[q] += red[((slot + (kp + o) % KP) * TPW + q) * 64 + lane];
        }
        if (co_ok) {
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                if (!fin(q)) continue;
                f4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = gelu(fmaf(acc[q][e], descale, bb[e]));
                if (do_res) v += resv[q];
                *reinterpret_cast<f4*>(out + (row0 + 16 * q) * cout + co) = v;
                amx = fmaxf(amx, amax4(v));
            }
        }
        if (nxt < items) stash(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (amax_out != nullptr) publish_amax(amax_out, amx);
}

// slab: 2 buffers x (hi, lo) x (64 Q + 6 dil) rows; KP = 2: + the partial sums, 8 waves x TPW tiles x 64 lanes x 16 B
// (the kernel places them after the dil = 4 slab)
static size_t ws16_lds_bytes(int kb, int Q, int dil, int kp) {
    const size_t slab = (size_t)2 * 2 * (64 * Q + 6 * (kp > 1 ? 4 : dil)) * (32 * kb + kWs16Pad) * 2;
    return slab + (kp > 1 ? (size_t)8 * (2 * Q * kp) * 64 * 16 : 0);
}

// ------------------------------------------------------------------------------ host
// blocks of a persistent kernel: per_cu per CU, a multiple of the 64-channel slice count (a block keeps one slice's
// weights), no more than there are (slice, item) pairs
static unsigned persistent_blocks(const LayerPlan& L, const LayerArgs& a, int per_cu) {
    const int nslices = (L.cout + 63) / 64;
    const int64_t items = a.nb * (a.N / (64 * L.q)) * nslices;
    int64_t nblk = (int64_t)device_cu_count() * per_cu;
    nblk -= nblk % nslices;
    if (nblk > items) nblk = items;
    return (unsigned)(nblk < nslices ? nslices : nblk);
}

// KS = 1: one persistent 4-wave block per CU.  KS = 2: two independent blocks per CU (67 KB of LDS each), so one
// block's barrier and latency waits are filled by the other's work
template <int NG, int Q, int KS>
static int launch_ws(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    return launch_lds<conv_split_ws_kernel<NG, Q, KS, 4>>(
        "conv_split_ws_kernel launch", persistent_blocks(L, a, KS), 256, ws_lds_bytes(NG, Q, KS, L.dil), s, a.in,
        a.out, a.res, reinterpret_cast<const f4*>(a.img + L.woff), a.img + L.boff, L.cin, L.cout, a.N, L.dil, L.res, L.sw,
        a.am_in, a.am_out, a.nb, (L.cout + 63) / 64);
}

int launch_conv_ws(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    switch (100 * L.kdim + 10 * L.q + L.parts) {  // NG, Q, KS
        case 111: return launch_ws<1, 1, 1>(L, a, s);
        case 121: return launch_ws<1, 2, 1>(L, a, s);
        case 211: return launch_ws<2, 1, 1>(L, a, s);
        case 221: return launch_ws<2, 2, 1>(L, a, s);
        case 311: return launch_ws<3, 1, 1>(L, a, s);
        case 321: return launch_ws<3, 2, 1>(L, a, s);
        case 412: return launch_ws<4, 1, 2>(L, a, s);
    }
    return fail(NPD_ENOTSUP, "npd_conv: no conv_split_ws_kernel for this plan");
}

// one persistent 8-wave block per CU
template <int KB, int Q, int KP>
static int launch_ws16(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    return launch_lds<conv_ws16_kernel<KB, Q, kWs16Waves, KP>>(
        "conv_ws16_kernel launch", persistent_blocks(L, a, 8 / kWs16Waves), 64 * kWs16Waves,
        ws16_lds_bytes(KB, Q, L.dil, KP), s, a.in, a.out, a.res, reinterpret_cast<const f4*>(a.img + L.woff),
        a.img + L.boff, L.cout, a.N, L.dil, L.res, L.sw, a.am_in, a.am_out, a.nb, (L.cout + 63) / 64);
}

int launch_conv_ws16(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    switch (100 * L.kdim + 10 * L.q + L.parts) {  // KB, Q, KP
        case 111: return launch_ws16<1, 1, 1>(L, a, s);
        case 121: return launch_ws16<1, 2, 1>(L, a, s);
        case 211: return launch_ws16<2, 1, 1>(L, a, s);
        case 221: return launch_ws16<2, 2, 1>(L, a, s);
        case 412: return launch_ws16<4, 1, 2>(L, a, s);
    }
    return fail(NPD_ENOTSUP, "npd_conv: no conv_ws16_kernel for this plan");
}

}  // namespace conv
}  // namespace npd

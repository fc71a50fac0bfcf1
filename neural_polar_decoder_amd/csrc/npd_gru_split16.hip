// npd_gru_split16.hip -- gru16p_kernel, the headline kernel: the split 16-bit MFMA paths on 16-codeword waves.
// =============================================================================== split paths, 16-codeword waves
// F = 64, 2 layers (the metric's CRISP GRU), split precisions, N a multiple of 32.  The 32-codeword split kernels
// above need ~500 registers (P, both states, the gate accumulators): one wave per SIMD, and a step is one serial
// chain (layer-0 GEMM -> update -> split -> layer-1 GEMM -> update -> output -> decision) that leaves the MFMA pipe
// idle while the wave does its VALU work.  Here a wave owns 16 codewords on v_mfma_f32_16x16x32_{f16,bf16} (the same
// FLOP per cycle as 32x32x16), so every register array halves and TWO waves share each SIMD, hiding each other's
// LDS and dependency latencies.  (They do not hide each other's VALU work behind MFMAs: measured, an fp16 MFMA wave
// and an FMA wave on one SIMD take the sum of their times, profiles/round3/coissue.txt; PMC: MFMA busy + VALU
// active ~ all SIMD cycles.  Hence the VALU trims below: no fp32 k-step MFMAs, folded gate constants, permlane
// reductions, immediate-offset LDS reads.)
// 16x16x32 maps: lane l = 16 g + c holds D[row 4g + i][codeword c] (i = 0..3), A[row c][k 8g + j], B[k 8g + j][col c].
// Hidden units form 16-row tiles ht = 0..3; K block kb (32 units) is tiles 2kb, 2kb + 1, with MFMA k index 8g + j
// <-> hidden unit 16 (2kb + (j >> 2)) + 4g + (j & 3): an updated state tile converts register for register into the
// next GEMM's B fragment (no lane movement); the host permutes the weight images to match.
// Constants: layer 0's biases and one-hot column 0 enter P once per codeword, the x_i column is one FMA per
// accumulator element, layer 1's biases initialise its accumulators from LDS: no fp32 k-step MFMAs.
// The arithmetic per element (split products, fp32 accumulation, gate nonlinearities) is the 32-codeword kernels'.
#include "npd_gru_split.hpp"

namespace npd {
namespace gru {

struct Geo16 {
    static constexpr int RT = 12, KB = 2, NG = 3;    // 16-row gate tiles, 32-unit K blocks, weight matrices
    static constexpr int IMG4 = NG * RT * KB * 64;   // 16-B fragments per split image
    // fragment (matrix g, row tile t, K block kb, part p = hi / lo) of lane l at f4 index (((g RT + t) KB + kb) 2 + p) 64 + l:
    // a matrix spans 48 KB, so every read of a GEMM is an immediate offset (< 64 KB) from one per-lane base
    static constexpr int G_BYTES = RT * KB * 2 * 1024;
    static constexpr int OFF_C = 2 * IMG4 * 4;       // floats: constants after the weight fragments
    static constexpr int C0L0 = OFF_C, C1L0 = OFF_C + 192, BHN0 = OFF_C + 384, C0L1 = OFF_C + 448,
                         BHN1 = OFF_C + 640, WLIN = OFF_C + 704, TOTAL = OFF_C + 768;
    // behind the image in LDS, written by every block from the kernel arguments: one word per step in DECODE order
    // (rev applied), bits 0-7 the position's message slot, bit 8 its is-information bit, bit 9 set where the decision
    // is compared with the message (a bit of its own: all 256 slot values are slots, K = 256)
    static constexpr int LDS_BYTES = TOTAL * 4 + kMaxN * 4;
};

__device__ __forceinline__ f4 mfma16s(const hf8& a, const hf8& b, const f4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f4 mfma16s(const bf8& a, const bf8& b, const f4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// B fragments of a state: fragment kb, element j = tile 2kb + (j >> 2), register j & 3 (hi and, split, lo)
template <int SPLIT>
__device__ __forceinline__ void split16s(const f4 (&h)[4], typename SplitT<SPLIT>::V (&hi)[2],
                                         typename SplitT<SPLIT>::V (&lo)[2]) {
    using S = SplitT<SPLIT>;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = h[2 * kb + (j >> 2)][j & 3] * S::kIn;
            const typename S::E b = (typename S::E)v;
            hi[kb][j] = b;
            if (S::kLo) lo[kb][j] = (typename S::E)(v - (float)b);
        }
}

// LDS fragment of the 16-codeword image: wb = this lane's byte base of the matrix (laundered once per kernel)
__device__ __forceinline__ f4 frag16(const f4* __restrict__ smem4, uint32_t wb, int t, int kb, int part) {
    return *reinterpret_cast<const f4*>(reinterpret_cast<const char*>(smem4) + wb +
                                        ((t * Geo16::KB + kb) * 2 + part) * 1024);
}
#ifdef NPD_GRU16_READ2
__device__ __forceinline__ f4 frag16v(const f4* __restrict__ smem4, uint32_t wb, int t, int kb, int part) {
    // volatile and in the LDS address space: a ds_read_b128 that is neither merged with the first read nor dropped
    typedef __attribute__((address_space(3))) const char LdsC;
    typedef __attribute__((address_space(3))) const volatile f4 LdsVF4;
    return *(LdsVF4*)((LdsC*)smem4 + wb + ((t * Geo16::KB + kb) * 2 + part) * 1024);
}
#endif

// (p_row0 + p_row1) + (p_row2 + p_row3) over the four 16-lane rows, the same in every lane (the order of
// __shfl_xor 16 then 32) on v_permlane16_swap / v_permlane32_swap: VALU, no LDS round trip
__device__ __forceinline__ float sum_rows16(float p) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(p), false, false);
    const float s = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
}

__device__ __forceinline__ f4 fma4(float x, const f4& c, const f4& p) {
    return f4{fmaf(x, c[0], p[0]), fmaf(x, c[1], p[1]), fmaf(x, c[2], p[2]), fmaf(x, c[3], p[3])};
}

// The two-tile body needs more than 256 registers, so some values live in accumulation registers, which the VALU
// cannot read: a copy per use.  The y projection P is read once per step and element, the cheapest to keep there;
// pinned there where it is read, it leaves the arch registers to the values that are read more often.  Row tiles of
// the mask (bit t: row tile t of both codeword tiles): eight with a lo part, the n-gate's four without -- the fewest
// copies in the step loop with the weight fragments already in accumulation registers (gemm16i), by `make asm` and
// tools/isa_loopmix.py --inner: 66 and 33 per step of two tiles against 173 and 121 where the compiler chooses alone
// (profiles/round8/gru16_pair_ab.txt).
#ifndef NPD_GRU16_P_AGPR
#define NPD_GRU16_P_AGPR (SplitT<SPLIT>::kLo ? 0x0ff : 0xf00)
#endif
template <int SPLIT, int NTL, int T>
__device__ __forceinline__ const f4& proj(f4 (&P)[Geo16::RT]) {
    if constexpr (NTL > 1 && (((NPD_GRU16_P_AGPR) >> T) & 1)) asm volatile("" : "+a"(P[T]));
    return P[T];
}

#define NPD_GRU16_WPB 8
// codeword tiles per wave of the count-only instantiation (the general one: 1); 1 builds the two-waves-per-SIMD form
// for A/B runs (tools/build_variants.sh)
#ifndef NPD_GRU16_CNT_TILES
#define NPD_GRU16_CNT_TILES 2
#endif
#define NPD_TILES _Pragma("unroll") for (int tl = 0; tl < NTL; ++tl)
// ---- the step is software-pipelined (measured 14.86 -> 14.42 ms per 2^20 words against the plain tile-by-tile
// order, profiles/round3/gru_split_ab.txt; the plain order was removed in round 4).  A wave's own VALU instructions issue in the gaps of its 16-bit
// MFMAs (8 of the 16 cycles of a 16x16x32 are busy for vector issue, MI355X_MICROARCH.md), while another wave's
// do not (profiles/round3/coissue.txt: an fp16 MFMA wave and an FMA wave on one SIMD take the sum of their times).
// So each hidden tile's GEMM carries the update of the PREVIOUS tile (cut into 12 chunks of ~5 instructions:
// element i, stage 0 exp2s / 1 rcps + n-gate input + exp2 / 2 rcp + blend), spread over its MFMA triples between
// sched_barrier fences; the h1 update of tile 3, the output, the decision and the h1 split ride on the NEXT step's
// layer-0 tile-0 GEMM (which needs only h0', not x_i: the x_i column and P are added after it).
// What follows that GEMM's last MFMA has no MFMA of this wave to ride on, so the count-only body (CNT) keeps it
// short (instruction counts per path: profiles/round7/gru16_strip_ab.txt):
//  - no scalar memory load in the step loop: the position's message slot and is-information bit come from a table
//    in LDS (Geo16::LDS_BYTES), read with one wave-uniform ds_read a GEMM ahead.  SMEM returns out of order, so a
//    wait for it was an lgkmcnt(0) that also drained the `cur` fragment look-ahead;
//  - the x_i columns the top of the step needs are read beside the tail GEMM, not at the top;
//  - CNT computes the output, its row reduction and the sign only at information positions: a frozen position's
//    decision is the constant 1.0.
// The h1 split stays after the decision: splitting each finished h1 tile beside a later layer-1 GEMM (results pinned
// with empty asm, or the compiler sinks them back) measured 0.25 % slower than leaving it there (same file).
template <int SPLIT>
struct Upd4 {
    f4 er, ez, en, z;
    template <int C>
    __device__ __forceinline__ void step(f4& h, const f4& ar, const f4& az, const f4& ain, const f4& ahn) {
        constexpr float c1 = SplitT<SPLIT>::kC1, c2 = SplitT<SPLIT>::kC2;
        constexpr int i = C / 3, st = C % 3;
        if constexpr (st == 0) {
            er[i] = __builtin_amdgcn_exp2f(c1 * ar[i]);
            ez[i] = __builtin_amdgcn_exp2f(c1 * az[i]);
        } else if constexpr (st == 1) {
            const float r = __builtin_amdgcn_rcpf(1.0f + er[i]);
            z[i] = __builtin_amdgcn_rcpf(1.0f + ez[i]);
            en[i] = __builtin_amdgcn_exp2f(c2 * (ain[i] + ahn[i] * r));
        } else {
            const float nn = fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + en[i]), -1.0f);
            h[i] = (h[i] - nn) * z[i] + nn;
        }
    }
};

template <int SPLIT>
__device__ __forceinline__ void split_kb(const f4 (&h)[4], int kb, typename SplitT<SPLIT>::V (&hi)[2],
                                         typename SplitT<SPLIT>::V (&lo)[2]) {
    using S = SplitT<SPLIT>;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = h[2 * kb + (j >> 2)][j & 3] * S::kIn;
        const typename S::E b = (typename S::E)v;
        hi[kb][j] = b;
        if (S::kLo) lo[kb][j] = (typename S::E)(v - (float)b);
    }
}

// A fragments (hi, lo) of one K block of a GEMM's NU row tiles
template <int SPLIT, int NU>
struct Frag16 {
    typename SplitT<SPLIT>::V h[NU], l[NU];
};
template <int SPLIT, int NU>
__device__ __forceinline__ void load_kb16(const f4* __restrict__ smem4, uint32_t wb, const int (&t)[NU], int kb,
                                          Frag16<SPLIT, NU>& f) {
    using V = typename SplitT<SPLIT>::V;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        f.h[u] = __builtin_bit_cast(V, frag16(smem4, wb, t[u], kb, 0));
        if (SplitT<SPLIT>::kLo) f.l[u] = __builtin_bit_cast(V, frag16(smem4, wb, t[u], kb, 1));
    }
#ifdef NPD_GRU16_READ2
    // measurement build (profiles/round8/gru16_pair_ab.txt): every fragment is read from LDS a second time and the
    // value dropped (a volatile read, so it is issued; holding the copies in pinned registers spills at 256)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        (void)frag16v(smem4, wb, t[u], kb, 0);
        if (SplitT<SPLIT>::kLo) (void)frag16v(smem4, wb, t[u], kb, 1);
    }
#endif
}

// acc[u] += W_g[row tile t[u]] . state (both K blocks); work(IC<c>) for chunks C0 .. C0 + NCH - 1 spread evenly
// over the 2 NU MFMA triples, one sched_barrier-fenced region per triple.  The K block 0 fragments arrive in `cur`,
// loaded by the previous GEMM, and this GEMM loads the next one's (matrix base wbn, tiles tn) into it once its own
// K block 0 triples have issued, so no GEMM starts on an LDS round trip (measured 13.08-13.13 against 13.21-13.25 ms
// per 2^20 words with each GEMM loading its own fragments, profiles/round5/gru16_ab.txt).
// A wave owns NTL codeword tiles (their accumulators, states and B fragments are arrays over the tile): every A
// fragment read from LDS feeds the MFMAs of all of them, in the same order on each accumulator as with one tile, and
// work(IC<c>) does chunk c for every tile.
template <int SPLIT, int NTL, int NU, int C0, int NCH, typename Work>
__device__ __forceinline__ void gemm16i(const f4* __restrict__ smem4, uint32_t wb, const int (&t)[NU],
                                        f4 (&acc)[NTL][NU], const typename SplitT<SPLIT>::V (&bh)[NTL][2],
                                        const typename SplitT<SPLIT>::V (&bl)[NTL][2], Frag16<SPLIT, NU>& cur,
                                        uint32_t wbn, const int (&tn)[NU], Work&& work) {
    constexpr int NT = 2 * NU;
    Frag16<SPLIT, NU> f[2];  // f[1]: this GEMM's K block 1 (K block 0 is `cur`)
    load_kb16<SPLIT, NU>(smem4, wb, t, 1, f[1]);
    asm volatile("" ::: "memory");  // keeps the (loop-invariant) LDS fragment reads in the step loop
    static_for<0, NT>([&](auto trc) {
        constexpr int tr = decltype(trc)::value;
        constexpr int kb = tr / NU, u = tr % NU;
        Frag16<SPLIT, NU>& F = kb == 0 ? cur : f[kb];
        // two tiles: the fragment is pinned into accumulation registers where the MFMAs (which read them at no cost)
        // would wait for it anyway, so that ds_read_b128 writes it there and it takes no arch registers
        if constexpr (NTL > 1) {
            asm volatile("" : "+a"(F.h[u]));
            if (SplitT<SPLIT>::kLo) asm volatile("" : "+a"(F.l[u]));
        }
        // tile by tile, each tile's products back to back on its accumulator (one product at a time across the
        // tiles measured 0.8 % slower, profiles/round8/gru16_pair_ab.txt)
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) {
            acc[tl][u] = mfma16s(F.h[u], bh[tl][kb], acc[tl][u]);
            if (SplitT<SPLIT>::kLo) {
                acc[tl][u] = mfma16s(F.h[u], bl[tl][kb], acc[tl][u]);
                acc[tl][u] = mfma16s(F.l[u], bh[tl][kb], acc[tl][u]);
            }
        }
        if constexpr (tr == NU - 1) {
            asm volatile("" ::: "memory");
            load_kb16<SPLIT, NU>(smem4, wbn, tn, 0, cur);
        }
        static_for<C0 + NCH * tr / NT, C0 + NCH * (tr + 1) / NT>([&](auto cc) { work(cc); });
        __builtin_amdgcn_sched_barrier(0);
    });
}

// CNT: the count-only body (counters != NULL; decoded, logits, gt and h0 all NULL): no decision store, no genie load,
// and at a frozen position the decision is the constant 1.0 without the output having been computed.
// NTL: codeword tiles per wave.  1: eight waves per workgroup, two per SIMD, which hide each other's latencies (the
// general body).  2: four waves, one per SIMD with the whole register file; the wave's two tiles are tiles 2p, 2p + 1
// of one segment and step together, each weight fragment and each constant read from LDS once for both
// (profiles/round8/gru16_pair_ab.txt).
template <int SPLIT, bool CNT, int NTL>
__global__ __launch_bounds__(64 * NPD_GRU16_WPB / NTL) void gru16p_kernel(const ArgsB a) {
    constexpr int WPB = NPD_GRU16_WPB / NTL;
    using G = Geo16;
    using S = SplitT<SPLIT>;
    using V = typename S::V;
    using E = typename S::E;
    extern __shared__ __attribute__((aligned(16))) f4 smem4[];
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(smem4) + G::TOTAL;
    {
        const f4* src = reinterpret_cast<const f4*>(a.img);
        for (int i = threadIdx.x; i < G::TOTAL / 4; i += blockDim.x) smem4[i] = src[i];
        uint32_t* tw = reinterpret_cast<uint32_t*>(smem4) + G::TOTAL;
        for (int i = threadIdx.x; i < a.N; i += blockDim.x) {
            const int jj = a.rev ? a.N - 1 - i : i;
            const uint32_t sl = (a.slotw[jj >> 2] >> (8 * (jj & 3))) & 255u;
            const uint32_t cmp = a.counters ? (a.cmp[jj >> 5] >> (jj & 31)) & 1u : 0u;
            tw[i] = sl | (((a.info[jj >> 5] >> (jj & 31)) & 1u) << 8) | (cmp << 9);
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g4 = lane >> 4;
    const int col = lane & 15;
    const int N = a.N;
    const int nkb = N / 32;
    const int64_t tps = (a.B + 15) / 16;  // tiles per segment
    const int64_t ups = (tps + NTL - 1) / NTL;  // wave units per segment: NTL consecutive tiles (the last may lack some)
    const int64_t nunits = ups * (a.nseg > 1 ? a.nseg : 1);
    const bool count = a.counters != nullptr;
    uint32_t be_w = 0, bl_w = 0;  // this wave's bit / block errors of the current segment (wave-uniform)
    // per-lane LDS byte bases, laundered so that every fragment / constant read is base + immediate offset
    uint32_t wbs[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        uint32_t v = g * G::G_BYTES + lane * 16;
        asm volatile("" : "+v"(v));
        wbs[g] = v;
    }
    uint32_t cb = (G::OFF_C + 4 * g4) * 4;
    asm volatile("" : "+v"(cb));
    auto c4 = [&](int off, int t) -> f4 {
        return *reinterpret_cast<const f4*>(reinterpret_cast<const char*>(smem4) + cb + (off - G::OFF_C + 16 * t) * 4);
    };
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    constexpr int T0[3] = {0, 4, 8};
    auto nowork = [](auto) {};

    for (int64_t unit = (int64_t)blockIdx.x * WPB + wave; unit < nunits; unit += (int64_t)gridDim.x * WPB) {
        const int64_t seg = unit / ups;
        int64_t cw[NTL], cwc[NTL], rowoff[NTL];
        bool valid[NTL];
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) {
            cw[tl] = ((unit - seg * ups) * NTL + tl) * 16 + col;  // codeword within the segment
            valid[tl] = cw[tl] < a.B;                             // a tile past the segment's last: no lane valid
            cwc[tl] = valid[tl] ? cw[tl] : a.B - 1;
            rowoff[tl] = (seg * a.B + cw[tl]) * N;                // this codeword's row of y / decoded / logits
        }
        // count mode: the codeword's messages as 2-bit codes of rint(msg) (-1: 0, +1: 1, 0: 2, else 3; the decision
        // d is in {-1, 0, +1}), slot sl held by row sl & 3 at bits 2 (q & 15) of word q >> 4, q = sl >> 2: 4 registers
        // cover K <= 256, loaded once per tile, so no step waits on a message load.  Eight slots of a row form a group
        // behind one wave-uniform bound; inside it the index is clamped instead of guarded, so the group's eight
        // loads are in flight together (K = 32: one round trip per tile)
        uint32_t mc[NTL][4];
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) {
#pragma unroll
            for (int w = 0; w < 4; ++w) mc[tl][w] = 0u;
            if (!count) continue;
            const float* mr = a.msg + cwc[tl] * a.K;
            int g4t = g4;  // laundered per tile: the clamped indices are not to be hoisted out of the tile loop
            asm volatile("" : "+v"(g4t));
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int j0 = 0; j0 < 16; j0 += 8)
                    if (4 * (16 * w + j0) < a.K) {
                        float mv[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int sl = 4 * (16 * w + j0 + j) + g4t;
                            mv[j] = mr[sl < a.K ? sl : a.K - 1];
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int sl = 4 * (16 * w + j0 + j) + g4t;
                            const float v = rintf(mv[j]);
                            const uint32_t code = v == -1.0f ? 0u : v == 1.0f ? 1u : v == 0.0f ? 2u : 3u;
                            mc[tl][w] |= (sl < a.K ? code : 0u) << (2 * (j0 + j));
                        }
                    }
        }
        uint32_t nerr[NTL];  // this row's share of the codeword's bit errors
        f4 P[NTL][G::RT];
#pragma unroll
        for (int t = 0; t < G::RT; ++t) {
            const f4 c = c4(G::C0L0, t);
#pragma unroll
            for (int tl = 0; tl < NTL; ++tl) P[tl][t] = c;
        }
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) nerr[tl] = 0u;
        if (a.y) {
            for (int kb = 0; kb < nkb; ++kb) {
                V yh[NTL], yl[NTL];
#pragma unroll
                for (int tl = 0; tl < NTL; ++tl) {
                    const float* yr = a.y + (seg * a.B + cwc[tl]) * N;
                    const f4 y0 = *reinterpret_cast<const f4*>(yr + 32 * kb + 8 * g4);
                    const f4 y1 = *reinterpret_cast<const f4*>(yr + 32 * kb + 8 * g4 + 4);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float v = (j < 4 ? y0[j] : y1[j - 4]) * S::kIn;
                        yh[tl][j] = (E)v;
                        if (S::kLo) yl[tl][j] = (E)(v - (float)yh[tl][j]);
                    }
                }
                // the K block's weight fragments, all requested before the first MFMA (states, B fragments and the
                // step's accumulators are not live yet): one L2 round trip per K block, not one per row tile
                V wh[G::RT], wl[G::RT];
#pragma unroll
                for (int t = 0; t < G::RT; ++t) {
                    wh[t] = __builtin_bit_cast(V, a.wy[(t * nkb + kb) * 64 + lane]);
                    if (S::kLo) wl[t] = __builtin_bit_cast(V, a.wy[a.wy_lo + (t * nkb + kb) * 64 + lane]);
                }
                asm volatile("" ::: "memory");
#pragma unroll
                for (int t = 0; t < G::RT; ++t)
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        P[tl][t] = mfma16s(wh[t], yh[tl], P[tl][t]);
                        if (S::kLo) {
                            P[tl][t] = mfma16s(wh[t], yl[tl], P[tl][t]);
                            P[tl][t] = mfma16s(wl[t], yh[tl], P[tl][t]);
                        }
                    }
            }
        }
        f4 h0[NTL][4], h1[NTL][4];
        V fh[NTL][2], fl[NTL][2], gh[NTL][2], gl[NTL][2];
        float xb[NTL];
        f4 a0[NTL][3];
        {
            const f4 bhn = c4(G::BHN0, 0);
#pragma unroll
            for (int tl = 0; tl < NTL; ++tl) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    h0[tl][t] = zero;
                    h1[tl][t] = zero;
                }
                if (!CNT && a.h0) {  // register e of tile t = hidden unit 16 t + 4 g4 + e of codeword col (F = 64, 2 layers)
                    const float* hr = a.h0 + (seg * a.B + cwc[tl]) * 128;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int f = 16 * t + 4 * g4 + e;
                            h0[tl][t][e] = hr[2 * f];
                            h1[tl][t][e] = hr[2 * f + 1];
                        }
                }
                split16s<SPLIT>(h0[tl], fh[tl], fl[tl]);
                split16s<SPLIT>(h1[tl], gh[tl], gl[tl]);
                xb[tl] = 1.0f;
                // layer 0, hidden tile 0 of step 0: W_hh0 h0 part (the x_i column and P are added at the top of the step)
                a0[tl][0] = zero;
                a0[tl][1] = zero;
                a0[tl][2] = bhn;
            }
        }
        constexpr int T1[3] = {1, 5, 9};
        Frag16<SPLIT, 3> cur;
        load_kb16<SPLIT, 3>(smem4, wbs[0], T0, 0, cur);
        gemm16i<SPLIT, NTL, 3, 0, 0>(smem4, wbs[0], T0, a0, fh, fl, cur, wbs[0], T1, nowork);
        // the x_i columns of hidden tile 0 and of tile 1's r and z rows (the step's first GEMM), read a GEMM ahead
        // (here, then beside the tail GEMM): the top of the step, which has no MFMA of this wave to hide behind, does
        // not start on an LDS round trip.  Tile 1's: count-only (the general body has no registers to hold them
        // across the tail: it spills with them)
        constexpr int NX = CNT ? 5 : 3;
        f4 xc[5] = {c4(G::C1L0, 0), c4(G::C1L0, 4), c4(G::C1L0, 8), c4(G::C1L0, 1), c4(G::C1L0, 5)};
        // PRE (one wave per SIMD: no partner wave runs while this one waits): every GEMM's accumulator constants are
        // read from LDS a GEMM ahead into kq, so that no GEMM's first MFMA waits for an LDS round trip
        constexpr bool PRE = NTL > 1;
        f4 kq[3];
        auto ahead = [&](int o0, int t0, int o1, int t1, int o2, int t2) {
            kq[0] = c4(o0, t0);
            kq[1] = c4(o1, t1);
            kq[2] = c4(o2, t2);
        };
        if constexpr (PRE) kq[2] = c4(G::BHN0, 1);
        for (int ii = 0; ii < N; ++ii) {
            Upd4<SPLIT> u[NTL];
            // ================= layer 0
            f4 ap[NTL][3], ainp[NTL];
            NPD_TILES {
                ap[tl][0] = a0[tl][0] + fma4(xb[tl], xc[0], proj<SPLIT, NTL, 0>(P[tl]));
                ap[tl][1] = a0[tl][1] + fma4(xb[tl], xc[1], proj<SPLIT, NTL, 4>(P[tl]));
                ap[tl][2] = a0[tl][2];
                ainp[tl] = fma4(xb[tl], xc[2], proj<SPLIT, NTL, 8>(P[tl]));
            }
            static_for<1, 4>([&](auto htc) {
                constexpr int ht = decltype(htc)::value;
                const int T[3] = {ht, 4 + ht, 8 + ht};
                f4 acc[NTL][3];
                {
                    const f4 cr = (ht == 1 && NX == 5) ? xc[3] : PRE ? kq[0] : c4(G::C1L0, ht);
                    const f4 cz = (ht == 1 && NX == 5) ? xc[4] : PRE ? kq[1] : c4(G::C1L0, 4 + ht);
                    const f4 bhn = PRE ? kq[2] : c4(G::BHN0, ht);
                    NPD_TILES {
                        acc[tl][0] = fma4(xb[tl], cr, proj<SPLIT, NTL, ht>(P[tl]));
                        acc[tl][1] = fma4(xb[tl], cz, proj<SPLIT, NTL, 4 + ht>(P[tl]));
                        acc[tl][2] = bhn;
                    }
                }
                constexpr int TN[3] = {ht < 3 ? ht + 1 : 0, ht < 3 ? 5 + ht : 4, ht < 3 ? 9 + ht : 8};
                f4 cn;
                if constexpr (PRE) {
                    cn = c4(G::C1L0, 8 + ht);
                    if constexpr (ht < 3) ahead(G::C1L0, ht + 1, G::C1L0, 5 + ht, G::BHN0, ht + 1);
                    else ahead(G::C0L1, 0, G::C0L1, 4, G::BHN1, 0);
                }
                gemm16i<SPLIT, NTL, 3, 0, 12>(smem4, wbs[0], T, acc, fh, fl, cur, wbs[ht < 3 ? 0 : 2], TN, [&](auto cc) {
                    NPD_TILES u[tl].template step<decltype(cc)::value>(h0[tl][ht - 1], ap[tl][0], ap[tl][1], ainp[tl],
                                                                       ap[tl][2]);
                });
                if constexpr (!PRE) cn = c4(G::C1L0, 8 + ht);
                NPD_TILES {
                    ainp[tl] = fma4(xb[tl], cn, proj<SPLIT, NTL, 8 + ht>(P[tl]));
#pragma unroll
                    for (int k = 0; k < 3; ++k) ap[tl][k] = acc[tl][k];
                }
            });
            // ================= layer 1, hidden tile 0: W_hh1 h1 beside h0 tile 3's update and the h0' split
            f4 b[NTL][3], bi[NTL][3];
            {
                const f4 cr = PRE ? kq[0] : c4(G::C0L1, 0), cz = PRE ? kq[1] : c4(G::C0L1, 4);
                const f4 bhn = PRE ? kq[2] : c4(G::BHN1, 0);
                NPD_TILES {
                    b[tl][0] = cr;
                    b[tl][1] = cz;
                    b[tl][2] = bhn;
                }
            }
            f4 ci;  // the input-side GEMM's n-gate constant
            if constexpr (PRE) ci = c4(G::C0L1, 8);
            gemm16i<SPLIT, NTL, 3, 0, 14>(smem4, wbs[2], T0, b, gh, gl, cur, wbs[1], T0, [&](auto cc) {
                constexpr int c = decltype(cc)::value;
                NPD_TILES {
                    if constexpr (c < 12) u[tl].template step<c>(h0[tl][3], ap[tl][0], ap[tl][1], ainp[tl], ap[tl][2]);
                    else split_kb<SPLIT>(h0[tl], c - 12, fh[tl], fl[tl]);
                }
            });
            if constexpr (!PRE) ci = c4(G::C0L1, 8);
            NPD_TILES {
                bi[tl][0] = b[tl][0];
                bi[tl][1] = b[tl][1];
                bi[tl][2] = ci;
            }
            if constexpr (PRE) ahead(G::C0L1, 1, G::C0L1, 5, G::BHN1, 1);
            gemm16i<SPLIT, NTL, 3, 0, 0>(smem4, wbs[1], T0, bi, fh, fl, cur, wbs[2], T1, nowork);
            f4 q[NTL][4];  // r, z, in, hn of the previous layer-1 tile
            float part[NTL];
            NPD_TILES {
                q[tl][0] = bi[tl][0];
                q[tl][1] = bi[tl][1];
                q[tl][2] = bi[tl][2];
                q[tl][3] = b[tl][2];
                part[tl] = 0.0f;
            }
            static_for<1, 4>([&](auto htc) {
                constexpr int ht = decltype(htc)::value;
                const int T[3] = {ht, 4 + ht, 8 + ht};
                f4 bb[NTL][3], bbi[NTL][3];
                {
                    const f4 cr = PRE ? kq[0] : c4(G::C0L1, ht), cz = PRE ? kq[1] : c4(G::C0L1, 4 + ht);
                    const f4 bhn = PRE ? kq[2] : c4(G::BHN1, ht);
                    NPD_TILES {
                        bb[tl][0] = cr;
                        bb[tl][1] = cz;
                        bb[tl][2] = bhn;
                    }
                }
                // chunks 0-11: h1 tile ht - 1's update; 12: its output terms (count-only: in the decision chunk, where
                // the position is an information one)
                auto work = [&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    if constexpr (c < 12) {
                        NPD_TILES u[tl].template step<c>(h1[tl][ht - 1], q[tl][0], q[tl][1], q[tl][2], q[tl][3]);
                    } else if constexpr (!CNT) {
                        const f4 wl = c4(G::WLIN, ht - 1);
                        NPD_TILES {
#pragma unroll
                            for (int i = 0; i < 4; ++i) part[tl] = fmaf(wl[i], h1[tl][ht - 1][i], part[tl]);
                        }
                    }
                };
                if constexpr (PRE) ci = c4(G::C0L1, 8 + ht);
                gemm16i<SPLIT, NTL, 3, 0, 7>(smem4, wbs[2], T, bb, gh, gl, cur, wbs[1], T, work);
                if constexpr (!PRE) ci = c4(G::C0L1, 8 + ht);
                NPD_TILES {
                    bbi[tl][0] = bb[tl][0];
                    bbi[tl][1] = bb[tl][1];
                    bbi[tl][2] = ci;
                }
                if constexpr (PRE) {
                    if constexpr (ht < 3) ahead(G::C0L1, ht + 1, G::C0L1, 5 + ht, G::BHN1, ht + 1);
                    else kq[2] = c4(G::BHN0, 0);
                }
                constexpr int TN[3] = {ht < 3 ? ht + 1 : 0, ht < 3 ? 5 + ht : 4, ht < 3 ? 9 + ht : 8};
                gemm16i<SPLIT, NTL, 3, 7, 6>(smem4, wbs[1], T, bbi, fh, fl, cur, wbs[ht < 3 ? 2 : 0], TN, work);
                NPD_TILES {
                    q[tl][0] = bbi[tl][0];
                    q[tl][1] = bbi[tl][1];
                    q[tl][2] = bbi[tl][2];
                    q[tl][3] = bb[tl][2];
                }
            });
            // ================= tail: next step's layer-0 tile-0 GEMM beside h1 tile 3's update, the decision and the
            // h1 split.  This step's table word is read here, a GEMM ahead of the decision: LDS returns in order, so
            // its wait is a counted one behind the `cur` look-ahead
            const uint32_t tv = tab[ii];
            uint32_t te = 0u;
#pragma unroll
            for (int k = 0; k < NX; ++k) xc[k] = c4(G::C1L0, k < 3 ? 4 * k : 4 * k - 11);
            {
                const f4 bhn = PRE ? kq[2] : c4(G::BHN0, 0);
                NPD_TILES {
                    a0[tl][0] = zero;
                    a0[tl][1] = zero;
                    a0[tl][2] = bhn;
                }
            }
            if constexpr (PRE) kq[2] = c4(G::BHN0, 1);
            gemm16i<SPLIT, NTL, 3, 0, 15>(smem4, wbs[0], T0, a0, fh, fl, cur, wbs[0], T1, [&](auto cc) {
                constexpr int c = decltype(cc)::value;
                if constexpr (c < 12) {
                    NPD_TILES u[tl].template step<c>(h1[tl][3], q[tl][0], q[tl][1], q[tl][2], q[tl][3]);
                    if constexpr (c == 10) te = __builtin_amdgcn_readfirstlane(tv);
                } else if constexpr (c == 12) {
                    const bool info = (te >> 8) & 1u;
                    const uint32_t sl = te & 255u;  // message slot
                    float d[NTL];
                    if constexpr (CNT) {
                        NPD_TILES d[tl] = 1.0f;  // a frozen position's decision: no output, no reduction, no sign test
                        if (info) {
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const f4 wl = c4(G::WLIN, t);
                                NPD_TILES {
#pragma unroll
                                    for (int i = 0; i < 4; ++i) part[tl] = fmaf(wl[i], h1[tl][t][i], part[tl]);
                                }
                            }
                            NPD_TILES {
                                const float out = sum_rows16(part[tl]) + a.b_lin;
                                d[tl] = out > 0.0f ? 1.0f : (out < 0.0f ? -1.0f : 0.0f);
                            }
                        }
                    } else {
                        const int jj = a.rev ? N - 1 - ii : ii;
                        const f4 wl = c4(G::WLIN, 3);
                        NPD_TILES {
#pragma unroll
                            for (int i = 0; i < 4; ++i) part[tl] = fmaf(wl[i], h1[tl][3][i], part[tl]);
                            const float out = sum_rows16(part[tl]) + a.b_lin;
                            if (info) d[tl] = out > 0.0f ? 1.0f : (out < 0.0f ? -1.0f : 0.0f);
                            else d[tl] = a.gt ? a.gt[(seg * a.B + cwc[tl]) * N + jj] : 1.0f;
                            if (g4 == 0 && valid[tl]) {
                                if (a.decoded) a.decoded[rowoff[tl] + jj] = d[tl];
                                if (a.logits) a.logits[rowoff[tl] + ii] = out;
                            }
                        }
                    }
                    if (te & 512u) {  // compared: count_errors_kernel's test, rint(msg) != rint(d), on the 2-bit codes
                        const uint32_t q = sl >> 2;
                        NPD_TILES {
                            const uint32_t m01 = (q & 16u) ? mc[tl][1] : mc[tl][0], m23 = (q & 16u) ? mc[tl][3] : mc[tl][2];
                            const uint32_t mw = (q & 32u) ? m23 : m01;
                            const uint32_t dc = d[tl] > 0.0f ? 1u : (d[tl] < 0.0f ? 0u : 2u);
                            nerr[tl] += (g4 == (sl & 3u) && ((mw >> (2 * (q & 15u))) & 3u) != dc) ? 1u : 0u;
                        }
                    }
                    NPD_TILES {
                        const float sd = d[tl] > 0.0f ? 1.0f : (d[tl] < 0.0f ? -1.0f : 0.0f);
                        xb[tl] = a.onehot ? (sd > 0.0f ? 1.0f : 0.0f) : sd;
                    }
                } else {
                    NPD_TILES split_kb<SPLIT>(h1[tl], c - 13, gh[tl], gl[tl]);
                }
            });
        }
        if (count) {
            NPD_TILES {
                // the 16 codewords' errors: each row counted its slots; sum the four rows of every codeword
                uint32_t ne = nerr[tl];
                ne += __shfl_xor(ne, 16, 64);
                ne += __shfl_xor(ne, 32, 64);
                const bool mine = g4 == 0 && valid[tl];
                bl_w += (uint32_t)__builtin_popcountll(__ballot(mine && ne != 0u));
                uint32_t e = mine ? ne : 0u;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) e += __shfl_xor(e, o, 64);
                be_w += (uint32_t)__builtin_amdgcn_readfirstlane(e);
            }
            // flush when this wave's next unit is in another segment (or there is none): one atomic pair per
            // wave and segment
            const int64_t nt = unit + (int64_t)gridDim.x * WPB;
            if (nt >= nunits || nt / ups != seg) {
                if (lane == 0 && (be_w | bl_w)) {
                    atomicAdd(a.counters + 2 * seg, (unsigned long long)be_w);
                    atomicAdd(a.counters + 2 * seg + 1, (unsigned long long)bl_w);
                }
                be_w = bl_w = 0;
            }
        }
    }
}

// image of gru16p_kernel: weight fragments (hi, lo) in the 16x16x32 A-operand order, constants x kc
template <int SPLIT>
static void build_image16(const float* W, int N, int onehot, std::vector<float>& img, std::vector<float>& wy,
                          int64_t& wy_lo) {
    using G = Geo16;
    constexpr int F = 64, L = 2;
    const int Din = N + (onehot ? 2 : 1);
    const Weights u = unpack_weights(W, 3, F, L, Din);
    const auto &wih = u.wih, &bih = u.bih, &bhh = u.bhh;
    img.assign(G::TOTAL, 0.0f);
    // SPLIT 5: every gate row pre-multiplied by its exp2 constant (r, z: -log2 e; n: -2 log2 e; one fp32 rounding)
    auto fold = [&](int row) { return SPLIT == 5 ? (row < 2 * F ? -1.44269504088896340736f : -2.88539008177792681472f) : 1.0f; };
    uint16_t* u16 = reinterpret_cast<uint16_t*>(img.data());
    for (int g = 0; g < G::NG; ++g)
        for (int t = 0; t < G::RT; ++t)
            for (int kb = 0; kb < G::KB; ++kb)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int row = 16 * t + (l & 15);
                        const int hid = 16 * (2 * kb + (j >> 2)) + 4 * (l >> 4) + (j & 3);
                        uint16_t hi, lo;
                        split16<SPLIT>(fold(row) * u.mats[g][(size_t)row * F + hid], hi, lo);
                        const size_t e = (((((size_t)(g * G::RT + t) * G::KB + kb) * 2) * 64 + l) * 8 + j);
                        u16[e] = hi;
                        if (SPLIT >= 3) u16[e + 64 * 8] = lo;
                    }
    const float kc = SPLIT == 4 ? 65536.0f : 1.0f;
    auto col = [&](int row, int k) { return wih[0][(size_t)row * Din + k]; };
    for (int row = 0; row < 3 * F; ++row) {
        const bool rz = row < 2 * F;
        // x_i enters as c0 + x_i c1 (one-hot: columns N, N + 1 -> c0 = w_N, c1 = w_{N+1} - w_N; else c1 = w_N)
        const float c0x = onehot ? col(row, N) : 0.0f;
        const float c1x = onehot ? col(row, N + 1) - col(row, N) : col(row, N);
        img[G::C0L0 + row] = fold(row) * (kc * (rz ? bih[0][row] + bhh[0][row] + c0x : bih[0][row] + c0x));
        img[G::C1L0 + row] = fold(row) * (kc * c1x);
        img[G::C0L1 + row] = fold(row) * (kc * (rz ? bih[1][row] + bhh[1][row] : bih[1][row]));
    }
    for (int j = 0; j < F; ++j) {
        img[G::BHN0 + j] = fold(2 * F + j) * (kc * bhh[0][2 * F + j]);
        img[G::BHN1 + j] = fold(2 * F + j) * (kc * bhh[1][2 * F + j]);
        img[G::WLIN + j] = u.wlin[j];
    }
    wy_lo = fill_wy16<SPLIT>(wih[0], G::RT, 16, N, Din, fold, wy);
}

using Split16s = Combos<Combo<3>, Combo<5>, Combo<1>>;

void build_image_split16(npd_gru& g, const float* W, HostImages& im) {
    if (g.precision == 0 || g.F != 64 || g.layers != 2 || g.N % 32 != 0) return;
    // fp16x3 here is the unscaled split with the gate constants folded into the weights (SPLIT 5); the
    // 32-codeword kernels (other shapes) run the x 2^8-scaled split (SPLIT 4)
    g.split16 = split_of(g.precision, true);
    dispatch(Split16s{}, [&](auto sp) { build_image16<sp.value>(W, g.N, g.onehot, im.img16, im.wy16, g.wy16_lo); },
             g.split16);
}

int launch_split16(const npd_gru* g, const ArgsB& b, hipStream_t s) {
    const int64_t tps = (b.B + 15) / 16, nseg = b.nseg > 1 ? b.nseg : 1;
    // counting with nothing else to read or write: the count-only body, NT tiles per wave and 8 / NT waves per block
    if (b.counters && !b.decoded && !b.logits && !b.gt && !b.h0) {
        constexpr int NT = NPD_GRU16_CNT_TILES, WPB = NPD_GRU16_WPB / NT;
        const int64_t units = (tps + NT - 1) / NT * nseg;
        const int grid = grid_for((units + WPB - 1) / WPB, 1, device_cu_count());
        return dispatch(Split16s{}, [&](auto sp) {
            return launch_lds<gru16p_kernel<sp.value, true, NT>>("gru16p_kernel launch (count-only)", grid, 64 * WPB,
                                                                 Geo16::LDS_BYTES, s, b);
        }, g->split16);
    }
    const int grid = grid_for((tps * nseg + NPD_GRU16_WPB - 1) / NPD_GRU16_WPB, 1, device_cu_count());
    return dispatch(Split16s{}, [&](auto sp) {
        return launch_lds<gru16p_kernel<sp.value, false, 1>>("gru16p_kernel launch", grid, 64 * NPD_GRU16_WPB,
                                                             Geo16::LDS_BYTES, s, b);
    }, g->split16);
}

int launch_split16_sweep(const npd_gru* g, const Args& a, int n_seg, const float* msg, int K,
                         const uint8_t (&slot)[kMaxN], const uint32_t (&cmp)[kMaxWords], unsigned long long* counters,
                         hipStream_t s) {
    ArgsB b = make_args_b(g, a);
    b.msg = msg; b.counters = counters; b.K = K; b.nseg = n_seg;
    memcpy(b.slotw, slot, sizeof(slot));
    memcpy(b.cmp, cmp, sizeof(cmp));
    return launch_split16(g, b, s);
}

}  // namespace gru
}  // namespace npd

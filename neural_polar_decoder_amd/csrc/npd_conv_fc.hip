// npd_conv_fc.hip -- conv model, fp16x3: the three Linear layers' GEMMs on hi / lo fp16 planes.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "npd_conv_host.hpp"

namespace npd {
namespace conv {

constexpr int GK = 32;  // K block, as fc_kernel's
// ------------------------------------------------------------------------------ FC GEMM, fp16x3
// precision 3: the same 64 x 64 block tile on v_mfma_f32_32x32x16_f16, hi + lo fp16 operands, three products per
// multiply, fp32 accumulation.  X (activations, fp32) is split as it is staged (x 2^SA); W arrives pre-split on the
// host (hi and lo planes of fp16(w 2^SW), same row-major (Nout, K) layout).  LDS: per buffer four fp16 planes (A hi,
// A lo, B hi, B lo) of 64 rows x 32 k, row stride 40 (16-B aligned, conflict-free row reads); k-step s of a 32-wide K
// block reads k = 16 s + 8 h .. + 7 (one ds_read_b128 per plane).  6 MFMAs of 32 cycles per K block per wave against
// 16 fp32 MFMAs of 64.  Epilogue: descale 2^-(SW+SA) (exact), bias, GELU.
constexpr int GS16 = GK + 8;

__global__ __launch_bounds__(256) void fc_split_kernel(const float* __restrict__ X, const uint16_t* __restrict__ Whi,
                                                       const uint16_t* __restrict__ Wlo, const float* __restrict__ bias,
                                                       float* __restrict__ out, int M, int K, int Nout, int act,
                                                       int sw, const uint32_t* __restrict__ amax_in,
                                                       uint32_t* __restrict__ amax_out) {
    __shared__ __attribute__((aligned(16))) _Float16 sm[2][4][64 * GS16];
    const int sa = split_sa(amax_in);
    const float sa_scale = __builtin_ldexpf(1.0f, sa), descale = __builtin_ldexpf(1.0f, -(sw + sa));
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int m0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int msub = wave & 1, jsub = wave >> 1;
    // loader: A 64 rows x 32 k fp32 = 512 f4 (2 per thread); B planes 64 x 32 fp16 = 256 x 16 B (1 per thread each)
    f4 ra[2];
    f4 rbh, rbl;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx >> 3, c4 = (idx & 7) * 4;
            int mr = m0 + r;
            if (mr >= M) mr = M - 1;
            ra[u] = *reinterpret_cast<const f4*>(X + (int64_t)mr * K + k0 + c4);
        }
        const int r = tid >> 2, c8 = (tid & 3) * 8;
        rbh = *reinterpret_cast<const f4*>(Whi + (int64_t)(j0 + r) * K + k0 + c8);
        rbl = *reinterpret_cast<const f4*>(Wlo + (int64_t)(j0 + r) * K + k0 + c8);
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx >> 3, c4 = (idx & 7) * 4;
            hf4 hi, lo;
            split4(ra[u], sa_scale, hi, lo);
            *reinterpret_cast<hf4*>(&sm[buf][0][r * GS16 + c4]) = hi;
            *reinterpret_cast<hf4*>(&sm[buf][1][r * GS16 + c4]) = lo;
        }
        const int r = tid >> 2, c8 = (tid & 3) * 8;
        *reinterpret_cast<f4*>(&sm[buf][2][r * GS16 + c8]) = rbh;
        *reinterpret_cast<f4*>(&sm[buf][3][r * GS16 + c8]) = rbl;
    };
    f16v acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nk = K / GK;
    fetch(0);
    stash(0);
    __syncthreads();
    const int ar = (msub * 32 + col) * GS16 + 8 * h, br = (jsub * 32 + col) * GS16 + 8 * h;
    for (int kb = 0; kb < nk; ++kb) {
        const int cur = kb & 1;
        if (kb + 1 < nk) fetch((kb + 1) * GK);
#pragma unroll
        for (int st = 0; st < GK / 16; ++st) {
            const hf8 ah = *reinterpret_cast<const hf8*>(&sm[cur][0][ar + 16 * st]);
            const hf8 al = *reinterpret_cast<const hf8*>(&sm[cur][1][ar + 16 * st]);
            const hf8 bh = *reinterpret_cast<const hf8*>(&sm[cur][2][br + 16 * st]);
            const hf8 bl = *reinterpret_cast<const hf8*>(&sm[cur][3][br + 16 * st]);
            acc = mfma16(ah, bh, acc);
            acc = mfma16(ah, bl, acc);
            acc = mfma16(al, bh, acc);
        }
        if (kb + 1 < nk) stash(cur ^ 1);
        __syncthreads();
    }
    float amx = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + msub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int j = j0 + jsub * 32 + col;
        if (m < M) {
            float v = fmaf(acc[r], descale, bias[j]);
            if (act) v = gelu(v);
            out[(int64_t)m * Nout + j] = v;
            amx = fmaxf(amx, fabsf(v));
        }
    }
    if (amax_out != nullptr) publish_amax(amax_out, amx);
}

// fp16x3 FC GEMM with a BM x 128 block tile, BM = 128 or 256 (Nout a multiple of 128: FC0 at every N, FC1 / FC2 from
// N = 128; K is E N, 4 N or N, always a multiple of 32).  Tiles are dealt XCD by XCD (blocks b, b + 8, ... share an XCD
// and its L2): the column tiles of one row block run on one XCD, so X -- FC0 streams 537 MB of it per 4096 codewords at
// configs[4] -- comes from HBM about once (PMC of this kernel: 1.79 GB fetched per 4096-codeword FC0 against the 1.61 GB
// floor of X once + W once per XCD, profiles/round6/pmc_fc_final.txt).  What bounds it is not settled by any single
// resource: with the loads replaced by constants it ran 0.62 ms per 4096 codewords, with the MFMAs removed 0.8 ms, both
// together ~1.0 ms; deeper register rings, padded or panel-major operands (round 5), conflict-free LDS stores, a
// 256-row tile (25 % fewer operand bytes per MFMA) and fragment reads pinned a k-step ahead (round 6,
// profiles/round6/fc_tile_ab.txt) all measured within +-5 %.  The loader waves' split VALU shares each SIMD's issue
// port with the MFMA wave beside it (copy-only loaders on pre-split X: -12 %, fc0_presplit_ab.txt).
constexpr int FB = 128;

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// The waves are specialised (512 threads, two waves per SIMD): waves 0-3 only read fragments and issue MFMAs (64 x 64
// each, v_mfma_f32_32x32x16_f16, three per product); waves 4-7 only load, split (x 2^SA) and store.  The loaders keep
// FDL K blocks in flight in their registers and fill a 3-slot LDS ring two blocks ahead of the MFMA waves, which read
// the next block's first fragments during the current block's MFMAs; one LDS-only barrier per K block.  Against the
// round-4 kernel (4 waves each loading and computing, one per SIMD): 355-365 vs 386-412 us average over FC0-FC2.
constexpr int kFcFDL = 3;
// workgroup barrier that orders LDS only: a __syncthreads() also waits for every global load in flight (vmcnt(0)),
// which would drain the loaders' register ring at each K block
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
constexpr int kWspSlots = 3;
constexpr int kWspChain = 85;  // ring rounds (of kWspSlots K blocks) per accumulation chain of fc_split_wsp_kernel
// LDS image of one K block: 64-B rows (32 halfs) with the 16-B chunk q of row r stored at chunk q ^ ((r >> 2) & 3).
// The MFMA waves' ds_read_b128 (lane -> row col, chunk 2 st + h) then hit all 64 banks in each of its 16-lane groups
// (rows r and r + 4 of a 256-B bank line differ in the swizzle), and the loaders' stores -- ds_write_b64 of 2 rows x
// 8 x 8 B per 16 lanes, ds_write_b128 of 2 rows x 4 x 16 B per 8 lanes -- cover the 32 write banks once (bank
// (a/4) mod 32: two 64-B rows).  Round 5's padded 80-B rows were conflict-free for the reads only (a third of FC0's
// LDS cycles were store conflicts, profiles/round6/pmc_fc_final.txt) and do not fit three 256-row slots in 160 KB.
__device__ __forceinline__ int wsp_off(int r, int c) { return r * 32 + ((((c >> 3) ^ (r >> 2)) & 3) << 3) + (c & 7); }
__host__ __device__ constexpr size_t fc_wsp_lds(int bm) { return (size_t)kWspSlots * (2 * bm + 2 * FB) * 32 * 2; }
// PRE: X arrives already split (fp16 hi / lo planes of X 2^SA, row-major like X, written by split_planes_kernel), so the
// loaders only copy: 16-B loads of both planes into 16-B LDS stores, no split VALU.
// BM: rows (codewords) per block tile, 128 or 256, x 128 output features.  BM = 256 moves X 32 KB + W 16 KB per K block
// for twice the 128-row tile's MFMAs (each MFMA wave owns 128 x 64, TM = 4: 128 accumulator registers, 248 VGPRs); it
// runs where the chunk gives >= one 256-row tile per CU (npd_conv_forward_ex) at the same speed as BM = 128.
template <int FDL, bool PRE, int BM>
__global__ __launch_bounds__(512, 1) void fc_split_wsp_kernel(const float* __restrict__ X, const uint16_t* __restrict__ Xhi,
                                                              const uint16_t* __restrict__ Xlo,
                                                              const uint16_t* __restrict__ Whi,
                                                              const uint16_t* __restrict__ Wlo,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              int M, int K, int Nout, int act, int sw,
                                                              const uint32_t* __restrict__ amax_in,
                                                              uint32_t* __restrict__ amax_out) {
    constexpr int GKT = 32, NS = kWspSlots;
    static_assert(FDL >= 2 && FDL % NS == 0, "the prologue stashes two K blocks; LDS slots repeat with the ring");
    static_assert(BM == 128 || BM == 256, "block tile rows");
    constexpr int NL = 256;                            // loader threads
    constexpr int A4 = PRE ? GKT / 8 : GKT / 4, B8 = GKT / 8;  // 16-B pieces per A row (per plane), per B row
    constexpr int UA = BM * A4 / NL, UB = FB * B8 / NL;
    constexpr int TM = BM / 64, TN = 2;
    constexpr int PA = BM * 32, PB = FB * 32;  // halfs per A plane, per B plane
    constexpr int SLOT = 2 * PA + 2 * PB;
    const uint32_t am_raw = amax_in != nullptr ? __builtin_nontemporal_load(amax_in + (threadIdx.x & 63) * kAmaxStride) : 0u;
    extern __shared__ __attribute__((aligned(16))) _Float16 smb[];  // [slot][A hi, A lo (BM rows), B hi, B lo (128)][32]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool loader = wave >= 4;
    const int gx = Nout / FB;
    const int total = gridDim.x;
    int lin = blockIdx.x;
    if ((total & 7) == 0) lin = (blockIdx.x & 7) * (total >> 3) + (blockIdx.x >> 3);
    const int m0 = (lin / gx) * BM, j0 = (lin % gx) * FB;
    const int nk = K / GKT;
    const int sa = amax_in != nullptr ? min(kSplitSA, 15 - ((int)((wave_max_u32(am_raw) >> 23) & 0xFFu) - 126)) : kSplitSA;
    const float sa_scale = __builtin_ldexpf(1.0f, sa), descale = __builtin_ldexpf(1.0f, -(sw + sa));
    float amx = 0.0f;
    if (loader) {
        const int lt = tid - 256;
        // per-lane byte offsets (fixed for the launch) against wave-uniform K-block bases: one 32-bit address register
        // per load, no 64-bit address arithmetic per K block.  The offsets are relative to the block's first row of X
        // and of W (64-bit bases), so they stay below 256 K 4 B < 2^29 at the largest accepted K = 512 x 1024.
        // Piece idx -> row idx / A4: 16 (8) consecutive lanes store 2 whole rows, conflict-free (wsp_off)
        const char* const xblk = reinterpret_cast<const char*>(X) + (size_t)m0 * K * 4;
        const char* const xhblk = reinterpret_cast<const char*>(Xhi) + (size_t)m0 * K * 2;
        const char* const xlblk = reinterpret_cast<const char*>(Xlo) + (size_t)m0 * K * 2;
        const char* const hblk = reinterpret_cast<const char*>(Whi) + (size_t)j0 * K * 2;
        const char* const lblk = reinterpret_cast<const char*>(Wlo) + (size_t)j0 * K * 2;
        uint32_t offA[UA], offB[UB], ldsA[UA], ldsB[UB];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int idx = lt + NL * u;
            const int r = idx / A4, c4 = (idx % A4) * (PRE ? 8 : 4);
            const int mr = min(m0 + r, M - 1) - m0;  // row within the block: < BM
            offA[u] = (uint32_t)(((int64_t)mr * K + c4) * (PRE ? 2 : 4));
            ldsA[u] = (uint32_t)wsp_off(r, c4);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int idx = lt + NL * u;
            const int r = idx / B8, c8 = (idx % B8) * 8;
            offB[u] = (uint32_t)(((int64_t)r * K + c8) * 2);
            ldsB[u] = (uint32_t)wsp_off(r, c8);
        }
        f4 ra[FDL][UA], ral[FDL][PRE ? UA : 1], rbh[FDL][UB], rbl[FDL][UB];
        auto fetch = [&](int slot, int kb) {
            const int k0 = min(kb, nk - 1) * GKT;
            const char* const xk = xblk + (size_t)k0 * 4;
            const char* const hk = hblk + (size_t)k0 * 2;
            const char* const lk = lblk + (size_t)k0 * 2;
            if constexpr (PRE) {
#pragma unroll
                for (int u = 0; u < UA; ++u) {
                    ra[slot][u] = *reinterpret_cast<const f4*>(xhblk + (size_t)k0 * 2 + offA[u]);
                    ral[slot][u] = *reinterpret_cast<const f4*>(xlblk + (size_t)k0 * 2 + offA[u]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < UA; ++u) ra[slot][u] = *reinterpret_cast<const f4*>(xk + offA[u]);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                rbh[slot][u] = *reinterpret_cast<const f4*>(hk + offB[u]);
                rbl[slot][u] = *reinterpret_cast<const f4*>(lk + offB[u]);
            }
        };
        auto stash = [&](int slot, auto lds_slot) {
            _Float16* const base = smb + (size_t)decltype(lds_slot)::value * SLOT;
            if constexpr (PRE) {
#pragma unroll
                for (int u = 0; u < UA; ++u) {
                    *reinterpret_cast<f4*>(base + ldsA[u]) = ra[slot][u];
                    *reinterpret_cast<f4*>(base + PA + ldsA[u]) = ral[slot][u];
                }
            } else
#pragma unroll
            for (int u = 0; u < UA; ++u) {
                hf4 hi, lo;
                split4(ra[slot][u], sa_scale, hi, lo);
                *reinterpret_cast<hf4*>(base + ldsA[u]) = hi;
                *reinterpret_cast<hf4*>(base + PA + ldsA[u]) = lo;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                *reinterpret_cast<f4*>(base + 2 * PA + ldsB[u]) = rbh[slot][u];
                *reinterpret_cast<f4*>(base + 2 * PA + PB + ldsB[u]) = rbl[slot][u];
            }
        };
        // block b lives in register slot b % FDL from its fetch to its stash into LDS slot b % NS
        static_for<0, FDL>([&](auto i) { fetch(i.value, i.value); });
        stash(0, std::integral_constant<int, 0>{});
        stash(1, std::integral_constant<int, 1>{});
        fetch(0, FDL);
        fetch(1, FDL + 1);
        lds_barrier();
        // step k: the MFMA waves read slot k % NS; the loaders stash block k + 2 and fetch block k + 2 + FDL
        int kb = 0;
        for (; kb + FDL <= nk; kb += FDL)
            static_for<0, FDL>([&](auto i) {
                constexpr int RS = (i.value + 2) % FDL;
                stash(RS, std::integral_constant<int, (i.value + 2) % NS>{});
                fetch(RS, kb + i.value + 2 + FDL);
                lds_barrier();
            });
        static_for<0, FDL>([&](auto i) {
            if (kb + i.value < nk) {
                constexpr int RS = (i.value + 2) % FDL;
                stash(RS, std::integral_constant<int, (i.value + 2) % NS>{});
                lds_barrier();
            }
        });
    } else {
        __builtin_amdgcn_s_setprio(1);
        const int h = lane >> 5, col = lane & 31;
        const int wm = wave & 1, wn = wave >> 1;
        f16v acc[TM][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
                acc[a][b] = f16v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // fragment rows wm 32 TM + 32 t + col (A) and wn 64 + 32 t + col (B): every tile base is a multiple of 32, so
        // the swizzle of chunk 2 st + h depends on col only
        const int xr = (col >> 2) & 3;
        const int cq0 = ((0 + h) ^ xr) << 3, cq1 = ((2 + h) ^ xr) << 3;
        const int ar = (wm * 32 * TM + col) * 32, br = (wn * 32 * TN + col) * 32;
        struct Frags {
            hf8 ah[TM], al[TM], bh[TN], bl[TN];
        };
        auto read = [&](int slot, int st, Frags& f) {
            const _Float16* const cb = smb + (size_t)slot * SLOT + (st ? cq1 : cq0);
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                f.ah[t] = *reinterpret_cast<const hf8*>(cb + ar + t * 32 * 32);
                f.al[t] = *reinterpret_cast<const hf8*>(cb + PA + ar + t * 32 * 32);
            }
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                f.bh[t] = *reinterpret_cast<const hf8*>(cb + 2 * PA + br + t * 32 * 32);
                f.bl[t] = *reinterpret_cast<const hf8*>(cb + 2 * PA + PB + br + t * 32 * 32);
            }
        };
        Frags f[2];
        lds_barrier();
        read(0, 0, f[0]);
        // slot (kb + 1) % NS was complete at the barrier that ended step kb - 1, so its first k-step's fragments are
        // read during step kb's MFMAs (the loaders write slot (kb + 2) % NS meanwhile)
        auto step = [&](auto slot_c) {
            constexpr int SL = decltype(slot_c)::value;  // kb % NS
#pragma unroll
            for (int st = 0; st < GKT / 16; ++st) {
                if (st + 1 < GKT / 16)
                    read(SL, st + 1, f[(st + 1) & 1]);
                else
                    read((SL + 1) % NS, 0, f[(st + 1) & 1]);
                const Frags& c = f[st & 1];
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b) {
                        acc[a][b] = mfma16(c.ah[a], c.bh[b], acc[a][b]);
                        acc[a][b] = mfma16(c.ah[a], c.bl[b], acc[a][b]);
                        acc[a][b] = mfma16(c.al[a], c.bh[b], acc[a][b]);
                    }
            }
            lds_barrier();
        };
        // One fp32 accumulation chain covers kWspChain ring rounds (255 K blocks, 8160 terms): a single chain over
        // FC0's K = E N terms rounds about sqrt(K) times (11 x a blocked fp32 GEMM's error at K = 65536,
        // tests/conv_layers_helper.py).  A finished chain's sums are parked in this lane's own elements of out (no
        // registers are free for a second accumulator set at BM = 256) and added back in the epilogue; K <= 8160 never
        // parks, and both block tiles park at the same K.  Later chains are added with fire-and-forget atomics on
        // elements only this lane touches, in program order, so the sum is deterministic.
        auto park = [&](bool add) {
            // opaque to the optimiser, so that the 16 TM TN addresses are formed here, not kept live across the K loop
            int lm = wm * 32 * TM + 4 * h, lj = wn * 32 * TN + col;
            asm volatile("" : "+v"(lm), "+v"(lj));
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    const int j = j0 + lj + 32 * b;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + lm + 32 * a + (r & 3) + 8 * (r >> 2);
                        if (m < M) {
                            float* const p = out + (int64_t)m * Nout + j;
                            // atomic accesses throughout (the epilogue's load too), so the one location is coherent
                            // for this lane; the add returns nothing, so nothing waits for a load
                            if (add) __hip_atomic_fetch_add(p, acc[a][b][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            else __hip_atomic_store(p, acc[a][b][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        acc[a][b][r] = 0.0f;
                    }
                }
        };
        bool parked = false;
        int kb = 0;
        for (;;) {
            int kend = kb + NS * kWspChain;
            if (nk - kend <= 32) kend = nk;  // a rest of up to 1024 terms joins the last chain
            for (; kb + NS <= kend; kb += NS) static_for<0, NS>([&](auto i) { step(i); });
            if (kend == nk) break;
            park(parked);
            parked = true;
        }
        static_for<0, NS>([&](auto i) {
            if (kb + i.value < nk) step(i);
        });
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int j = j0 + wn * 32 * TN + 32 * b + col;
                const float bj = bias[j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * 32 * TM + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < M) {
                        const float sum = parked ? __hip_atomic_load(out + (int64_t)m * Nout + j, __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_AGENT) + acc[a][b][r]
                                                 : acc[a][b][r];
                        float v = fmaf(sum, descale, bj);
                        if (act) v = gelu(v);
                        out[(int64_t)m * Nout + j] = v;
                        amx = fmaxf(amx, fabsf(v));
                    }
                }
            }
    }
    if (amax_out != nullptr) publish_amax(amax_out, amx);
}

// X (n floats, n % 4 == 0) -> fp16 planes hi = fp16(x 2^SA), lo = fp16(x 2^SA - hi), SA from the producer's max |x| as
// in every split consumer (split_sa): the operands fc_split_wsp_kernel<.., true> copies instead of splitting
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ X, int64_t n4,
                                                           const uint32_t* __restrict__ amax_in,
                                                           uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
    const float sc = __builtin_ldexpf(1.0f, split_sa(amax_in));
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(X) + i);
        hf4 h, l;
        split4(v, sc, h, l);
        reinterpret_cast<hf4*>(hi)[i] = h;
        reinterpret_cast<hf4*>(lo)[i] = l;
    }
}

// ------------------------------------------------------------------------------ host
void pack_fc_split(const float* w, LayerPlan& L, std::vector<float>& img) {
    const int64_t n = (int64_t)L.cin * L.cout, plane = (n + 7) / 8 * 4;  // floats per (16-B aligned) fp16 plane
    L.sw = split_sw(w, n);
    const float sc = ldexpf(1.0f, L.sw);
    L.woff = append_aligned(img, (size_t)2 * plane);
    L.wlo = L.woff + plane;
    uint16_t* hp = reinterpret_cast<uint16_t*>(img.data() + L.woff);
    uint16_t* lp = reinterpret_cast<uint16_t*>(img.data() + L.wlo);
    for (int64_t i = 0; i < n; ++i) split_hi_lo(w[i] * sc, hp + i, lp + i);
}

// A/B switch NPD_FC0_PRESPLIT=0/1 (default 0): FC0 on pre-split X planes (split_planes_kernel + fc_split_wsp_kernel<..,
// true>).  Round 6 (profiles/round6/fc0_presplit_ab.txt): with copy-only loaders FC0 takes 935-938 us
// per 4096 codewords against 1,061 us splitting in its loaders (-12 %), but the separate split pass costs 197 us, so the
// default keeps the in-loader split; a split fused into the producing conv layer's epilogue would bound the gain at
// those 12 % of FC0 (~3 % of the forward) -- the FC0 GEMM is not bound by its loaders' split work
static bool fc0_presplit() {
    const char* e = getenv("NPD_FC0_PRESPLIT");
    return e != nullptr && atoi(e) != 0;
}
// A/B switch NPD_FC_BM = 128 / 256 (default 0: automatic): FC block-tile rows, see fc_split_wsp_kernel
static int fc_bm_env() {
    const char* e = getenv("NPD_FC_BM");
    const int v = e == nullptr ? 0 : atoi(e);
    return v == 128 || v == 256 ? v : 0;  // anything else: automatic (the grid is sized for the tile actually launched)
}

int launch_fc_split(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    const uint16_t* wh = reinterpret_cast<const uint16_t*>(a.img + L.woff);
    const uint16_t* wl = reinterpret_cast<const uint16_t*>(a.img + L.wlo);
    const float* bias = a.img + L.boff;
    const int M = (int)a.nb, K = L.cin, Nout = L.cout;
    if (L.family != kFcWsp) {
        hipLaunchKernelGGL(fc_split_kernel, dim3(Nout / 64, (unsigned)((a.nb + 63) / 64)), dim3(256), 0, s, a.in, wh, wl,
                           bias, a.out, M, K, Nout, L.res, L.sw, a.am_in, a.am_out);
        return launch_check("fc_split_kernel launch");
    }
    auto wsp = [&](auto pre, auto bm, const uint16_t* xh, const uint16_t* xl) {
        constexpr int BM = decltype(bm)::value;
        return launch_lds<fc_split_wsp_kernel<kFcFDL, decltype(pre)::value, BM>>(
            "fc_split_wsp_kernel launch", (unsigned)((Nout / FB) * ((a.nb + BM - 1) / BM)), 512, fc_wsp_lds(BM), s, a.in,
            xh, xl, wh, wl, bias, a.out, M, K, Nout, L.res, L.sw, a.am_in, a.am_out);
    };
    using std::false_type, std::true_type;
    using BM128 = std::integral_constant<int, 128>;
    if (a.planes != nullptr && fc0_presplit()) {
        // FC0's X split once into fp16 planes in a free activation buffer, then copied by the GEMM's loaders
        uint16_t* xh = a.planes;
        uint16_t* xl = xh + a.nb * K;
        const int64_t n4 = a.nb * K / 4;
        const int gs = (int)std::min<int64_t>((n4 + 255) / 256, (int64_t)device_cu_count() * 8);
        hipLaunchKernelGGL(split_planes_kernel, dim3(gs), dim3(256), 0, s, a.in, n4, a.am_in, xh, xl);
        return wsp(true_type{}, BM128{}, xh, xl);
    }
    // 256-row tiles where they alone give every CU a tile (FC0 of an 8192-codeword chunk at N >= 256), else 128 x 128
    const int64_t t256 = (Nout / FB) * ((a.nb + 255) / 256);
    const int bm = fc_bm_env() ? fc_bm_env() : (t256 >= device_cu_count() ? 256 : 128);
    if (bm == 256) return wsp(false_type{}, std::integral_constant<int, 256>{}, nullptr, nullptr);
    return wsp(false_type{}, BM128{}, nullptr, nullptr);
}

}  // namespace conv
}  // namespace npd

// npd_gru_wide_list.hip -- CRISP GRU list decoder at hidden 256 / 512 (RNN_decoder.list_decode, rnn_all.py:563-664):
// gru_list_kernel's column map and list semantics (npd_gru_list.hip) on gru_wide_kernel's step (npd_gru_wide.hip).
//
// One workgroup of NW = 8 waves owns a 32-column tile = 32 / Lp codewords x Lp path slots (Lp = L rounded up to 1, 2, 4
// or 8), column = cw * Lp + slot.  The step is the greedy wide kernel's, operation for operation: weights streamed from
// L2 / MALL in the handle's permuted image, both layers' states in LDS in B-operand order, each wave updating its HPW
// hidden tiles, and the part[] reduction that leaves every wave holding `out` of every column.  So L = 1 is
// gru_wide_kernel bit for bit.
//
// Everything per column -- the path metric, the path's bit words, the previous bit x_i and the prune decision -- is
// computed by every wave, redundantly and identically, from that reduced `out`; nothing about it crosses waves.  What
// does is the hidden state: after a prune that moves a column, each wave permutes the columns of the hidden tiles it
// owns, in both layers: it reads Hs[(4 jt + q) 64 + half 32 + parent(col)] into registers and writes them to its own
// lane position (a wave's LDS operations execute in order, and the 64-lane chunk read is the chunk written).  One
// workgroup barrier follows before the next step's GEMMs read the state; the branch is workgroup-uniform because every
// wave derives the same map, and it is skipped, barrier included, when no column of the tile moves (always while the
// list fills: the slots of a codeword are bit-identical copies and a fork only flips bits).
#include "npd_gru_list.hpp"
#include "npd_gru_wide.hpp"

namespace npd {
namespace gru {

// CA: list_finish's CRC-aided / counting epilogue (npd_gru_list.hpp), run by wave 0 like the plain one
template <int F, int L, bool CA>
__global__ __launch_bounds__(64 * WideGeo<F>::NW) void gru_wide_list_kernel(const ListArgs a) {
    using G = Geo<F, L>;
    using WG = WideGeo<F>;
    constexpr int TT = G::TT, HT = G::HT, KG = G::KG, NW = WG::NW, HPW = WG::HPW;
    extern __shared__ __attribute__((aligned(16))) f4 lds4[];
    const int N = a.N;
    f4* const Hs0 = lds4;
    f4* const Hs1 = lds4 + (L == 2 ? F * 8 : 0);
    f4* const Ys = lds4 + L * F * 8;
    float* const part = reinterpret_cast<float*>(Ys + N * 8);
    const float* img = a.img;
    const f4* W0 = reinterpret_cast<const f4*>(img);
    const f4* W1 = reinterpret_cast<const f4*>(img + (size_t)G::G_SIZE);
    const f4* W2 = reinterpret_cast<const f4*>(img + 2 * (size_t)G::G_SIZE);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int col = lane & 31;
    const int jt0 = wave * HPW;
    const int ng = N / 8;
    const int lpl = a.lp_log2, Lp = 1 << lpl;
    const int slot = col & (Lp - 1);
    const int base = lane - slot;  // this codeword's slot 0, in this lane half
    const int cpt = 32 >> lpl;     // codewords per tile
    const uint32_t gmask = (1u << Lp) - 1u;
    const int64_t ntiles = (a.B + cpt - 1) / cpt;
    const f16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float one_or_zero = half ? 0.0f : 1.0f;
    constexpr int R = 0, Z = 1, IN = 2, HN = 3;
    [[maybe_unused]] unsigned long long cnt[3] = {0ull, 0ull, 0ull};  // CA: wave 0's error counts (wave-uniform)

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t cw = tile * cpt + (col >> lpl);
        const bool valid = cw < a.B;
        const int64_t cwc = valid ? cw : a.B - 1;
        __syncthreads();  // the previous tile's last readers are done
        {
            // the slots of a codeword hold the same Fy column; both layers' states start at zero
            const f4* yr = reinterpret_cast<const f4*>(a.fy + cwc * N + half * (N / 2));
            for (int q = wave; q < ng; q += NW) Ys[q * 64 + lane] = yr[q];
            for (int i = threadIdx.x; i < L * F * 8; i += NW * 64) lds4[i] = f4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        float xb = 1.0f;   // x_i of this column's path: onehot index of its previous bit (or its sign); +1 after frozen
        float met = 0.0f;  // path metric
        uint32_t bw[kMaxWords];  // the path's bits, bit i of word i / 32 set = position i decided -1
#pragma unroll
        for (int w = 0; w < kMaxWords; ++w) bw[w] = 0u;
        int ls = 1;  // live list size (the same for every codeword)

        for (int ii = 0; ii < N; ++ii) {
            const float xbe = half ? xb : 1.0f;
            f16v acc[4][HPW];
            f16v top[HPW];
            // ================= layer 0 (as gru_wide_kernel)
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < HPW; ++j) acc[k][j] = zero;
            wide_chain<HPW, R, Z, IN>(a.wy, ng, HT, jt0, Ys, lane, acc);
            wide_chain<HPW, R, Z, HN>(W0, KG, HT, jt0, Hs0, lane, acc);
#pragma unroll
            for (int j = 0; j < HPW; ++j) {
                const int jt = jt0 + j;
                acc[R][j] = mfma(img[G::OFF_X + (0 * TT + jt) * 64 + lane], xbe, acc[R][j]);
                acc[Z][j] = mfma(img[G::OFF_X + (0 * TT + HT + jt) * 64 + lane], xbe, acc[Z][j]);
                acc[HN][j] = mfma(img[G::OFF_X + (0 * TT + 2 * HT + jt) * 64 + lane], xbe, acc[HN][j]);
                acc[IN][j] = mfma(img[G::OFF_IN + jt * 64 + lane], xbe, acc[IN][j]);
            }
            __syncthreads();  // every wave has read h0
#pragma unroll
            for (int j = 0; j < HPW; ++j) wide_update<HPW>(Hs0, jt0 + j, lane, top[j], acc[R][j], acc[Z][j], acc[IN][j], acc[HN][j]);
            __syncthreads();  // h0' complete
            if constexpr (L == 2) {
                // ================= layer 1 (as gru_wide_kernel)
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < HPW; ++j) acc[k][j] = zero;
                wide_chain<HPW, R, Z, IN>(W1, KG, HT, jt0, Hs0, lane, acc);
#pragma unroll
                for (int j = 0; j < HPW; ++j) {
                    const int jt = jt0 + j;
                    acc[R][j] = mfma(img[G::OFF_X + (TT + jt) * 64 + lane], one_or_zero, acc[R][j]);
                    acc[Z][j] = mfma(img[G::OFF_X + (TT + HT + jt) * 64 + lane], one_or_zero, acc[Z][j]);
                    acc[IN][j] = mfma(img[G::OFF_X + (TT + 2 * HT + jt) * 64 + lane], one_or_zero, acc[IN][j]);
                }
                wide_chain<HPW, R, Z, HN>(W2, KG, HT, jt0, Hs1, lane, acc);
#pragma unroll
                for (int j = 0; j < HPW; ++j)
                    acc[HN][j] = mfma(img[G::OFF_X + (2 * TT + 2 * HT + jt0 + j) * 64 + lane], one_or_zero, acc[HN][j]);
                __syncthreads();  // every wave has read h1
#pragma unroll
                for (int j = 0; j < HPW; ++j)
                    wide_update<HPW>(Hs1, jt0 + j, lane, top[j], acc[R][j], acc[Z][j], acc[IN][j], acc[HN][j]);
            }
            // ================= output: Linear(F, 1) on the top layer, reduced over the waves in a fixed order
            float p = 0.0f;
#pragma unroll
            for (int j = 0; j < HPW; ++j)
#pragma unroll
                for (int i = 0; i < 16; ++i) p += img[G::OFF_WL + (half * HT + jt0 + j) * 16 + i] * top[j][i];
            p += __shfl_xor(p, 32, 64);
            if (half == 0) part[wave * 32 + col] = p;
            __syncthreads();  // every wave's updates of this step are in LDS, too
            float out = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) out += part[w * 32 + col];
            out += a.b_lin;

            const bool info = (a.info[ii >> 5] >> (ii & 31)) & 1u;
            if (!info) {  // frozen: only the state advances; the bit stays +1
                xb = 1.0f;
                continue;
            }
            // ================= information position: fork, prune (every wave alike), gather
            const float ao = fabsf(out);
            uint32_t neg = out < 0.0f ? 1u : 0u;  // the kept child's bit is sign(out) (an exact 0 counts as +1)
            bool flip;
            if (2 * ls <= a.L) {
                // filling: slot s already holds its parent (path s mod ls); its new path index is s mod 2 ls
                flip = (slot & (2 * ls - 1)) >= ls;
                if (flip) met += ao;
                ls *= 2;
            } else {
                const int src = list_prune(met, neg, flip, ao, ls, a.L, lane, slot, base, gmask);
                // the same lanes move in every wave, so this branch and its barrier are workgroup-uniform
                if (__ballot(src != lane) != 0ull) {
#pragma unroll
                    for (int w = 0; w < kMaxWords; ++w)
                        if (32 * w < N) bw[w] = (uint32_t)__shfl((int)bw[w], src, 64);
                    // this wave's hidden tiles, both layers: column <- parent column, inside the lane half
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        f4* const Hs = l == 0 ? Hs0 : Hs1;
                        f4 v[HPW][4];
#pragma unroll
                        for (int j = 0; j < HPW; ++j)
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[j][q] = Hs[(4 * (jt0 + j) + q) * 64 + src];
#pragma unroll
                        for (int j = 0; j < HPW; ++j)
#pragma unroll
                            for (int q = 0; q < 4; ++q) Hs[(4 * (jt0 + j) + q) * 64 + lane] = v[j][q];
                    }
                    __syncthreads();  // the permuted state is complete before the next step's GEMMs read it
                }
                ls = a.L;
            }
            neg ^= flip ? 1u : 0u;
#pragma unroll
            for (int w = 0; w < kMaxWords; ++w) bw[w] |= (w == (ii >> 5)) ? (neg << (ii & 31)) : 0u;
            xb = a.onehot ? (neg ? 0.0f : 1.0f) : (neg ? -1.0f : 1.0f);
        }

        // ================= epilogue (every wave holds every column's path: wave 0 finishes them)
        if (wave == 0) {
            if constexpr (CA)
                list_finish<true>(a, bw, met, ls, cw, cwc, valid, half, slot, base, cnt);
            else
                list_finish(a, bw, met, ls, cw, cwc, valid, half, slot, base);
        }
    }
    if constexpr (CA) {
        if (wave == 0) list_count_flush(a, cnt, lane);
    }
}

// one tile of 32 >> lp_log2 codewords per workgroup of NW waves, as many workgroups per CU as LDS and registers allow
template <int F, int L, bool CA>
static int launch_wide_list_tiles(const npd_gru* g, const ListArgs& a, hipStream_t s) {
    constexpr int NW = WideGeo<F>::NW;
    constexpr auto kern = gru_wide_list_kernel<F, L, CA>;
    const size_t lds = (size_t)wide_lds_bytes(g->N, F, L);
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 64 * NW, lds) != hipSuccess || occ <= 0) {
        (void)hipGetLastError();
        occ = 1;
    }
    const int cpt = 32 >> a.lp_log2;
    return launch_lds<kern>("gru_wide_list_kernel launch", grid_for((a.B + cpt - 1) / cpt, occ, device_cu_count()), 64 * NW,
                            lds, s, a);
}

int launch_wide_list(const npd_gru* g, const ListArgs& a, bool ca, hipStream_t s) {
    using Shapes = Combos<Combo<512, 2>, Combo<512, 1>, Combo<256, 2>, Combo<256, 1>>;  // WideShapes without F = 128
    if (ca)
        return dispatch(Shapes{}, [&](auto f, auto l) { return launch_wide_list_tiles<f.value, l.value, true>(g, a, s); },
                        g->F, g->layers);
    return dispatch(Shapes{}, [&](auto f, auto l) { return launch_wide_list_tiles<f.value, l.value, false>(g, a, s); },
                    g->F, g->layers);
}

}  // namespace gru
}  // namespace npd

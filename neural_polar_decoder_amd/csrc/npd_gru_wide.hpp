// npd_gru_wide.hpp -- what the weight-streaming GRU kernels share (npd_gru_wide.hip: gru_wide_kernel;
// npd_gru_wide_list.hip: gru_wide_list_kernel): the workgroup geometry, the streamed GEMM chain and the update of one
// hidden tile against the LDS state.  The list kernel's L = 1 equals the greedy kernel bit for bit because both run
// these, in the same order.
#pragma once

#include "npd_gru_host.hpp"

namespace npd {
namespace gru {

template <int F>
struct WideGeo {
    static constexpr int HT = F / 32;
    static constexpr int NW = HT < 8 ? HT : 8;
    static constexpr int HPW = HT / NW;
};

// acc[D0|D1|D2][j] += W[tiles k*HT + jt0 + j, k = 0, 1, 2] . B over kg groups of 4 k-steps.
// W: f4 image of one matrix ([tile][group][lane]), B: LDS state in B-operand order ([group][lane]).
template <int HPW, int D0, int D1, int D2>
__device__ __forceinline__ void wide_chain(const f4* __restrict__ W, int kg, int HT, int jt0,
                                           const f4* __restrict__ Bs, int lane, f16v (&acc)[4][HPW]) {
    constexpr int D[3] = {D0, D1, D2};
    f4 wc[3][HPW];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < HPW; ++j) wc[k][j] = W[((size_t)(k * HT + jt0 + j) * kg + 0) * 64 + lane];
    for (int q = 0; q < kg; ++q) {
        f4 wn[3][HPW];
        if (q + 1 < kg) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < HPW; ++j) wn[k][j] = W[((size_t)(k * HT + jt0 + j) * kg + q + 1) * 64 + lane];
        }
        const f4 b = Bs[q * 64 + lane];
        asm volatile("" ::: "memory");
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < HPW; ++j) acc[D[k]][j] = mfma(wc[k][j][e], b[e], acc[D[k]][j]);
        if (q + 1 < kg) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < HPW; ++j) wc[k][j] = wn[k][j];
        }
    }
}

// one hidden tile's GRU update against its old value in the LDS state (B-operand order)
template <int HPW>
__device__ __forceinline__ void wide_update(f4* __restrict__ Hs, int jt, int lane, f16v& hv, const f16v& ar,
                                            const f16v& az, const f16v& ain, const f16v& ahn) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f4 v = Hs[(4 * jt + q) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[4 * q + e] = v[e];
    }
    gru_update(hv, ar, az, ain, ahn);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = hv[4 * q + e];
        Hs[(4 * jt + q) * 64 + lane] = v;
    }
}

}  // namespace gru
}  // namespace npd

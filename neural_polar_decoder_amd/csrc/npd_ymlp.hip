// npd_ymlp.hip -- y MLP (decoding_type 'y_h0').
// One Linear layer + activation of RNN_Model.get_h0 / get_Fy (rnn_all.py:362-385): out[b][j] = act(sum_k x[b][k]
// W[j][k] + bias[j]), fp32, k summed in order.  64 x 64 outputs per 256-thread block (4 x 4 per thread, strided by
// 16 so a row's 16 lanes read consecutive W rows from LDS), K in LDS-staged chunks of 16.  Once per codeword (the
// MLP is < 2 % of a hidden-64 decode's MACs), so plain FMA, no MFMA.
#include "npd_common.hpp"

namespace npd {
namespace gru {
constexpr int MK = 16;

__device__ __forceinline__ float mlp_act(float x, int act) {
    switch (act) {
        case 1: return x > 0.0f ? x : 0.0f;                                           // relu
        case 2: return 1.0507009873554805f * (x > 0.0f ? x : 1.6732632423543772f * expm1f(x));  // selu
        case 3: return x > 0.0f ? x : expm1f(x);                                      // elu (alpha 1)
        case 4: return tanhf(x);
        case 5: return 1.0f / (1.0f + expf(-x));                                      // sigmoid
        default: return x;                                                            // linear / unknown
    }
}

__global__ __launch_bounds__(256) void mlp_layer_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int64_t B, int K, int Nout, int act) {
    __shared__ float xs[64][MK + 1];
    __shared__ float ws[64][MK + 1];
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
    const int64_t m0 = (int64_t)blockIdx.y * 64;
    const int j0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += MK) {
        for (int e = tid; e < 64 * MK; e += 256) {
            const int r = e / MK, k = e % MK;
            const int64_t m = m0 + r;
            const int j = j0 + r;
            xs[r][k] = (m < B && k0 + k < K) ? x[m * K + k0 + k] : 0.0f;
            ws[r][k] = (j < Nout && k0 + k < K) ? W[(int64_t)j * K + k0 + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MK; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(xs[ty + 16 * i][k], ws[tx + 16 * c][k], acc[i][c]);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + ty + 16 * i;
        if (m >= B) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (j < Nout) out[m * Nout + j] = mlp_act(acc[i][c] + bias[j], act);
        }
    }
}
}  // namespace gru
}  // namespace npd

using namespace npd;

extern "C" int npd_ymlp_layer(const float* x, const float* W, const float* bias, float* out, int64_t B, int K, int Nout,
                              int act, void* stream) {
    NPD_ARG(B >= 0 && K > 0 && Nout > 0, "npd_ymlp_layer: bad sizes");
    if (B == 0) return NPD_OK;
    NPD_ARG(x != nullptr && W != nullptr && bias != nullptr && out != nullptr, "npd_ymlp_layer: null pointer");
    NPD_ARG(act >= 0 && act <= 5, "npd_ymlp_layer: act must be 0 (linear), 1 relu, 2 selu, 3 elu, 4 tanh, 5 sigmoid");
    NPD_ARG(B <= (int64_t)65535 * 64, "npd_ymlp_layer: B too large for one launch (split the batch)");
    dim3 grid((unsigned)((Nout + 63) / 64), (unsigned)((B + 63) / 64));
    hipLaunchKernelGGL(gru::mlp_layer_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, W, bias, out, B, K, Nout, act);
    return launch_check("mlp_layer_kernel launch");
}

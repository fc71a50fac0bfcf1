// npd_conv_train.hpp -- what the conv training kernels' file (npd_conv_train.hip) exports to the plan and the C ABI
// (npd_conv_train_api.hip), and the sizing rules both sides share.  No device code here.
#pragma once

#include <algorithm>

#include "npd_conv_host.hpp"

namespace npd {
namespace conv {

// floats of conv_layer_kernel's A-operand image of R rows (padded to 64-row tiles) and C contraction channels
inline int64_t conv_img_floats(int R, int C) {
    const int64_t t32n = (R + 63) / 64 * 2;
    return C == 1 ? t32n * 256 : t32n * 7 * (C / 8) * 256;
}

// the partial sums of one weight gradient may take this many floats of scratch at the most
constexpr int64_t kPartCap = (int64_t)64 << 20;

// conv dW: `items` 64-position items over S workgroups per tile, *ipb items each: 16 items (one 1024-term chain) per
// workgroup until S would pass 4096 or the partials kPartCap; past that a workgroup's chain grows with the batch
inline int conv_dw_splits(int64_t items, int cin, int cout, int* ipb) {
    int64_t S = (items + 15) / 16;
    const int64_t cap = kPartCap / ((int64_t)cout * cin * 7);
    if (S > 4096) S = 4096;
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    *ipb = (int)std::max<int64_t>(1, (items + S - 1) / S);  // items = 0 (an empty batch): one empty split
    return (int)((items + *ipb - 1) / *ipb);
}

// Linear dW: M words over S splits of *rps words (a multiple of 32): enough splits for about 1024 workgroups, at least
// 128 words each, the partials within kPartCap
inline int fc_dw_splits(int64_t M, int64_t J, int64_t K, int* rps) {
    const int64_t tiles = (J / 64) * (K / 64);
    int64_t S = (1024 + tiles - 1) / tiles;
    const int64_t by_words = (M + 127) / 128, cap = kPartCap / (J * K);
    if (S > by_words) S = by_words;
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    const int64_t r = std::max<int64_t>(32, ((M + S - 1) / S + 31) / 32 * 32);  // M = 0: no split at all
    *rps = (int)r;
    return (int)((M + r - 1) / r);
}

// column sums: kColsumRows rows per split (4 chains of 1024 terms)
constexpr int kColsumRows = 4096;
inline int colsum_splits(int64_t M) { return (int)((M + kColsumRows - 1) / kColsumRows); }

// Every launcher returns NPD_OK or the failed launch's code.  `part` is scratch for the partial sums.
int train_pack_conv(const float* w, float* img, int cout, int cin, int flip, hipStream_t s);
int train_pack_fc(const float* w, float* img, int J, int64_t K, int mode, int E, int N, hipStream_t s);
// forward (bwd = false): zout = conv(in) + bias, out = gelu(zout) (+ res).  dX (bwd = true): wimg the flipped image, cin /
// cout swapped by the caller; v = conv(in) (+ res); gout = v (or NULL); out = v * GELU'(gz)
int train_conv_layer(bool bwd, const float* in, float* out, const float* res, const float* wimg, const float* bias,
                     float* zout, const float* gz, float* gout, int cin, int cout, int N, int dil, int64_t B,
                     hipStream_t s);
// v = X Wt^T (+ bias); zout = v (or NULL); gelu if act; * GELU'(gz) (or NULL); out = v.  K % 32 == 0, Nout % 64 == 0
int train_fc(const float* X, const float* Wt, const float* bias, float* out, float* zout, const float* gz, int64_t M,
             int64_t K, int64_t Nout, int act, hipStream_t s);
// grad (J, K) = dZ^T X; permE > 0: FC0, column l E + c is written at c N + l
int train_fc_dw(const float* dZ, const float* X, float* part, float* grad, int64_t M, int64_t J, int64_t K, int permE,
                int permN, hipStream_t s);
int train_conv_dw(const float* dZ, const float* X, float* part, float* grad, int cin, int cout, int N, int dil, int64_t B,
                  hipStream_t s);
int train_colsum(const float* A, float* part, float* grad, int64_t M, int C, hipStream_t s);
int train_ln_fwd(float* d, const float* drop, const float* g, const float* be, float* logits, float* mean, float* rstd,
                 int64_t M, int N, hipStream_t s);
int train_ln_bwd(const float* d, const float* drop, const float* g, const float* dy, const float* mean, const float* rstd,
                 float* dz, float* dgt, int64_t M, int N, hipStream_t s);

}  // namespace conv
}  // namespace npd

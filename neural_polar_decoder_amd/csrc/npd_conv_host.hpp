// npd_conv_host.hpp -- host side of the conv model: the per-layer launch plan npd_conv_create (npd_conv_api.hip) decides
// once, what each kernel family's file (npd_conv.hip, npd_conv_slab.hip, npd_conv_ws.hip, npd_conv_fc.hip) exports to
// it, and the host helpers they share.  No device code here.
#pragma once

#include <string.h>

#include <vector>

#include "npd_conv_common.hpp"
#include "npd_launch.hpp"

namespace npd {
namespace conv {

// The kernel family that runs a layer.  fp32 (precision 0, and layer 0's cin = 1 at every precision): conv_layer_kernel
// and fc_kernel.  fp16x3 conv layers: cin 32 / 64 / 128 on conv_ws16_kernel, other cin <= 64 on conv_split_ws_kernel,
// wider ones (80, 96, ...: a 2-part split of 96 channels spills) on conv_layer_split_kernel.  fp16x3 Linear layers:
// fc_split_wsp_kernel where Nout is a multiple of its 128 columns (FC0 at every N, FC1 / FC2 from N = 128), else
// fc_split_kernel.
enum Family { kConvF32, kConvSlab, kConvWs, kConvWs16, kFcF32, kFcSplit, kFcWsp };

// One conv or Linear layer as planned at create time: the family, its template instantiation, and the one weight image
// that instantiation reads.  Linear layers: cin = K, cout = Nout, res = apply GELU.
struct LayerPlan {
    int family, cin, cout, dil;
    int res;              // 1: add the block input (residual) after GELU
    int kdim, q, parts;   // kConvWs: NG, Q, KS; kConvWs16: KB, Q, KP; kConvSlab: q = P
    int64_t woff, boff;   // offsets (floats) into the device image: weights (fp16x3: the fragments / the hi plane), bias
    int64_t wlo;          // the Linear layers' fp16 lo plane
    int sw;  // fp16x3: the weight scale exponent SW (the kernels descale by 2^-(SW + SA), SA from the input's range)
};

// one launch of a layer on a chunk of nb codewords: img = the handle's device image, res = the residual source or NULL,
// am_in / am_out = the input's and output's activation-range words (fp16x3) or NULL, planes = FC0 only: room for X's
// fp16 planes (4 B per element of X) should NPD_FC0_PRESPLIT ask for them
struct LayerArgs {
    const float* in;
    float* out;
    const float *res, *img;
    int N;
    int64_t nb;
    const uint32_t* am_in;
    uint32_t* am_out;
    uint16_t* planes;
};

// ---------------------------------------------------------------------------------- host packing, fp16x3
// SW of a weight tensor: max |w| 2^SW in [2^12, 2^13)
inline int split_sw(const float* w, int64_t n) {
    float m = 0.0f;
    for (int64_t i = 0; i < n; ++i) m = fmaxf(m, fabsf(w[i]));
    return m > 0.0f ? 12 - (int)floorf(log2f(m)) : 0;
}
// v (already scaled by 2^SW) -> hi = fp16(v), lo = fp16(v - hi)
inline void split_hi_lo(float v, uint16_t* hi, uint16_t* lo) {
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    memcpy(hi, &h, 2);
    memcpy(lo, &l, 2);
}
inline int64_t append_aligned(std::vector<float>& img, size_t n) {  // 16-B aligned room for n floats, zeroed
    img.resize((img.size() + 3) / 4 * 4 + n, 0.0f);
    return (int64_t)(img.size() - n);
}
// A fragments of a conv layer's weights w (cout, cin, 7) x 2^SW for MFMA tiles of R = 32 rows (32x32x16: the slab and
// conv_split_ws kernels) or 16 rows (16x16x32: conv_ws16_kernel): [tile][tap][K block][part hi / lo][lane][8 x fp16].
// Lane l holds row l % R of its tile and, as element j, channel KB kb + 8 (l / R) + j of K block kb, KB = 512 / R
// channels per block; rows past cout and channels past cin are zero.  Sets L.woff and L.sw.
inline void pack_conv_split(const float* w, LayerPlan& L, int R, std::vector<float>& img) {
    const int co = L.cout, ci = L.cin, KB = 512 / R;
    const int tiles = (co + 63) / 64 * 64 / R, nkb = (ci + KB - 1) / KB;
    L.sw = split_sw(w, (int64_t)co * ci * 7);
    const float sc = ldexpf(1.0f, L.sw);
    L.woff = append_aligned(img, (size_t)tiles * 7 * nkb * 2 * 64 * 8 / 2);
    uint16_t* u16 = reinterpret_cast<uint16_t*>(img.data() + L.woff);
    for (int tile = 0; tile < tiles; ++tile)
        for (int t = 0; t < 7; ++t)
            for (int kb = 0; kb < nkb; ++kb)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int row = R * tile + l % R, cc = KB * kb + 8 * (l / R) + j;
                        const float v = (row < co && cc < ci) ? w[((int64_t)row * ci + cc) * 7 + t] * sc : 0.0f;
                        const size_t e = ((((size_t)(tile * 7 + t) * nkb + kb) * 2) * 64 + l) * 8 + j;
                        split_hi_lo(v, &u16[e], &u16[e + 64 * 8]);
                    }
}

// LDS bytes of conv_layer_split_kernel<P>: a hi and a lo plane of 64 P positions plus the halo, cin16 + 8 halfs a row
inline size_t slab_lds_bytes(int cin, int P, int dil) {
    return (size_t)2 * (64 * P + 6 * dil) * (((cin + 15) & ~15) + 8) * 2;
}

// ---------------------------------------------------------------------------------- what the family files export
// Each launch_* runs the instantiation the plan names (NPD_ENOTSUP if the family has none such); pack_* appends the
// image its kernels read and sets L.woff (pack_fc_split: the hi / lo planes of w (Nout, K) x 2^SW; L.wlo and L.sw too).
typedef int LaunchFn(const LayerPlan& L, const LayerArgs& a, hipStream_t s);
void pack_conv_f32(const float* w, LayerPlan& L, std::vector<float>& img);
void pack_fc_split(const float* w, LayerPlan& L, std::vector<float>& img);
LaunchFn launch_conv_f32, launch_fc_f32;       // npd_conv.hip
LaunchFn launch_conv_slab;                     // npd_conv_slab.hip
LaunchFn launch_conv_ws, launch_conv_ws16;     // npd_conv_ws.hip
LaunchFn launch_fc_split;                      // npd_conv_fc.hip: kFcSplit and kFcWsp
int launch_channels_first(const float* in, float* out, int N, int C, int64_t nb, hipStream_t s);  // npd_conv.hip
int launch_layernorm_sign(const float* x, const float* g, const float* be, float* logits, float* dec, int64_t M, int N,
                          hipStream_t s);

}  // namespace conv
}  // namespace npd

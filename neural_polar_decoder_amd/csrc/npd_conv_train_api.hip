// npd_conv_train_api.hip -- convNet training: the plan (image buffers, no weights), the workspace layout and the C ABI
// (include/npd.h).  The kernels are in npd_conv_train.hip.
#include <algorithm>
#include <new>

#include "npd_conv_train.hpp"

using namespace npd;
using namespace npd::conv;

struct npd_conv_train {
    int N, E, device;
    int cin[kLayers], cout[kLayers], dil[kLayers];
    int64_t w[kLayers + 3], b[kLayers + 3], ln[2], n_weights;  // offsets into the flat weight / gradient vector
    int64_t fimg[kLayers], bimg[kLayers], fc0f, fcb[3];        // offsets into img: forward / backward images
    float* img;
};

namespace {

int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }

// `saved`: per conv layer z and the output, then FC0 z | out, FC1 z | out, the dropout-scaled FC2 output, mean, rstd
struct Saved {
    int64_t z[kLayers], a[kLayers], z10, h1, z11, h2, d, mean, rstd, total;
};
Saved saved_layout(const npd_conv_train* p, int64_t B) {
    Saved L;
    int64_t o = 0;
    const int64_t N = p->N;
    for (int i = 0; i < kLayers; ++i) {
        L.z[i] = o;
        o += B * N * p->cout[i];
        L.a[i] = o;
        o += B * N * p->cout[i];
    }
    L.z10 = o, o += B * 4 * N;
    L.h1 = o, o += B * 4 * N;
    L.z11 = o, o += B * N;
    L.h2 = o, o += B * N;
    L.d = o, o += B * N;
    L.mean = o, o += up4(B);
    L.rstd = o, o += up4(B);
    L.total = o;
    return L;
}

// `scratch`: two gradient buffers of (B, N, E), two skip-gradient buffers of (B, N, E / 2), the LayerNorm weight's
// per-word products (B, N), then the partial sums of the largest reduction
struct Scratch {
    int64_t ga, gb, sa, sb, dgt, part, total;
};
Scratch scratch_layout(const npd_conv_train* p, int64_t B) {
    Scratch L;
    const int64_t N = p->N, E = p->E;
    int64_t o = 0;
    L.ga = o, o += B * N * E;
    L.gb = o, o += B * N * E;
    L.sa = o, o += B * N * (E / 2);
    L.sb = o, o += B * N * (E / 2);
    L.dgt = o, o += B * N;
    L.part = o;
    int64_t need = 0;
    for (int i = 0; i < kLayers; ++i) {
        int ipb;
        need = std::max(need, (int64_t)conv_dw_splits(B * (N / 64), p->cin[i], p->cout[i], &ipb) * p->cout[i] * p->cin[i] * 7);
        need = std::max(need, (int64_t)colsum_splits(B * N) * p->cout[i]);
    }
    const int64_t fj[3] = {4 * N, N, N}, fk[3] = {E * N, 4 * N, N};
    for (int f = 0; f < 3; ++f) {
        int rps;
        const int S = fc_dw_splits(B, fj[f], fk[f], &rps);
        if (S > 1) need = std::max(need, S * fj[f] * fk[f]);
        need = std::max(need, (int64_t)colsum_splits(B) * fj[f]);
    }
    L.total = o + up4(need);
    return L;
}

}  // namespace

extern "C" int npd_conv_train_create(int N, int embed, npd_conv_train** out) {
    NPD_ARG(out != nullptr, "npd_conv_train_create: out is NULL");
    *out = nullptr;
    NPD_ARG(N >= 64 && N <= 1024 && N % 64 == 0, "npd_conv_train_create: N must be a multiple of 64 in [64, 1024]");
    NPD_ARG(embed >= 16 && embed <= 512 && embed % 16 == 0,
            "npd_conv_train_create: embed must be a multiple of 16 in [16, 512]");
    // layer 8's dX stages all `embed` channels of 64 + 24 positions in LDS: (embed + 4) 88 floats <= 160 KB
    if (embed > 448)
        return fail(NPD_ENOTSUP, "npd_conv_train_create: embed > 448 is not covered: the dX kernel of the dilation-4 layer "
                                 "with `embed` output channels stages (embed + 4) x 88 floats in LDS, past 160 KB");
    npd_conv_train* p = new (std::nothrow) npd_conv_train;
    if (!p) return fail(NPD_ENOMEM, "npd_conv_train_create: out of memory");
    memset(p, 0, sizeof(*p));
    p->N = N;
    p->E = embed;
    const int E = embed, H = E / 2;
    static const int dils[kLayers] = {1, 2, 4, 1, 2, 4, 1, 2, 4, 1};
    int64_t wo = 0, io = 0;
    for (int i = 0; i < kLayers; ++i) {
        p->cin[i] = i == 0 ? 1 : (i == 9 ? E : H);
        p->cout[i] = i >= 8 ? E : H;
        p->dil[i] = dils[i];
        p->w[i] = wo, wo += (int64_t)p->cout[i] * p->cin[i] * 7;
        p->b[i] = wo, wo += p->cout[i];
        p->fimg[i] = io, io += conv_img_floats(p->cout[i], p->cin[i]);
        p->bimg[i] = io;
        if (i > 0) io += conv_img_floats(p->cin[i], p->cout[i]);
    }
    const int64_t fj[3] = {4 * (int64_t)N, N, N}, fk[3] = {(int64_t)E * N, 4 * (int64_t)N, N};
    for (int f = 0; f < 3; ++f) {
        p->w[kLayers + f] = wo, wo += fj[f] * fk[f];
        p->b[kLayers + f] = wo, wo += fj[f];
    }
    p->ln[0] = wo, wo += N;
    p->ln[1] = wo, wo += N;
    p->n_weights = wo;
    p->fc0f = io, io += fj[0] * fk[0];
    for (int f = 0; f < 3; ++f) p->fcb[f] = io, io += fj[f] * fk[f];
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc(&p->img, (size_t)io * 4);
    if (e != hipSuccess) {
        delete p;
        return hip_fail(e, "npd_conv_train_create");
    }
    *out = p;
    return NPD_OK;
}

extern "C" int npd_conv_train_destroy(npd_conv_train* p) {
    NPD_ARG(p != nullptr, "npd_conv_train_destroy: plan is NULL");
    if (p->img) (void)hipFree(p->img);
    delete p;
    return NPD_OK;
}

extern "C" int npd_conv_train_workspace(const npd_conv_train* p, int64_t B, int64_t* saved_floats,
                                        int64_t* scratch_floats) {
    NPD_ARG(p != nullptr, "npd_conv_train_workspace: plan is NULL");
    NPD_ARG(saved_floats != nullptr && scratch_floats != nullptr, "npd_conv_train_workspace: null pointer");
    NPD_ARG(B >= 0 && B <= ((int64_t)1 << 22), "npd_conv_train_workspace: B must be in [0, 2^22]");
    *saved_floats = saved_layout(p, B).total;
    *scratch_floats = scratch_layout(p, B).total;
    return NPD_OK;
}

static bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

extern "C" int npd_conv_train_forward(npd_conv_train* p, const float* weights_dev, const float* y,
                                      const float* drop_mult_or_null, float* logits, float* saved, int64_t B,
                                      void* stream) {
    NPD_ARG(p != nullptr, "npd_conv_train_forward: plan is NULL");
    NPD_ARG(B >= 0 && B <= ((int64_t)1 << 22), "npd_conv_train_forward: B must be in [0, 2^22]");
    NPD_ARG(weights_dev != nullptr, "npd_conv_train_forward: weights_dev is NULL");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr && logits != nullptr && saved != nullptr, "npd_conv_train_forward: null pointer");
    NPD_ARG(aligned16(weights_dev) && aligned16(saved) && aligned16(y),
            "npd_conv_train_forward: weights_dev, y and saved must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int N = p->N, E = p->E;
    const Saved S = saved_layout(p, B);
    const float* W = weights_dev;
    int rc;
    for (int i = 0; i < kLayers; ++i)
        if ((rc = train_pack_conv(W + p->w[i], p->img + p->fimg[i], p->cout[i], p->cin[i], 0, s))) return rc;
    if ((rc = train_pack_fc(W + p->w[kLayers], p->img + p->fc0f, 4 * N, (int64_t)E * N, 0, E, N, s))) return rc;
    for (int i = 0; i < kLayers; ++i) {
        const float* in = i == 0 ? y : saved + S.a[i - 1];
        const float* res = (i == 3 || i == 5 || i == 7) ? saved + S.a[i - 2] : nullptr;  // the block input
        if ((rc = train_conv_layer(false, in, saved + S.a[i], res, p->img + p->fimg[i], W + p->b[i], saved + S.z[i], nullptr,
                                   nullptr, p->cin[i], p->cout[i], N, p->dil[i], B, s)))
            return rc;
    }
    if ((rc = train_fc(saved + S.a[9], p->img + p->fc0f, W + p->b[10], saved + S.h1, saved + S.z10, nullptr, B,
                       (int64_t)E * N, 4 * N, 1, s)))
        return rc;
    if ((rc = train_fc(saved + S.h1, W + p->w[11], W + p->b[11], saved + S.h2, saved + S.z11, nullptr, B, 4 * N, N, 1, s)))
        return rc;
    if ((rc = train_fc(saved + S.h2, W + p->w[12], W + p->b[12], saved + S.d, nullptr, nullptr, B, N, N, 0, s))) return rc;
    return train_ln_fwd(saved + S.d, drop_mult_or_null, W + p->ln[0], W + p->ln[1], logits, saved + S.mean,
                        saved + S.rstd, B, N, s);
}

extern "C" int npd_conv_train_backward(npd_conv_train* p, const float* weights_dev, const float* y,
                                       const float* drop_mult_or_null, const float* grad_logits, const float* saved,
                                       float* scratch, float* grad_weights_dev, int64_t B, void* stream) {
    NPD_ARG(p != nullptr, "npd_conv_train_backward: plan is NULL");
    NPD_ARG(B >= 0 && B <= ((int64_t)1 << 22), "npd_conv_train_backward: B must be in [0, 2^22]");
    NPD_ARG(weights_dev != nullptr && grad_weights_dev != nullptr, "npd_conv_train_backward: null weight pointer");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        NPD_HIP(hipMemsetAsync(grad_weights_dev, 0, (size_t)p->n_weights * 4, s));
        return NPD_OK;
    }
    NPD_ARG(y != nullptr && grad_logits != nullptr && saved != nullptr && scratch != nullptr,
            "npd_conv_train_backward: null pointer");
    NPD_ARG(aligned16(weights_dev) && aligned16(saved) && aligned16(y) && aligned16(scratch) && aligned16(grad_weights_dev),
            "npd_conv_train_backward: weights_dev, y, saved, scratch and grad_weights_dev must be 16-byte aligned");
    const int N = p->N, E = p->E;
    const Saved S = saved_layout(p, B);
    const Scratch C = scratch_layout(p, B);
    const float* W = weights_dev;
    float* G = grad_weights_dev;
    float* part = scratch + C.part;
    int rc;
    for (int i = 1; i < kLayers; ++i)
        if ((rc = train_pack_conv(W + p->w[i], p->img + p->bimg[i], p->cout[i], p->cin[i], 1, s))) return rc;
    const int64_t fj[3] = {4 * (int64_t)N, N, N}, fk[3] = {(int64_t)E * N, 4 * (int64_t)N, N};
    for (int f = 0; f < 3; ++f)
        if ((rc = train_pack_fc(W + p->w[kLayers + f], p->img + p->fcb[f], (int)fj[f], fk[f], f == 0 ? 1 : 2, E, N, s)))
            return rc;
    float* bufs[2] = {scratch + C.ga, scratch + C.gb};
    int cur = 0;  // bufs[cur] holds the current layer's dZ
    // LayerNorm and dropout
    if ((rc = train_ln_bwd(saved + S.d, drop_mult_or_null, W + p->ln[0], grad_logits, saved + S.mean, saved + S.rstd,
                           bufs[cur], scratch + C.dgt, B, N, s)))
        return rc;
    if ((rc = train_colsum(scratch + C.dgt, part, G + p->ln[0], B, N, s))) return rc;
    if ((rc = train_colsum(grad_logits, part, G + p->ln[1], B, N, s))) return rc;
    // Linear layers, last to first: X = the layer's input, gz = the z its input came from
    const float* fx[3] = {saved + S.a[9], saved + S.h1, saved + S.h2};
    const float* fgz[3] = {saved + S.z[9], saved + S.z10, saved + S.z11};
    for (int f = 2; f >= 0; --f) {
        const float* dZ = bufs[cur];
        if ((rc = train_fc_dw(dZ, fx[f], part, G + p->w[kLayers + f], B, fj[f], fk[f], f == 0 ? E : 0, N, s))) return rc;
        if ((rc = train_colsum(dZ, part, G + p->b[kLayers + f], B, (int)fj[f], s))) return rc;
        if ((rc = train_fc(dZ, p->img + p->fcb[f], nullptr, bufs[cur ^ 1], nullptr, fgz[f], B, fj[f], fk[f], 0, s))) return rc;
        cur ^= 1;
    }
    // conv layers, last to first.  G_i, the whole gradient at layer i's output, is kept for i = 7, 5, 3: it also
    // arrives along the skip at the output two layers before
    float* skips[2] = {scratch + C.sa, scratch + C.sb};
    int sk = 0;  // skips[sk ^ 1] holds the last G kept
    for (int i = kLayers - 1; i >= 0; --i) {
        const float* dZ = bufs[cur];
        const float* X = i == 0 ? y : saved + S.a[i - 1];
        if ((rc = train_conv_dw(dZ, X, part, G + p->w[i], p->cin[i], p->cout[i], N, p->dil[i], B, s))) return rc;
        if ((rc = train_colsum(dZ, part, G + p->b[i], B * N, p->cout[i], s))) return rc;
        if (i == 0) break;
        const int j = i - 1;  // the layer whose output this dX is the gradient of
        const float* skip = (j == 1 || j == 3 || j == 5) ? skips[sk ^ 1] : nullptr;
        float* keep = (j == 3 || j == 5 || j == 7) ? skips[sk] : nullptr;
        if ((rc = train_conv_layer(true, dZ, bufs[cur ^ 1], skip, p->img + p->bimg[i], nullptr, nullptr, saved + S.z[j], keep,
                                   p->cout[i], p->cin[i], N, p->dil[i], B, s)))
            return rc;
        if (keep) sk ^= 1;
        cur ^= 1;
    }
    return NPD_OK;
}

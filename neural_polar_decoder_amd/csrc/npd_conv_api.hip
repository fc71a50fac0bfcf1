// npd_conv_api.hip -- conv model: the handle, the per-layer plan decided at create time and the C ABI (include/npd.h).
// The kernels and their image builders are in npd_conv.hip (fp32, LayerNorm, transpose), npd_conv_slab.hip,
// npd_conv_ws.hip and npd_conv_fc.hip (fp16x3); npd_conv_host.hpp is what they export.
#include <algorithm>
#include <new>

#include "npd_conv_host.hpp"

using namespace npd;
using namespace npd::conv;

struct npd_conv {
    int N, E, precision, device;
    LayerPlan layers[kLayers + 3];  // the plan: the 10 conv layers, then the Linear layers FC0 .. FC2
    float* img;                     // device: each layer's one weight image and its bias, then the LN params
    int64_t off_ln[2];
};

static void conv_spec(int E, int idx, int& cin, int& cout, int& dil, int& res) {
    const int H = E / 2;
    // (cin, cout, dilation, residual-after) for layers1.0, layers1.2, layers2.0, ..., layers5.2
    static const int dils[kLayers] = {1, 2, 4, 1, 2, 4, 1, 2, 4, 1};
    dil = dils[idx];
    cin = idx == 0 ? 1 : (idx == 9 ? E : H);
    cout = idx >= 8 ? E : H;
    res = (idx == 3 || idx == 5 || idx == 7) ? 1 : 0;
}

// Which kernel family and instantiation runs conv layer L (cin, cout, dil set) at code length N: decided here, once;
// the packer packs the one image that choice reads and the forward loop launches it.
static void plan_conv(int N, int precision, LayerPlan& L) {
    const bool q2 = N % 128 == 0;  // the weight-stationary kernels walk 128-position items where N allows
    if (L.cin == 1 || precision != 3) {
        L.family = kConvF32;
    } else if (L.cin == 32 || L.cin == 64 || L.cin == 128) {
        // each wave holds all input channels of its 16 output channels; cin 128: two channel parts of 64, 64-position
        // items
        L.family = kConvWs16;
        L.kdim = L.cin / 32;
        L.parts = L.kdim == 4 ? 2 : 1;
        L.q = L.parts == 1 && q2 ? 2 : 1;
    } else if (L.cin <= 64) {
        // cin <= 48: no channel parts; 56: 2 channel parts, 64-position items.  (conv_spec's dilation <= 4 bounds the
        // halo both weight-stationary kernels are sized for.)
        L.family = kConvWs;
        L.kdim = (L.cin + 15) / 16;
        L.parts = L.kdim <= 3 ? 1 : 2;
        L.q = L.parts == 1 && q2 ? 2 : 1;
    } else {
        // positions per block 64 P: P = 2 where 128 <= N and the two fp16 slab planes fit, else 1.  (P = 4 reuses
        // each weight fragment over 4 position tiles but its 80 KB slab leaves one block per CU, no overlap of
        // one block's staging with another's MFMAs: configs[4] forward 11.6-12.1 ms at P = 4, 10.3-10.6 at
        // P = 2, 10.6-10.7 at P = 1 per 8192 codewords, profiles/round4/conv_p_ab.txt)
        L.family = kConvSlab;
        L.q = 2;
        while (L.q > 1 && (64 * L.q > N || slab_lds_bytes(L.cin, L.q, L.dil) > 160 * 1024)) L.q >>= 1;
    }
}

static int launch_layer(const LayerPlan& L, const LayerArgs& a, hipStream_t s) {
    static LaunchFn* const by_family[] = {launch_conv_f32, launch_conv_slab, launch_conv_ws, launch_conv_ws16,
                                          launch_fc_f32,   launch_fc_split,  launch_fc_split};  // enum Family's order
    return by_family[L.family](L, a, s);
}

extern "C" int npd_conv_create(int N, int embed, const float* weights, int64_t n_weights, int precision,
                               npd_conv** out) {
    NPD_ARG(out != nullptr, "npd_conv_create: out is NULL");
    *out = nullptr;
    NPD_ARG(weights != nullptr, "npd_conv_create: weights is NULL");
    NPD_ARG(N >= 64 && N <= 1024 && N % 64 == 0, "npd_conv_create: N must be a multiple of 64 in [64, 1024]");
    NPD_ARG(embed >= 16 && embed <= 512 && embed % 16 == 0, "npd_conv_create: embed must be a multiple of 16 in [16, 512]");
    NPD_ARG(precision == 0 || precision == 3, "npd_conv_create: precision must be 0 (fp32) or 3 (fp16x3 conv layers)");
    const int E = embed;
    // host weights in state_dict order: (w, b) per conv layer, then 3 x (w, b) Linear, then LN (g, b)
    int64_t expect = 0;
    for (int i = 0; i < kLayers; ++i) {
        int ci, co, d, r;
        conv_spec(E, i, ci, co, d, r);
        expect += (int64_t)co * ci * 7 + co;
    }
    expect += (int64_t)4 * N * E * N + 4 * N + (int64_t)N * 4 * N + N + (int64_t)N * N + N + 2 * N;
    NPD_ARG(n_weights == expect, "npd_conv_create: weight count does not match (N, embed)");
    npd_conv* c = new (std::nothrow) npd_conv;
    if (!c) return fail(NPD_ENOMEM, "npd_conv_create: out of memory");
    memset(c, 0, sizeof(*c));
    c->N = N;
    c->E = E;
    c->precision = precision;
    std::vector<float> img;
    const float* p = weights;
    for (int i = 0; i < kLayers; ++i) {
        LayerPlan& L = c->layers[i];
        conv_spec(E, i, L.cin, L.cout, L.dil, L.res);
        plan_conv(N, precision, L);
        if (L.family == kConvF32) pack_conv_f32(p, L, img);  // p: (cout, cin, 7)
        else pack_conv_split(p, L, L.family == kConvWs16 ? 16 : 32, img);
        p += (int64_t)L.cout * L.cin * 7;
        L.boff = append_aligned(img, (size_t)(L.cout + 63) / 64 * 64);  // zero-padded to the 64-channel tiles
        std::copy(p, p + L.cout, img.begin() + L.boff);
        p += L.cout;
    }
    const int fk[3] = {E * N, 4 * N, N}, fo[3] = {4 * N, N, N};
    for (int f = 0; f < 3; ++f) {
        LayerPlan& L = c->layers[kLayers + f];
        L.cin = fk[f];
        L.cout = fo[f];
        L.res = f < 2;  // GELU after FC0 and FC1
        L.family = precision != 3 ? kFcF32 : (fo[f] % 128 == 0 ? kFcWsp : kFcSplit);
        const int64_t n = (int64_t)fk[f] * fo[f];
        const float* w = p;
        std::vector<float> perm;
        if (f == 0) {
            // the activations are (B, N, E): flatten index l*E + c instead of torch's c*N + l
            perm.resize(n);
            for (int64_t j = 0; j < fo[0]; ++j)
                for (int cc = 0; cc < E; ++cc)
                    for (int l = 0; l < N; ++l) perm[j * fk[0] + (int64_t)l * E + cc] = p[j * fk[0] + (int64_t)cc * N + l];
            w = perm.data();
        }
        if (L.family == kFcF32) {
            L.woff = append_aligned(img, n);
            std::copy(w, w + n, img.begin() + L.woff);
        } else {
            pack_fc_split(w, L, img);
        }
        p += n;
        L.boff = (int64_t)img.size();
        img.insert(img.end(), p, p + fo[f]);
        p += fo[f];
    }
    c->off_ln[0] = (int64_t)img.size();
    img.insert(img.end(), p, p + N);
    p += N;
    c->off_ln[1] = (int64_t)img.size();
    img.insert(img.end(), p, p + N);
    hipError_t e = hipGetDevice(&c->device);
    if (e == hipSuccess) e = hipMalloc(&c->img, img.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(c->img, img.data(), img.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (c->img) (void)hipFree(c->img);
        delete c;
        return hip_fail(e, "npd_conv_create");
    }
    *out = c;
    return NPD_OK;
}

extern "C" int npd_conv_destroy(npd_conv* c) {
    if (!c) return NPD_OK;
    if (c->img) (void)hipFree(c->img);
    delete c;
    return NPD_OK;
}

// codewords per pass: kChunk, halved (to >= 512) while the three (chunk, E, N) fp32 activation buffers would pass
// 4 GiB -- configs[4] (E N = 32768) keeps 8192 (3.2 GB); the widest accepted net (E 512, N 1024) runs 512
static int64_t chunk_of(const npd_conv* c, int64_t B) {
    int64_t ch = kChunk;
    while (ch > 512 && 3 * ch * (int64_t)c->E * c->N * 4 > ((int64_t)4 << 30)) ch >>= 1;
    return B < ch ? B : ch;
}

extern "C" int64_t npd_conv_workspace_bytes(const npd_conv* c, int64_t B) {
    if (!c || B <= 0) return 0;
    const int64_t Bc = chunk_of(c, B);
    // three activation buffers of (Bc, E, N) + FC1/FC2/FC3 outputs + the activation-range words (kAmaxSlots)
    return (3 * Bc * (int64_t)c->E * c->N + Bc * 4 * (int64_t)c->N + 2 * Bc * (int64_t)c->N) * 4 + 256 + (int64_t)kAmaxSlots * kAmaxWords * 4;
}

extern "C" int npd_conv_forward_tap(const npd_conv* c, const float* y, float* logits, float* decoded, int tap,
                                    float* tap_out, void* workspace, int64_t B, void* stream);

extern "C" int npd_conv_forward(const npd_conv* c, const float* y, float* logits, float* decoded, void* workspace,
                                int64_t B, void* stream) {
    return npd_conv_forward_tap(c, y, logits, decoded, 5, nullptr, workspace, B, stream);
}

// input4 is the tap after conv layer 5 (layers3 + residual)
extern "C" int npd_conv_forward_ex(const npd_conv* c, const float* y, float* logits, float* decoded, float* input4,
                                   void* workspace, int64_t B, void* stream) {
    return npd_conv_forward_tap(c, y, logits, decoded, 5, input4, workspace, B, stream);
}

// tap 0 .. 9: conv layer tap's output (after GELU and the residual) as channels-first (B, cout, N); tap 10 .. 12: the
// FC0 / FC1 / FC2 outputs (B, 4N) / (B, N) / (B, N), FC2 before LayerNorm.  Written only if tap_out != NULL.
extern "C" int npd_conv_forward_tap(const npd_conv* c, const float* y, float* logits, float* decoded, int tap,
                                    float* tap_out, void* workspace, int64_t B, void* stream) {
    NPD_ARG(c != nullptr, "npd_conv_forward: conv is NULL");
    NPD_ARG(B >= 0, "npd_conv_forward: B < 0");
    NPD_ARG(tap >= 0 && tap < kLayers + 3, "npd_conv_forward_tap: tap must be 0 .. 12");
    if (B == 0) return NPD_OK;
    NPD_ARG(y != nullptr && workspace != nullptr, "npd_conv_forward: null pointer");
    NPD_ARG(logits != nullptr || decoded != nullptr, "npd_conv_forward: nothing to write");
    hipStream_t s = (hipStream_t)stream;
    const int N = c->N, E = c->E;
    const int64_t Bc = chunk_of(c, B);
    float* ws = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* A0 = ws;
    float* A1 = A0 + Bc * (int64_t)E * N;
    float* A2 = A1 + Bc * (int64_t)E * N;
    float* H1 = A2 + Bc * (int64_t)E * N;
    float* H2 = H1 + Bc * 4 * (int64_t)N;
    float* H3 = H2 + Bc * (int64_t)N;
    uint32_t* amax = reinterpret_cast<uint32_t*>(H3 + Bc * (int64_t)N);
    const bool split = c->precision == 3;
    // fp16x3: layer j (conv 0 .. 9, FC 10 .. 12) reads its input's range at record j - 1 and publishes its output's at
    // record j; FC2 feeds the fp32 LayerNorm and publishes none
    auto am_in = [&](int j) { return split && j > 0 ? amax + (j - 1) * kAmaxWords : nullptr; };
    auto am_out = [&](int j) { return split && j < kLayers + 2 ? amax + j * kAmaxWords : nullptr; };
    for (int64_t b0 = 0; b0 < B; b0 += Bc) {
        const int64_t nb = (B - b0) < Bc ? (B - b0) : Bc;
        if (split) NPD_HIP(hipMemsetAsync(amax, 0, (size_t)kAmaxSlots * kAmaxWords * 4, s));
        // layer inputs/outputs: x (N floats per cw) -> A0 -> A1 -> ... ; block inputs kept for the residual
        float* bufs[3] = {A0, A1, A2};
        int in_idx = -1;   // -1: y
        int res_idx = -1;  // buffer holding the current block input
        for (int i = 0; i < kLayers; ++i) {
            const LayerPlan& L = c->layers[i];
            // choose an output buffer that is neither the input nor the pending residual
            int out_idx = 0;
            while (out_idx == in_idx || out_idx == res_idx) ++out_idx;
            float* o = bufs[out_idx];
            int rc = launch_layer(L, {in_idx < 0 ? y + b0 * N : bufs[in_idx], o, L.res ? bufs[res_idx] : nullptr, c->img, N,
                                      nb, am_in(i), am_out(i), nullptr}, s);
            if (rc) return rc;
            // block structure (models.py:742-766): the output of layers1 (i == 1) and of each residual
            // block (i == 3, 5, 7) is the next block's input and residual
            if (i == 1 || i == 3 || i == 5 || i == 7) res_idx = out_idx;
            in_idx = out_idx;
            if (i == tap && tap_out) {  // tap 5: input4 = layers3(input3) + residual3 (models.py:750)
                rc = launch_channels_first(o, tap_out + b0 * (int64_t)L.cout * N, N, L.cout, nb, s);
                if (rc) return rc;
            }
        }
        // FC0 reads the last activation as (nb, N*E): l*E + c (its weights are permuted to match); an activation buffer
        // no longer read is room for its split planes (NPD_FC0_PRESPLIT)
        int free_idx = 0;
        while (free_idx == in_idx) ++free_idx;
        const float* fin[3] = {bufs[in_idx], H1, H2};
        float* fout[3] = {H1, H2, H3};
        for (int f = 0; f < 3; ++f) {
            uint16_t* planes = f == 0 ? reinterpret_cast<uint16_t*>(bufs[free_idx]) : nullptr;
            const int rc = launch_layer(c->layers[kLayers + f], {fin[f], fout[f], nullptr, c->img, N, nb, am_in(kLayers + f),
                                                                 am_out(kLayers + f), planes}, s);
            if (rc) return rc;
        }
        if (tap >= kLayers && tap_out) {
            const int64_t fo = c->layers[tap].cout;
            NPD_HIP(hipMemcpyAsync(tap_out + b0 * fo, fout[tap - kLayers], (size_t)nb * fo * 4, hipMemcpyDeviceToDevice, s));
        }
        const int rc = launch_layernorm_sign(H3, c->img + c->off_ln[0], c->img + c->off_ln[1],
                                             logits ? logits + b0 * N : nullptr, decoded ? decoded + b0 * N : nullptr, nb,
                                             N, s);
        if (rc) return rc;
    }
    return NPD_OK;
}

// npd_gru_api.hip -- the RNN decoders' C ABI (include/npd.h): handle create / destroy, decode, decode_count_sweep.
// Argument validation (all of it before the first HIP call) and routing only; the kernels, their images and their
// template dispatch are in the family files behind npd_gru_host.hpp.
#include <string.h>

#include <new>

#include "npd_gru_host.hpp"

using namespace npd;

// the reference's weight count: `gates` F gate rows per cell (GRU 3, LSTM 4), then Linear(F, 1)
static int64_t weight_count(int gates, int N, int F, int layers, int onehot) {
    const int Din = N + (onehot ? 2 : 1);
    int64_t expect = (int64_t)gates * F * Din + (int64_t)gates * F * F + 2 * gates * F;
    if (layers == 2) expect += (int64_t)2 * gates * F * F + 2 * gates * F;
    return expect + F + 1;
}

static hipError_t upload(float** dst, const std::vector<float>& src) {
    if (src.empty()) return hipSuccess;
    hipError_t e = hipMalloc(dst, src.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice);
    return e;
}

// the handle `proto` with its images on the device; on failure nothing stays allocated and *out stays NULL
static int finish_handle(const npd_gru& proto, const gru::HostImages& im, const char* who, npd_gru** out) {
    npd_gru* g = new (std::nothrow) npd_gru(proto);
    if (!g) return fail(NPD_ENOMEM, std::string(who) + ": out of memory");
    g->img_floats = (int64_t)im.img.size();
    hipError_t e = hipGetDevice(&g->device);
    if (e == hipSuccess) e = upload(&g->img, im.img);
    if (e == hipSuccess) e = upload(&g->wy, im.wy);
    if (e == hipSuccess) e = upload(&g->img16, im.img16);
    if (e == hipSuccess) e = upload(&g->wy16, im.wy16);
    if (e != hipSuccess) {
        npd_gru_destroy(g);
        return hip_fail(e, who);
    }
    *out = g;
    return NPD_OK;
}

extern "C" int npd_gru_destroy(npd_gru* g) {
    if (!g) return NPD_OK;
    for (float* p : {g->img, g->wy, g->img16, g->wy16, g->hd})
        if (p) (void)hipFree(p);
    delete g;
    return NPD_OK;
}

extern "C" int npd_rnn_create(int cell, int N, int F, int layers, int onehot, const float* weights, int64_t n_weights,
                              int precision, npd_gru** out) {
    NPD_ARG(out != nullptr, "npd_rnn_create: out is NULL");
    *out = nullptr;
    NPD_ARG(cell == 0 || cell == 1, "npd_rnn_create: cell must be 0 (GRU) or 1 (LSTM)");
    if (cell == 0) return npd_gru_create(N, F, layers, onehot, weights, n_weights, precision, out);
    NPD_ARG(weights != nullptr, "npd_rnn_create: weights is NULL");
    NPD_ARG(N >= 8 && N <= kMaxN && N % 8 == 0, "npd_rnn_create: N must be a multiple of 8 in [8, 256]");
    NPD_ARG(layers == 1 || layers == 2, "npd_rnn_create: 1 or 2 layers supported");
    NPD_ARG(F == 32 || F == 64 || F == 128 || F == 256 || F == 512,
            "npd_rnn_create: LSTM hidden size F must be 32, 64, 128, 256 or 512");
    NPD_ARG(F <= 64 || gru::wide_lds_bytes(N, F, layers) <= 160 * 1024,
            "npd_rnn_create: an LSTM with F = 512 and 2 layers needs N <= 248 (the 160 KiB of LDS hold both states and "
            "the tile's y)");
    NPD_ARG(precision == 0, "npd_rnn_create: LSTM cells run fp32 (precision 0)");
    NPD_ARG(n_weights == weight_count(4, N, F, layers, onehot),
            "npd_rnn_create: weight count does not match (LSTM, N, F, layers, onehot)");
    npd_gru h{};
    h.N = N; h.F = F; h.layers = layers; h.onehot = onehot; h.cell = 1;
    gru::HostImages im;
    gru::build_image_lstm(F, layers, weights, N, onehot, im.img, im.wy, h.b_lin);
    return finish_handle(h, im, "npd_rnn_create", out);
}

static int attach_head(npd_gru* g, int F, int head_depth, int head_hidden, const float* head_weights, int64_t n_head) {
    const int H = head_hidden;
    int64_t expect = (int64_t)H * F + H + (int64_t)(head_depth - 2) * (H * H + H) + H + 1;
    NPD_ARG(n_head == expect, "npd_rnn_create_ex: head weight count does not match (F, head_depth, head_hidden)");
    const int hdt = H <= 32 ? 1 : H <= 64 ? 2 : 4;
    std::vector<float> img;
    float bout = 0.0f;
    gru::build_head_image(head_weights, F, H, head_depth, hdt, img, bout);
    const hipError_t e = upload(&g->hd, img);
    if (e != hipSuccess) return hip_fail(e, "npd_rnn_create_ex (head)");
    g->hd_depth = head_depth; g->hd_tiles = hdt; g->hd_bout = bout;
    return NPD_OK;
}

extern "C" int npd_rnn_create_ex(int cell, int N, int F, int layers, int onehot, const float* weights,
                                 int64_t n_weights, int precision, const float* ln_weight, const float* ln_bias,
                                 float ln_eps, int head_depth, int head_hidden, const float* head_weights,
                                 int64_t n_head, npd_gru** out) {
    NPD_ARG(out != nullptr, "npd_rnn_create_ex: out is NULL");
    *out = nullptr;
    NPD_ARG(head_depth == 1 || (head_depth >= 2 && head_depth <= 8), "npd_rnn_create_ex: head_depth must be 1 .. 8");
    if (head_depth > 1) {
        NPD_ARG(head_weights != nullptr && weights != nullptr, "npd_rnn_create_ex: null pointer");
        NPD_ARG(ln_weight == nullptr, "npd_rnn_create_ex: a LayerNorm before an out_linear_depth > 1 head is not fused");
        NPD_ARG(cell == 0 && precision == 0 && (F == 32 || F == 64) && head_hidden >= 1 && head_hidden <= 128,
                "npd_rnn_create_ex: the out_linear_depth > 1 head runs on the fp32 GRU kernel (cell 0, precision 0, "
                "F 32 or 64, head_hidden 1 .. 128)");
        int rc = npd_gru_create(N, F, layers, onehot, weights, n_weights, 0, out);
        if (rc != NPD_OK) return rc;
        rc = attach_head(*out, F, head_depth, head_hidden, head_weights, n_head);
        if (rc != NPD_OK) {
            npd_gru_destroy(*out);
            *out = nullptr;
        }
        return rc;
    }
    if (ln_weight == nullptr) return npd_rnn_create(cell, N, F, layers, onehot, weights, n_weights, precision, out);
    NPD_ARG(weights != nullptr && ln_bias != nullptr, "npd_rnn_create_ex: null pointer");
    NPD_ARG(cell == 0 && precision == 0 && (F == 32 || F == 64),
            "npd_rnn_create_ex: the LayerNorm head runs on the fp32 GRU kernel (cell 0, precision 0, F 32 or 64)");
    NPD_ARG(n_weights > F, "npd_rnn_create_ex: weight count too small");
    // fold the LayerNorm's affine part into the output Linear: w' = w gamma, b' = b + sum w beta (in order, fp32)
    std::vector<float> w(weights, weights + n_weights);
    float* wl = w.data() + n_weights - F - 1;
    float bsum = w[n_weights - 1];
    for (int i = 0; i < F; ++i) {
        bsum += wl[i] * ln_bias[i];
        wl[i] *= ln_weight[i];
    }
    w[n_weights - 1] = bsum;
    const int rc = npd_gru_create(N, F, layers, onehot, w.data(), n_weights, 0, out);
    if (rc != NPD_OK) return rc;
    (*out)->ln = 1; (*out)->ln_eps = ln_eps;
    return NPD_OK;
}

extern "C" int npd_gru_create(int N, int F, int layers, int onehot, const float* weights, int64_t n_weights,
                              int precision, npd_gru** out) {
    NPD_ARG(out != nullptr, "npd_gru_create: out is NULL");
    *out = nullptr;
    NPD_ARG(weights != nullptr, "npd_gru_create: weights is NULL");
    NPD_ARG(N >= 8 && N <= kMaxN && N % 8 == 0, "npd_gru_create: N must be a multiple of 8 in [8, 256]");
    NPD_ARG(F == 32 || F == 64 || F == 128 || F == 256 || F == 512,
            "npd_gru_create: hidden size F must be 32, 64, 128, 256 or 512");
    NPD_ARG(F <= 64 || precision == 0, "npd_gru_create: the bf16 kernels cover F <= 64; F > 64 runs fp32");
    NPD_ARG(F <= 64 || gru::wide_lds_bytes(N, F, layers) <= 160 * 1024,
            "npd_gru_create: F = 512 with 2 layers needs N <= 248 (the 160 KiB of LDS hold both states and the tile's "
            "y)");
    NPD_ARG(layers == 1 || layers == 2, "npd_gru_create: 1 or 2 GRU layers supported");
    NPD_ARG(precision >= 0 && precision <= 3,
            "npd_gru_create: precision must be 0 (fp32), 1 (bf16x3), 2 (bf16) or 3 (fp16x3)");
    NPD_ARG(precision == 0 || N % 16 == 0, "npd_gru_create: bf16 paths need N % 16 == 0");
    NPD_ARG(n_weights == weight_count(3, N, F, layers, onehot),
            "npd_gru_create: weight count does not match (N, F, layers, onehot)");
    npd_gru h{};
    h.N = N; h.F = F; h.layers = layers; h.onehot = onehot; h.precision = precision;
    gru::HostImages im;
    if (precision == 0) {
        // gru_decode_kernel takes its gate rows folded with their exp2 constants, gru_wide_kernel plain
        gru::build_image(F, layers, weights, N, onehot, F <= 64, im.img, im.wy, h.b_lin);
    } else {
        gru::build_image_split(h, weights, im);
        gru::build_image_split16(h, weights, im);
    }
    return finish_handle(h, im, "npd_gru_create", out);
}

// the kernels' arguments from the handle and the call's operands
static gru::Args make_args(const npd_gru* g, const float* y, const float* h0, const uint8_t* is_info, int reverse,
                           const float* gt, float* decoded, float* logits, int64_t B) {
    gru::Args a{};
    a.img = g->img;
    a.wy = reinterpret_cast<const gru::f4*>(g->wy);
    a.y = y; a.h0 = h0; a.gt = gt; a.decoded = decoded; a.logits = logits; a.B = B;
    a.N = g->N; a.rev = reverse ? 1 : 0; a.onehot = g->onehot; a.b_lin = g->b_lin;
    a.ln = g->ln; a.ln_eps = g->ln_eps;
    a.hd = reinterpret_cast<const gru::f4*>(g->hd);
    a.hd_depth = g->hd_depth; a.hd_bout = g->hd_bout;
    gru::info_mask(is_info, g->N, a.info);
    return a;
}

extern "C" int npd_gru_decode_ex(const npd_gru* g, const float* y, const float* h0, const uint8_t* is_info, int reverse,
                                 const float* gt, float* decoded, float* logits, int64_t B, void* stream) {
    NPD_ARG(g != nullptr, "npd_gru_decode: gru is NULL");
    NPD_ARG(B >= 0, "npd_gru_decode: B < 0");
    if (B == 0) return NPD_OK;
    NPD_ARG(decoded != nullptr && is_info != nullptr, "npd_gru_decode: null pointer");
    NPD_ARG(y != nullptr || h0 != nullptr, "npd_gru_decode: y and h0 both NULL");
    NPD_ARG(((uintptr_t)y & 15) == 0, "npd_gru_decode: y must be 16-byte aligned");
    NPD_ARG(h0 == nullptr || g->precision == 0 || g->img16 != nullptr,
            "npd_gru_decode: an initial state (y_h0) needs precision 0 (fp32) or the 16-codeword split kernel "
            "(F = 64, 2 layers, N % 32 == 0)");
    NPD_ARG(y != nullptr || g->precision == 0 || g->img16 != nullptr,
            "npd_gru_decode: y = NULL (y_h0) needs precision 0 (fp32) or the 16-codeword split kernel");
    NPD_ARG(g->cell == 0 || ((y != nullptr) != (h0 != nullptr) && g->precision == 0),
            "npd_gru_decode: LSTM cells decode y_input (y, no initial state) or y_h0 (initial state, no y), fp32");
    const gru::Args a = make_args(g, y, h0, is_info, reverse, gt, decoded, logits, B);
    hipStream_t s = (hipStream_t)stream;
    // LSTM: F = 32 (1-2 layers) and F = 64 x 1 keep their weights in LDS (lstm_decode_kernel); else lstm_wide_kernel
    if (g->cell == 1) return g->F * g->layers <= 64 ? gru::launch_lstm(g, a, s) : gru::launch_lstm_wide(g, a, s);
    if (g->precision != 0) return gru::launch_split(g, a, s);
    return g->F > 64 ? gru::launch_wide(g, a, s) : gru::launch_f32(g, a, s);
}

extern "C" int npd_gru_decode_count_sweep(const npd_gru* g, int n_seg, const float* y, const uint8_t* is_info,
                                          int reverse, const float* msg, int K, const int32_t* cols, float* decoded,
                                          int64_t B, unsigned long long* counters, void* stream) {
    NPD_ARG(g != nullptr, "npd_gru_decode_count_sweep: gru is NULL");
    NPD_ARG(B >= 0 && n_seg >= 0 && K >= 0, "npd_gru_decode_count_sweep: negative size");
    if (B == 0 || n_seg == 0) return NPD_OK;
    NPD_ARG(y != nullptr && is_info != nullptr && counters != nullptr && (K == 0 || (msg != nullptr && cols != nullptr)),
            "npd_gru_decode_count_sweep: null pointer");
    NPD_ARG(((uintptr_t)y & 15) == 0, "npd_gru_decode_count_sweep: y must be 16-byte aligned");
    NPD_ARG(K <= g->N, "npd_gru_decode_count_sweep: K > N");
    // slot: the message column a position is compared with; cmp: the mask of the compared positions (as Args::info)
    uint8_t slot[kMaxN] = {};
    uint32_t cmp[kMaxWords] = {};
    for (int k = 0; k < K; ++k) {
        NPD_ARG(cols[k] >= 0 && cols[k] < g->N, "npd_gru_decode_count_sweep: column out of range");
        NPD_ARG(!((cmp[cols[k] >> 5] >> (cols[k] & 31)) & 1u), "npd_gru_decode_count_sweep: repeated column");
        cmp[cols[k] >> 5] |= 1u << (cols[k] & 31);
        slot[cols[k]] = (uint8_t)k;
    }
    if (g->img16 == nullptr || g->cell != 0) {
        // other kernels: one decode and one column count per segment (the same counts), into the caller's decoded
        NPD_ARG(decoded != nullptr, "npd_gru_decode_count_sweep: handles other than the 16-codeword split kernel (F = 64, "
                                    "2 layers, N % 32 == 0, precision != 0) need decoded (n_seg, B, N)");
        const int64_t rows = B * g->N;
        for (int sg = 0; sg < n_seg; ++sg) {
            int rc = npd_gru_decode_ex(g, y + sg * rows, nullptr, is_info, reverse, nullptr, decoded + sg * rows, nullptr,
                                       B, stream);
            if (rc == NPD_OK && K > 0)
                rc = npd_count_errors_cols(msg, decoded + sg * rows, B, K, g->N, cols, counters + 2 * sg, stream);
            if (rc != NPD_OK) return rc;
        }
        return NPD_OK;
    }
    const gru::Args a = make_args(g, y, nullptr, is_info, reverse, nullptr, decoded, nullptr, B);
    return gru::launch_split16_sweep(g, a, n_seg, msg, K, slot, cmp, counters, (hipStream_t)stream);
}

extern "C" int npd_gru_decode(const npd_gru* g, const float* y, const uint8_t* is_info, int reverse, const float* gt,
                              float* decoded, float* logits, int64_t B, void* stream) {
    if (B > 0 && y == nullptr) return fail(NPD_EINVAL, "npd_gru_decode: null pointer");
    return npd_gru_decode_ex(g, y, nullptr, is_info, reverse, gt, decoded, logits, B, stream);
}

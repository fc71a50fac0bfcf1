// npd_sc.hip -- SC decoding (PolarCode.sc_decode_new, polar.py:361-484; PAC.pac_sc_decode, pac_code.py:233-345,
// 534-573): the C ABI, the choice of kernel family and the Polar streaming kernels.  The kernel template is
// npd_sc.hpp; the other instantiation units are npd_sc_pac.hip and npd_sc_gen.hip; the fast Polar kernel is
// npd_sc_fast.hip.
#include "npd_sc.hpp"
#include "npd_sc_fast.hpp"

namespace npd {
namespace sc {

static int run(const npd_code* code, const Args& a, hipStream_t s) {
    if (a.B == 0) return NPD_OK;
    const bool full = (a.flags & (kLeaf | kGt | kUhat)) != 0;
    if (code->p.pac) return pac_run(code->p, a, s);
    return full ? dispatch<false, true>(code->p, a, s) : dispatch<false, false>(code->p, a, s);
}

}  // namespace sc
}  // namespace npd

using namespace npd;

extern "C" int npd_sc_decode(const npd_code* code, const float* y, float llr_scale, float* leaf_llr, float* msg_hat,
                             float* u_hat, const float* gt, int64_t B, void* stream) {
    NPD_ARG(code != nullptr, "npd_sc_decode: code is NULL");
    NPD_ARG(B >= 0, "npd_sc_decode: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_sc_decode: y is NULL");
    NPD_ARG(code->p.pac || u_hat == nullptr, "npd_sc_decode: u_hat is only produced for PAC codes");
    NPD_ARG((((uintptr_t)y) & 15) == 0, "npd_sc_decode: y must be 16-byte aligned");
    sc::Args a{};
    a.y = y;
    a.leaf = leaf_llr;
    a.msg = msg_hat;
    a.uhat = u_hat;
    a.gt = gt;
    a.B = B;
    a.scale = llr_scale;
    a.flags = (leaf_llr ? sc::kLeaf : 0u) | (msg_hat ? sc::kMsg : 0u) | (u_hat ? sc::kUhat : 0u) | (gt ? sc::kGt : 0u);
    if (!leaf_llr && !u_hat && !gt && B > 0 && !env_flag("NPD_SC_GENERIC") && sc_fast_eligible(code->p, y))
        return sc_fast_run(code->p, y, &llr_scale, 1, msg_hat, nullptr, 0, 0, B, (hipStream_t)stream);
    return sc::run(code, a, (hipStream_t)stream);
}

extern "C" int npd_sc_decode_mc(const npd_code* code, const float* y, float llr_scale, float* msg_hat, uint64_t seed,
                                uint64_t cw_offset, int64_t B, unsigned long long* counters, void* stream) {
    NPD_ARG(code != nullptr, "npd_sc_decode_mc: code is NULL");
    NPD_ARG(B >= 0, "npd_sc_decode_mc: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_sc_decode_mc: y is NULL");
    NPD_ARG(counters != nullptr, "npd_sc_decode_mc: counters is NULL");
    NPD_ARG((((uintptr_t)y) & 15) == 0, "npd_sc_decode_mc: y must be 16-byte aligned");
    sc::Args a{};
    a.y = y;
    a.msg = msg_hat;
    a.counters = counters;
    a.seed = seed;
    a.cw_offset = cw_offset;
    a.B = B;
    a.scale = llr_scale;
    a.flags = sc::kCount | (msg_hat ? sc::kMsg : 0u);
    if (B > 0 && !env_flag("NPD_SC_GENERIC") && sc_fast_eligible(code->p, y))
        return sc_fast_run(code->p, y, &llr_scale, 1, msg_hat, counters, seed, cw_offset, B, (hipStream_t)stream);
    return sc::run(code, a, (hipStream_t)stream);
}

extern "C" int npd_sc_decode_mc_sweep(const npd_code* code, int n_snr, const float* y, const float* llr_scale,
                                      float* msg_hat, uint64_t seed, uint64_t cw_offset, int64_t B,
                                      unsigned long long* counters, void* stream) {
    NPD_ARG(code != nullptr, "npd_sc_decode_mc_sweep: code is NULL");
    NPD_ARG(n_snr >= 1 && n_snr <= 16, "npd_sc_decode_mc_sweep: 1 <= n_snr <= 16");
    NPD_ARG(llr_scale != nullptr, "npd_sc_decode_mc_sweep: llr_scale is NULL");
    NPD_ARG(B >= 0, "npd_sc_decode_mc_sweep: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_sc_decode_mc_sweep: y is NULL");
    NPD_ARG(counters != nullptr, "npd_sc_decode_mc_sweep: counters is NULL");
    if (B == 0) return NPD_OK;
    if (!env_flag("NPD_SC_GENERIC") && sc_fast_eligible(code->p, y))
        return sc_fast_run(code->p, y, llr_scale, n_snr, msg_hat, counters, seed, cw_offset, B, (hipStream_t)stream);
    const int N = code->p.N, K = code->p.K;
    for (int i = 0; i < n_snr; ++i) {
        const int rc = npd_sc_decode_mc(code, y + (int64_t)i * B * N, llr_scale[i],
                                        msg_hat ? msg_hat + (int64_t)i * B * K : nullptr, seed, cw_offset, B,
                                        counters + 2 * i, stream);
        if (rc) return rc;
    }
    return NPD_OK;
}

extern "C" int npd_sc_mc_sweep_fused(const npd_code* code, int n_snr, const float* sigma, const float* llr_scale,
                                     uint32_t snr_index0, uint64_t seed, uint64_t cw_offset, int64_t B, float* msg_hat,
                                     unsigned long long* counters, void* stream) {
    NPD_ARG(code != nullptr, "npd_sc_mc_sweep_fused: code is NULL");
    NPD_ARG(n_snr >= 1 && n_snr <= 16, "npd_sc_mc_sweep_fused: 1 <= n_snr <= 16");
    NPD_ARG(sigma != nullptr && llr_scale != nullptr, "npd_sc_mc_sweep_fused: sigma / llr_scale is NULL");
    NPD_ARG(B >= 0, "npd_sc_mc_sweep_fused: B < 0");
    NPD_ARG(counters != nullptr || msg_hat != nullptr, "npd_sc_mc_sweep_fused: no output");
    if (B == 0) return NPD_OK;
    const CodeParams& p = code->p;
    if (!p.pac && p.N >= 8 && p.N <= 64 && p.K <= 128 && !env_flag("NPD_SC_GENERIC"))
        return npd::sc_fast_run_gen(p, sigma, llr_scale, n_snr, snr_index0, msg_hat, counters, seed, cw_offset, B,
                                    (hipStream_t)stream);
    // every code the fast kernel does not take (PAC, Polar N >= 128, N = 4): generation in registers, SC decode,
    // counts (and msg_hat) per SNR segment, one launch
    sc::Args a{};
    a.msg = msg_hat;
    a.counters = counters;
    a.seed = seed;
    a.cw_offset = cw_offset;
    a.B = B;
    a.n_seg = n_snr;
    a.snr_index0 = snr_index0;
    for (int i = 0; i < n_snr; ++i) {
        a.seg_scale[i] = llr_scale[i];
        a.seg_sigma[i] = sigma[i];
    }
    a.flags = (counters ? sc::kCount : 0u) | (msg_hat ? sc::kMsg : 0u);
    return sc::gen_run(p, a, (hipStream_t)stream);
}

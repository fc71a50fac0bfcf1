// npd_scl.hip -- SC-List decoding: the Polar instantiations of the kernels in npd_scl.hpp (PolarCode.scl_decode,
// polar.py:793-876, use_CRC=False) and the C ABI.  PAC code handles go to npd_scl_pac.hip's instantiations.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

static int run(const npd_code* code, Args& a, hipStream_t s) {
    const CodeParams& p = code->p;
    if (p.N < 8 || p.N > 256) return fail(NPD_ENOTSUP, "scl_decode: N must be 8..256");
    if (a.L < 1 || a.L > 32) return fail(NPD_EINVAL, "scl_decode: list size must be 1..32");
    if ((((uintptr_t)a.y) & 15) != 0) return fail(NPD_EINVAL, "scl_decode: y must be 16-byte aligned");
    if (a.B == 0) return NPD_OK;
    if (a.L > 8) return p.pac ? run_pac_wide(p, a, s) : run_wide(p, a, s);
    if (p.pac) return run_pac(p, a, s);
    return dispatch<false>(p, a, s);
}

}  // namespace scl
}  // namespace npd

using namespace npd;

extern "C" int npd_scl_decode(const npd_code* code, const float* y, float llr_scale, int list_size, float* msg_hat,
                              float* u_hat, int64_t B, void* stream) {
    NPD_ARG(code != nullptr, "npd_scl_decode: code is NULL");
    NPD_ARG(B >= 0, "npd_scl_decode: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_scl_decode: y is NULL");
    scl::Args a{};
    a.y = y;
    a.msg = msg_hat;
    a.uhat = u_hat;
    a.B = B;
    a.scale = llr_scale;
    a.L = list_size;
    return scl::run(code, a, (hipStream_t)stream);
}

extern "C" int npd_scl_decode_mc(const npd_code* code, const float* y, float llr_scale, int list_size,
                                 float* msg_hat, uint64_t seed, uint64_t cw_offset, int64_t B,
                                 unsigned long long* counters, void* stream) {
    NPD_ARG(code != nullptr, "npd_scl_decode_mc: code is NULL");
    NPD_ARG(B >= 0, "npd_scl_decode_mc: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_scl_decode_mc: y is NULL");
    NPD_ARG(counters != nullptr, "npd_scl_decode_mc: counters is NULL");
    scl::Args a{};
    a.y = y;
    a.msg = msg_hat;
    a.counters = counters;
    a.seed = seed;
    a.cw_offset = cw_offset;
    a.B = B;
    a.scale = llr_scale;
    a.L = list_size;
    a.count = 1u;
    return scl::run(code, a, (hipStream_t)stream);
}

extern "C" int npd_list_prune_select(const float* neg_metrics, int n, int keep, uint32_t* mask_out) {
    NPD_ARG(neg_metrics != nullptr && mask_out != nullptr, "npd_list_prune_select: NULL pointer");
    NPD_ARG(n >= 1 && n <= 16 && keep >= 1 && keep <= n, "npd_list_prune_select: need 1 <= keep <= n <= 16");
    *mask_out = nth::prune_mask(neg_metrics, n, keep);
    return NPD_OK;
}

extern "C" int npd_list_prune_select64(const float* neg_metrics, int n, int keep, uint64_t* mask_out) {
    NPD_ARG(neg_metrics != nullptr && mask_out != nullptr, "npd_list_prune_select64: NULL pointer");
    NPD_ARG(n >= 1 && n <= 64 && keep >= 1 && keep <= n, "npd_list_prune_select64: need 1 <= keep <= n <= 64");
    *mask_out = nth::prune_mask64(neg_metrics, n, keep);
    return NPD_OK;
}

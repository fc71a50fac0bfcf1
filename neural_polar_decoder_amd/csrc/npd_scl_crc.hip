// npd_scl_crc.hip -- CRC-aided SC-List decoding (PolarCode.scl_decode(..., use_CRC=True), polar.py:849-866, with the
// CRC defined in include/npd.h): the Polar, CRC instantiations of the kernels in npd_scl.hpp for 1 .. 8 paths and the
// C ABI.  PAC handles and lists of 9 .. 32 paths go to npd_scl_crc_pac.hip / npd_scl_crc_wide.hip /
// npd_scl_crc_pac_wide.hip.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

static int run_crc(const npd_code* code, Args& a, uint32_t crc_poly, hipStream_t s) {
    const CodeParams& p = code->p;
    a.crc_c = crc_degree(crc_poly, p.K);
    if (a.crc_c < 0) return fail(NPD_EINVAL, "scl_decode_crc: crc_poly needs degree 1 .. 24 below K and bit 0 set");
    a.crc_poly = crc_poly;
    if (p.N < 8 || p.N > 256) return fail(NPD_ENOTSUP, "scl_decode_crc: N must be 8..256");
    if (a.L < 1 || a.L > 32) return fail(NPD_EINVAL, "scl_decode_crc: list size must be 1..32");
    if ((((uintptr_t)a.y) & 15) != 0) return fail(NPD_EINVAL, "scl_decode_crc: y must be 16-byte aligned");
    if (a.B == 0) return NPD_OK;
    if (a.L > 8) return p.pac ? run_crc_pac_wide(p, a, s) : run_crc_wide(p, a, s);
    if (p.pac) return run_crc_pac(p, a, s);
    return dispatch<false, true>(p, a, s);
}

}  // namespace scl
}  // namespace npd

using namespace npd;

extern "C" int npd_scl_decode_crc(const npd_code* code, const float* y, float llr_scale, int list_size,
                                  uint32_t crc_poly, float* msg_hat, float* u_hat, int32_t* crc_ok, int64_t B,
                                  void* stream) {
    NPD_ARG(code != nullptr, "npd_scl_decode_crc: code is NULL");
    NPD_ARG(B >= 0, "npd_scl_decode_crc: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_scl_decode_crc: y is NULL");
    NPD_ARG(B == 0 || msg_hat != nullptr || u_hat != nullptr || crc_ok != nullptr, "npd_scl_decode_crc: no output given");
    scl::Args a{};
    a.y = y;
    a.msg = msg_hat;
    a.uhat = u_hat;
    a.crc_ok = crc_ok;
    a.B = B;
    a.scale = llr_scale;
    a.L = list_size;
    return scl::run_crc(code, a, crc_poly, (hipStream_t)stream);
}

extern "C" int npd_scl_decode_crc_mc(const npd_code* code, const float* y, float llr_scale, int list_size,
                                     uint32_t crc_poly, float* msg_hat, uint64_t seed, uint64_t cw_offset, int64_t B,
                                     unsigned long long* counters, void* stream) {
    NPD_ARG(code != nullptr, "npd_scl_decode_crc_mc: code is NULL");
    NPD_ARG(B >= 0, "npd_scl_decode_crc_mc: B < 0");
    NPD_ARG(B == 0 || y != nullptr, "npd_scl_decode_crc_mc: y is NULL");
    NPD_ARG(counters != nullptr, "npd_scl_decode_crc_mc: counters is NULL");
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
    return scl::run_crc(code, a, crc_poly, (hipStream_t)stream);
}

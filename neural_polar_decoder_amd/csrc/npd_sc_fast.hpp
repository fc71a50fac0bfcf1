// npd_sc_fast.hpp -- entry points of the fast Polar SC kernel (npd_sc_fast.hip), called from the C ABI in npd_sc.hip
#pragma once
#include "npd_common.hpp"

namespace npd {

// eligible: Polar, 8 <= N <= 64, K <= 128 (one Philox block of message bits), y 16-B aligned
bool sc_fast_eligible(const CodeParams& p, const void* y);
int sc_fast_run(const CodeParams& p, const float* y, const float* llr_scale, int n_seg, float* msg,
                unsigned long long* counters, uint64_t seed, uint64_t cw_offset, int64_t B, hipStream_t s);
// fused Monte-Carlo sweep: same eligibility as the decode path minus the y pointer
int sc_fast_run_gen(const CodeParams& p, const float* sigma, const float* llr_scale, int n_seg, uint32_t snr_index0,
                    float* msg, unsigned long long* counters, uint64_t seed, uint64_t cw_offset, int64_t B,
                    hipStream_t s);

}  // namespace npd

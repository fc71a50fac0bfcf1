// Occupancy of the LDS-resident SC-List kernels (N = 128 / 256), Polar and PAC, as the launcher queries it:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -Iinclude -Ineural_polar_decoder_amd/csrc \
//         tools/scl_occupancy.hip -o tools/bin/scl_occupancy && tools/bin/scl_occupancy
// Prints, per kernel, the dynamic LDS bytes of one 64-lane block and the blocks (= waves) that fit one CU.
#include <cstdio>

#include "npd_scl.hpp"

using namespace npd;
using namespace npd::scl;

template <int N, int G, bool PAC>
static int report() {
    const size_t lds = (size_t)LdsRows<N>::kRows * kWave * sizeof(float);
    auto kern = scl_lds_kernel<N, G, PAC>;
    if (lds > 65536 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 163840) != hipSuccess) {
        printf("scl_lds_kernel<%d,%d,%s>: hipFuncSetAttribute failed\n", N, G, PAC ? "pac" : "polar");
        return 1;
    }
    int occ = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 64, lds);
    printf("scl_lds_kernel<%d,%d,%s>: rows %d, LDS %zu B per wave, %d waves per CU (%s)\n", N, G, PAC ? "pac" : "polar",
           LdsRows<N>::kRows, lds, occ, hipGetErrorString(e));
    return e != hipSuccess;
}

template <int N>
static int report_n() {
    return report<N, 1, false>() + report<N, 1, true>() + report<N, 2, false>() + report<N, 2, true>() +
           report<N, 4, false>() + report<N, 4, true>() + report<N, 8, false>() + report<N, 8, true>();
}

int main() { return report_n<128>() + report_n<256>(); }

// npd_launch.hpp -- the launch helper the kernel families with dynamic LDS images share (GRU, conv).
#pragma once

#include "npd_common.hpp"

namespace npd {

// one launch of a kernel with a dynamic LDS image; its LDS limit is raised on first use, once per instantiation
template <auto Kern, typename... A>
int launch_lds(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... a) {
    static bool attr = false;
    if (!attr) {
        NPD_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
        attr = true;
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, s, a...);
    return launch_check(what);
}

}  // namespace npd

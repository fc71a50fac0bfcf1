// npd_sc_pac.hip -- the PAC streaming kernels of npd_sc.hpp, with both root modes of the compile-time PAC(128,64) RM
// frozen set.
#include "npd_sc.hpp"

namespace npd {
namespace sc {

static int root_mode() {  // NPD_SC_ROOT=0/1: root-level mode of the msg-only PAC(128,64) RM kernel (A/B); per call
    const char* e = getenv("NPD_SC_ROOT");
    return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : kRootModeDefault;
}

int pac_run(const CodeParams& p, const Args& a, hipStream_t s) {
    const bool full = (a.flags & (kLeaf | kGt | kUhat)) != 0;
    if (!full && !env_flag("NPD_SC_NOSPEC") && is_pac_rm128(p))
        switch (root_mode()) {
            case 1: return launch_t<128, 64, true, false, SpecPacRm128R<1>, false>(p, a, s);
            default: return launch_t<128, 64, true, false, SpecPacRm128, false>(p, a, s);
        }
    return full ? dispatch<true, true>(p, a, s) : dispatch<true, false>(p, a, s);
}

}  // namespace sc
}  // namespace npd

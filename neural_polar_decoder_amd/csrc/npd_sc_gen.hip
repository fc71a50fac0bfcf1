// npd_sc_gen.hip -- the fused Monte-Carlo (GEN) kernels of npd_sc.hpp, Polar and PAC: received words generated in
// registers, decoded and counted per SNR segment in one launch (npd_sc_mc_sweep_fused).
#include "npd_sc.hpp"

namespace npd {
namespace sc {

int gen_run(const CodeParams& p, const Args& a, hipStream_t s) {
    if (!env_flag("NPD_SC_NOSPEC") && is_pac_rm128(p)) return launch_t<128, 64, true, false, SpecPacRm128, true>(p, a, s);
    return p.pac ? dispatch<true, false, true>(p, a, s) : dispatch<false, false, true>(p, a, s);
}

}  // namespace sc
}  // namespace npd

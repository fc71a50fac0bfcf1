// npd_scl_pac_wide.hip -- SC-List decoding with 9 .. 32 paths, PAC codes: the G = 16 and G = 32 instantiations of
// scl_lds_kernel (npd_scl.hpp) with pac_sc_decode's leaf step at N = 8 .. 256, in a file of their own.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

int run_pac_wide(const CodeParams& p, const Args& a, hipStream_t s) { return dispatch_wide<true>(p, a, s); }

}  // namespace scl
}  // namespace npd

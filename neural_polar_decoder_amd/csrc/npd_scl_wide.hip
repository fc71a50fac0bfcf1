// npd_scl_wide.hip -- SC-List decoding with 9 .. 32 paths, Polar codes: the G = 16 and G = 32 instantiations of
// scl_lds_kernel (npd_scl.hpp) at N = 8 .. 256, in a file of their own so that they compile beside the L <= 8 ones.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

int run_wide(const CodeParams& p, const Args& a, hipStream_t s) { return dispatch_wide<false>(p, a, s); }

}  // namespace scl
}  // namespace npd

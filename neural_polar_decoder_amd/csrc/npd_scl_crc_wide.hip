// npd_scl_crc_wide.hip -- CRC-aided SC-List decoding with 9 .. 32 paths, Polar codes: the G = 16 and G = 32, CRC
// instantiations of scl_lds_kernel (npd_scl.hpp) at N = 8 .. 256.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

int run_crc_wide(const CodeParams& p, const Args& a, hipStream_t s) { return dispatch_wide<false, true>(p, a, s); }

}  // namespace scl
}  // namespace npd

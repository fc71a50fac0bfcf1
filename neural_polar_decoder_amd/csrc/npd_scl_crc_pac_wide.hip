// npd_scl_crc_pac_wide.hip -- CRC-aided SC-List decoding with 9 .. 32 paths, PAC codes: the G = 16 and G = 32, PAC,
// CRC instantiations of scl_lds_kernel (npd_scl.hpp) at N = 8 .. 256.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

int run_crc_pac_wide(const CodeParams& p, const Args& a, hipStream_t s) { return dispatch_wide<true, true>(p, a, s); }

}  // namespace scl
}  // namespace npd

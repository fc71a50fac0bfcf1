// npd_scl_crc_pac.hip -- CRC-aided SC-List decoding of PAC codes with 1 .. 8 paths: the PAC, CRC instantiations of the
// kernels in npd_scl.hpp, in a file of their own so that the sets of unrolled trees compile side by side.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

int run_crc_pac(const CodeParams& p, const Args& a, hipStream_t s) { return dispatch<true, true>(p, a, s); }

}  // namespace scl
}  // namespace npd

// npd_scl_pac.hip -- SC-List decoding of PAC codes: the PAC instantiations of the kernels in npd_scl.hpp (the
// list decoder of polar.py:793-876 with pac_sc_decode's leaf step, pac_code.py:534-573), in a file of their own
// so that the two sets of unrolled trees compile side by side.
#include "npd_scl.hpp"

namespace npd {
namespace scl {

int run_pac(const CodeParams& p, const Args& a, hipStream_t s) { return dispatch<true>(p, a, s); }

}  // namespace scl
}  // namespace npd

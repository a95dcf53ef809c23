// fa2_mfma16d_f16.hip -- the f16 instantiations of the LDS-DMA forward kernel (fa2_mfma16d_kernel.h), a translation unit of their
// own for the build time alone; fa2_mfma16d.hip hands f16 problems to launch_f16.
#include "fa2_mfma16d_kernel.h"

namespace fa2_mfma16d {

template <int F> int launch_f16(const Fa2Problem &p, const DmaArgs &a, int waves) { return launch_d<_Float16, F>(p, a, waves); }

template int launch_f16<0>(const Fa2Problem &, const DmaArgs &, int);
template int launch_f16<kWindow>(const Fa2Problem &, const DmaArgs &, int);
template int launch_f16<kWindow | kVarlen>(const Fa2Problem &, const DmaArgs &, int);
template int launch_f16<kWindow | kGqa>(const Fa2Problem &, const DmaArgs &, int);
template int launch_f16<kWindow | kVarlen | kGqa>(const Fa2Problem &, const DmaArgs &, int);

}  // namespace fa2_mfma16d

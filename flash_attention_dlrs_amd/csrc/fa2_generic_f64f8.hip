// fa2_generic_f64f8.hip -- the f64 and fp8 instantiations of the catch-all FA-2 forward kernel (fa2_generic_kernel.h), a
// translation unit of their own for the build time alone; fa2_generic.hip hands every dtype it does not compile to launch_f64_f8.
#include "fa2_generic_kernel.h"

namespace fa2_generic {

template <int F> int launch_f64_f8(const Fa2Problem &p, const GenericArgs &a) {
    if (p.dtype == FA2_DTYPE_F64) return launch_e<ElemF64, F>(p, a);
    if constexpr (!(F & kVarlen)) {  // (fp8 has no varlen form: no backward, and e4m3fn cannot hold L = +inf)
        if (p.dtype == FA2_DTYPE_F8E5M2) return launch_e<ElemF8E5M2, F>(p, a);
        if (p.dtype == FA2_DTYPE_F8E4M3) return launch_e<ElemF8E4M3, F>(p, a);
    }
    fa2_set_error("unknown dtype enum %d", p.dtype);
    return FA2_ERR_UNSUPPORTED;
}

template int launch_f64_f8<0>(const Fa2Problem &, const GenericArgs &);
template int launch_f64_f8<kWindow>(const Fa2Problem &, const GenericArgs &);
template int launch_f64_f8<kWindow | kVarlen>(const Fa2Problem &, const GenericArgs &);
template int launch_f64_f8<kWindow | kGqa>(const Fa2Problem &, const GenericArgs &);
template int launch_f64_f8<kWindow | kVarlen | kGqa>(const Fa2Problem &, const GenericArgs &);
template int launch_f64_f8<kWindow | kVarlen | kGqa | kDv>(const Fa2Problem &, const GenericArgs &);

}  // namespace fa2_generic

// The fp8-query instantiations of fa2_decode_generic.hip (fa2_fwd_kvcache_mla_q8, FA2_KVCACHE_VARIANT_GENERIC), alone in their translation
// unit -- the other kernels keep their code.
#define FA2_DECODE_Q8 1
#include "fa2_decode_generic.hip"

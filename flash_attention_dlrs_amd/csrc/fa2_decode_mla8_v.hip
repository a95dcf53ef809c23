// Packed-query instantiations of fa2_decode_mla8.hip (fa2_fwd_kvcache_mla_varlen_q8): the query-tiled form of the fp8 matrix kernel over
// the fp8 latent cache, alone in its translation unit -- the fixed-N_q kernels keep their code.
#define FA2_DECODE_VARLEN_Q 1
#include "fa2_decode_mla8.hip"

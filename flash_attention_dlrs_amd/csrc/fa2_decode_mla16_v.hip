// Variable-length-query instantiations of fa2_decode_mla16.hip (fa2_fwd_kvcache_mla_varlen): the query-tiled form over the latent
// cache, alone in its translation unit -- the fixed-N_q kernels keep their code.
#define FA2_DECODE_VARLEN_Q 1
#include "fa2_decode_mla16.hip"

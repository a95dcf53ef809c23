// Variable-length-query instantiations of fa2_decode_mfma16.hip (fa2_fwd_kvcache_varlen): the query-tiled form, alone in its
// translation unit -- the fixed-N_q kernels keep their code.
#define FA2_DECODE_VARLEN_Q 1
#include "fa2_decode_mfma16.hip"

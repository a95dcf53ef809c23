// List-addressed instantiations of fa2_decode_mla16.hip (fa2_fwd_kvcache_mla_sparse): per-query key lists over the latent cache,
// alone in their translation unit -- the dense kernels keep their code and their argument struct.
#define FA2_DECODE_SPARSE 1
#include "fa2_decode_mla16.hip"

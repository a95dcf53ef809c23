// List-addressed instantiations of fa2_decode_mla16.hip over packed queries (fa2_fwd_kvcache_mla_sparse_varlen): SP and VQ together,
// alone in their translation unit -- the dense, the query-tiled and the fixed list-addressed kernels keep their code.
#define FA2_DECODE_SPARSE 1
#define FA2_DECODE_VARLEN_Q 1
#include "fa2_decode_mla16.hip"

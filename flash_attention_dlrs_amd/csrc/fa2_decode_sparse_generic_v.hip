// Packed instantiations of fa2_decode_sparse_generic.hip (fa2_fwd_kvcache_mla_sparse_varlen, FA2_KVCACHE_VARIANT_GENERIC): the lists
// of packed queries on the VALU, alone in their translation unit -- the fixed kernels keep their code.
#define FA2_DECODE_SPARSE_VARLEN 1
#include "fa2_decode_sparse_generic.hip"

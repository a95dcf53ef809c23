// Packed instantiations of fa2_indexer_topk_split.hip (fa2_topk_indices_varlen_split), alone in their translation unit -- the fixed
// kernels keep their code.
#define FA2_INDEXER_VARLEN 1
#include "fa2_indexer_topk_split.hip"

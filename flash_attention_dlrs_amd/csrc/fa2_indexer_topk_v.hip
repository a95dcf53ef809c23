// Packed instantiations of fa2_indexer_topk.hip (the _varlen entry points of the MLA indexer), alone in their translation unit -- the
// fixed kernels keep their code.
#define FA2_INDEXER_VARLEN 1
#include "fa2_indexer_topk.hip"

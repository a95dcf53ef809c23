// Packed instantiations of fa2_indexer_mfma8.hip (the _varlen_q8 entry points of the MLA indexer), alone in their translation unit.
#define FA2_INDEXER_VARLEN 1
#include "fa2_indexer_mfma8.hip"

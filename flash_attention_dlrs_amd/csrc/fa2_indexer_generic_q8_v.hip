// The packed fp8-query instantiations of fa2_indexer_generic.hip (the _varlen_q8 entry points), alone in their translation unit.
#define FA2_INDEXER_VARLEN 1
#include "fa2_indexer_generic_q8.hip"

// The fp8-query instantiations of fa2_indexer_generic.hip (the _q8 entry points of the MLA indexer), alone in their translation unit --
// the 16-bit and f32 kernels keep their code.
#define FA2_INDEXER_Q8 1
#include "fa2_indexer_generic.hip"

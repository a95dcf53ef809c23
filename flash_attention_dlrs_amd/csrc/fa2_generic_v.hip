// Variable-length (packed) instantiations of fa2_generic.hip: the windowed form with per-sequence extents and the bottom-right
// shifted band, alone in its translation unit -- the plain and windowed kernels keep their code.
#define FA2_GENERIC_WINDOW 1
#define FA2_GENERIC_VARLEN 1
#include "fa2_generic.hip"

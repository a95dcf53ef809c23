// Variable-length (packed) instantiations of fa2_mfma16d.hip: the windowed form with per-sequence extents and the bottom-right
// shifted band, alone in its translation unit -- the plain and windowed kernels keep their code.
#define FA2_MFMA16D_WINDOW 1
#define FA2_MFMA16D_VARLEN 1
#include "fa2_mfma16d.hip"

// Local-attention (windowed) instantiations of fa2_mfma16d.hip, alone in their translation unit: the plain kernels there keep
// the code they had before the window existed.
#define FA2_MFMA16D_WINDOW 1
#include "fa2_mfma16d.hip"

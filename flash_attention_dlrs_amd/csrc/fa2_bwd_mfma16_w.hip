// Local-attention (windowed) instantiations of fa2_bwd_mfma16.hip, alone in their translation unit: the plain kernels there
// keep the code they had before the window existed.
#define FA2_BWD_MFMA16_WINDOW 1
#include "fa2_bwd_mfma16.hip"

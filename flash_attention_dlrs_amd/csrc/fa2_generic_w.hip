// Local-attention (windowed) instantiations of fa2_generic.hip, alone in their translation unit: the plain kernels there keep
// the code they had before the window existed.
#define FA2_GENERIC_WINDOW 1
#include "fa2_generic.hip"

// Grouped-query (GQA) instantiations of the windowed fa2_bwd_mfma16.hip, alone in their translation unit (fa2_bwd_api.hip: a dense
// GQA problem without a window runs here as the full band, whose arithmetic is the plain kernel's).
#define FA2_BWD_MFMA16_WINDOW 1
#define FA2_BWD_MFMA16_GQA 1
#include "fa2_bwd_mfma16.hip"

// Grouped-query (GQA) instantiations of the windowed fa2_bwd_generic.hip, alone in their translation unit (fa2_bwd_api.hip: a dense
// GQA problem without a window runs here as the full band).
#define FA2_BWD_GENERIC_WINDOW 1
#define FA2_BWD_GENERIC_GQA 1
#include "fa2_bwd_generic.hip"

// Grouped-query (GQA) instantiations of the windowed fa2_generic.hip, alone in their translation unit: query head h reads KV head
// h / gqa.  Non-mergeable dense layouts run here (fa2_api.hip: fwd_gqa); a plain or causal problem as the full band.
#define FA2_GENERIC_WINDOW 1
#define FA2_GENERIC_GQA 1
#include "fa2_generic.hip"

// Grouped-query (GQA) instantiations of the windowed fa2_mfma16d.hip, alone in their translation unit: query head hh reads KV
// head hh / group.  Non-mergeable dense layouts run here (fa2_api.hip: fwd_gqa); a plain or causal problem as the full band.
#define FA2_MFMA16D_WINDOW 1
#define FA2_MFMA16D_GQA 1
#include "fa2_mfma16d.hip"

// Grouped-query (GQA) instantiations of the varlen fa2_bwd_mfma16.hip, alone in their translation unit.
#define FA2_BWD_MFMA16_WINDOW 1
#define FA2_BWD_MFMA16_VARLEN 1
#define FA2_BWD_MFMA16_GQA 1
#include "fa2_bwd_mfma16.hip"

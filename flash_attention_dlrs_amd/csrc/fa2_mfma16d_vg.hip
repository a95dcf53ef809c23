// Grouped-query (GQA) instantiations of the varlen fa2_mfma16d.hip, alone in their translation unit: query head hh reads KV
// head hh / group.
#define FA2_MFMA16D_WINDOW 1
#define FA2_MFMA16D_VARLEN 1
#define FA2_MFMA16D_GQA 1
#include "fa2_mfma16d.hip"

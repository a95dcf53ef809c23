// Grouped-query (GQA) instantiations of the varlen fa2_bwd_generic.hip, alone in their translation unit.
#define FA2_BWD_GENERIC_WINDOW 1
#define FA2_BWD_GENERIC_VARLEN 1
#define FA2_BWD_GENERIC_GQA 1
#include "fa2_bwd_generic.hip"

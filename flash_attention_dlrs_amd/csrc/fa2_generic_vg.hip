// Grouped-query (GQA) instantiations of the varlen fa2_generic.hip, alone in their translation unit: query head h reads KV head
// h / gqa.
#define FA2_GENERIC_WINDOW 1
#define FA2_GENERIC_VARLEN 1
#define FA2_GENERIC_GQA 1
#include "fa2_generic.hip"

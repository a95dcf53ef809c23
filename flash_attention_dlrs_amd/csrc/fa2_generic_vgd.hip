// The varlen GQA instantiations of fa2_generic.hip with a value head size of its own (fa2_fwd_varlen_dv), alone in their
// translation unit: V and O have d_v columns, the scores run over d.
#define FA2_GENERIC_WINDOW 1
#define FA2_GENERIC_VARLEN 1
#define FA2_GENERIC_GQA 1
#define FA2_GENERIC_DV 1
#include "fa2_generic.hip"

// The varlen GQA instantiations of fa2_bwd_generic.hip with a value head size of its own (fa2_bwd_varlen_dv), alone in their
// translation unit: V, O, dO and dV have d_v columns, Q, K, dQ and dK have d.
#define FA2_BWD_GENERIC_WINDOW 1
#define FA2_BWD_GENERIC_VARLEN 1
#define FA2_BWD_GENERIC_GQA 1
#define FA2_BWD_GENERIC_DV 1
#include "fa2_bwd_generic.hip"

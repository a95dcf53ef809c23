// Dense instantiations of fa2_decode_mla16.hip over the tile-scaled fp8 latent cache (fa2_fwd_kvcache_mla_ds): the cache type CacheDS
// without key lists, uniform row addressing, alone in their translation unit -- every other unit keeps its code and its argument struct.
#define FA2_DECODE_DS 1
#include "fa2_decode_mla16.hip"

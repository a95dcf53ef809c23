// Dense, query-tiled instantiations of fa2_decode_mla16.hip over the tile-scaled fp8 latent cache and packed queries
// (fa2_fwd_kvcache_mla_varlen_ds): VQ with the cache type CacheDS, alone in their translation unit.
#define FA2_DECODE_VARLEN_Q 1
#define FA2_DECODE_DS 1
#include "fa2_decode_mla16.hip"

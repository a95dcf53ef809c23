"""MI355X-native Flash-Attention-2 forward behind the Python surface of 17ex/flash_attention_dlrs.

Modules mirror the reference's (src/flash_attention_torch.py, src/flash_attention_wrappers.py); the
Triton launch they make is replaced by the C-ABI call fa2_fwd() of libfa2_hip.so (include/fa2_fwd.h),
a hand-written HIP/CDNA4 kernel library.  There is no CPU fallback: without the built library, or on
non-GPU tensors, calls fail loudly.
"""
from .flash_attention_torch import (MIN_TENSOR_SIZE, FlashAttention, FlashAttentionDeterministic, FlashAttentionMLAPrefill,
                                    FlashAttentionVarlen, convert_triton_dtype, gqa_kv_heads, varlen_mask)
from .flash_attention_wrappers import (apply_rotary, dequantize_kv_cache, flash_attention_backward, flash_attention_forward,
                                       flash_attention_kvcache_forward, flash_attention_mla_decode_forward,
                                       flash_attention_varlen_backward, check_mla_append_args, mla_kvcache_append,
                                       mla_kvcache_append_varlen, check_mla_varlen_args, check_mla_sparse_args,
                                       flash_attention_mla_sparse_decode_forward,
                                       flash_attention_mla_varlen_decode_forward, flash_attention_mla_prefill_backward,
                                       flash_attention_mla_prefill_forward,
                                       flash_attention_varlen_forward, flash_attention_varlen_kvcache_forward, kvcache_append,
                                       kvcache_append_varlen, quantize_kv_cache, check_mla_indexer_args,
                                       flash_attention_mla_indexer_topk, mla_indexer_logits, quantize_index_keys, topk_indices,
                                       check_mla_sparse_varlen_args, flash_attention_mla_sparse_varlen_decode_forward,
                                       check_mla_indexer_varlen_args, mla_indexer_logits_varlen, topk_indices_varlen,
                                       flash_attention_mla_indexer_topk_varlen)

__all__ = ["FlashAttention", "FlashAttentionDeterministic", "FlashAttentionVarlen", "convert_triton_dtype", "MIN_TENSOR_SIZE",
           "flash_attention_forward", "flash_attention_backward", "flash_attention_varlen_forward",
           "flash_attention_varlen_backward", "flash_attention_kvcache_forward", "quantize_kv_cache", "dequantize_kv_cache",
           "varlen_mask", "gqa_kv_heads", "kvcache_append", "apply_rotary", "flash_attention_varlen_kvcache_forward",
           "kvcache_append_varlen", "flash_attention_mla_decode_forward", "mla_kvcache_append", "mla_kvcache_append_varlen",
           "check_mla_append_args", "flash_attention_mla_varlen_decode_forward", "check_mla_varlen_args",
           "flash_attention_mla_prefill_forward", "flash_attention_mla_prefill_backward", "FlashAttentionMLAPrefill",
           "flash_attention_mla_sparse_decode_forward", "check_mla_sparse_args", "flash_attention_mla_indexer_topk",
           "mla_indexer_logits", "topk_indices", "check_mla_indexer_args", "quantize_index_keys",
           "flash_attention_mla_sparse_varlen_decode_forward", "check_mla_sparse_varlen_args", "mla_indexer_logits_varlen",
           "topk_indices_varlen", "flash_attention_mla_indexer_topk_varlen", "check_mla_indexer_varlen_args"]

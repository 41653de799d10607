#pragma once
#include "common.hpp"

// calli.hip: PerceiverAttention's softmax(q k^T) v of T tiles (8 heads x 3 queries x 259 keys x 64 dims, scale 0.125): q / out [T * 3][512] bf16,
// kv [T * 259][1024] bf16 (K in columns 0..511, V in 512..1023).  which = 0: perceiver_attn_kernel, 1: round 1's perceiver_attn_v1_kernel (the same bits).
// The resampler (resample_chunk) and the test entry cr_op_perceiver_attention (api.hip) both launch through this function.
int launch_perceiver_attn(int which, const bf16* q, const bf16* kv, bf16* out, int T, hipStream_t stream);

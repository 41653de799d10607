// The weight map cr_ctx::w and what is derived from it (weights.hip).  Nothing else writes the map: a tensor, loaded or derived, gets in through w_put
// and out through w_drop*, which keeps a copy from outliving the tensor it was made from and the resolved table below from going stale.
#pragma once
#include "ctx.hpp"

// A derived COPY of the tensor `name` is filed in the same map under "<the kind's prefix><name>"
enum CopyKind {
    COPY_DECLAYOUT,     // "declayout.": bf16 in the decode layout (llm_finalize; all or nothing over the LLM's linears)
    COPY_FP8,           // "fp8.": e4m3 bytes, row by row ...
    COPY_FP8_SCALE,     // "fp8s.": ... and the fp32 scale of each row (build_fp8_copy makes the pair)
    COPY_FP8_BOUND,     // "fp8b.": {max row norm of W, max |bias|} of a ViT fc1 (cr_enable_fp8_mfma); the one kind that also depends on a second tensor, fc1's bias
    COPY_FP8_DECLAYOUT, // "fp8dl.": the e4m3 bytes in their decode layout (cr_enable_fp8_decode; all or nothing)
    COPY_KINDS
};

// the tensor `name` / its copy of kind k, or null (no error is set)
const DevTensor* w_find(const cr_ctx* c, const std::string& name);
const DevTensor* w_copy(const cr_ctx* c, CopyKind k, const std::string& name);
// The tensor `name` with room for `bytes`: an entry of that size keeps its allocation (the caller overwrites its contents), any other is freed and replaced.
// Null when the device has no room.
DevTensor* w_put(cr_ctx* c, const std::string& name, int dtype, std::vector<int64_t> shape, size_t bytes);
bool w_drop(cr_ctx* c, const std::string& name);      // whether there was one
// Every copy made from `name` goes (the tensor was reloaded or rebuilt).  True when an e4m3 kind was among them: fp8_decode and fp8_mfma are then off until
// cr_enable_fp8_* rebuilds what is missing.
bool w_drop_copies(cr_ctx* c, const std::string& name);
size_t w_drop_kind(cr_ctx* c, CopyKind k);            // every copy of one kind; the bytes freed

// One linear layer's weight [N][K] in the forms the GEMM kernels take (device pointers); all but `w` may be null
struct LinW {
    const bf16* w;                // bf16 as loaded (nn.Linear's layout; w1|w3: the interleaved derived tensor)
    int N, K;
    const bf16* dl;               // its decode-layout copy (llm_finalize)
    int dl_kind;                  // GemmParams::wsw of that copy: 1 plain tiles, 2 wqkv's RoPE tile order (only the K-sliced kernel reads it)
    const unsigned char* q8; const float* s8;      // e4m3 copy + one fp32 scale per row (cr_enable_fp8_mfma / cr_enable_fp8_decode)
    const unsigned char* dl8;     // the e4m3 copy in its decode layout (cr_enable_fp8_decode)
    bool e4m3() const { return q8 && s8; }
};
struct LayerW { const bf16 *an, *fn; LinW qkv, o, w13, w2; };
// The language model's weights, resolved: which copies EXIST (whether a launch takes one is the stage's decision: fp8_decode, fp8_mfma, the row count).
// Every write to the map drops it and the next llm_weights call rebuilds it, so it never points at a freed or replaced tensor.
struct LlmWeights {
    int ff;
    const bf16 *embed, *cosT, *sinT, *norm;      // tok_embeddings [vocab][4096], rope.cos / rope.sin [max_pos][128], the final RMSNorm
    LinW head;
    std::vector<LayerW> layer;
};
int llm_weights(cr_ctx* c, const LlmWeights** out);      // CR_ERR_STATE, the message naming the first missing tensor, without a whole language model
const bf16* llm_embed_table(cr_ctx* c);                  // all that cr_embed_splice needs (a context may hold it without the layers)

// e4m3 copy + scales of weight `name` (COPY_FP8 / COPY_FP8_SCALE); a no-op when already built for this shape
int build_fp8_copy(cr_ctx* c, const std::string& name, int k_multiple, hipStream_t st);
// bf16 rows [rows][K] (row stride ldw) -> e4m3 bytes [rows][K] + one scale per row (common.hpp's e4m3 row rule); K % 8 == 0
void launch_quant_fp8_rows(const bf16* w, int64_t ldw, int rows, int K, unsigned char* q, float* scale, hipStream_t st);

// cr_finalize: derive re-laid-out tensors once the checkpoint tensors are in (each stage's own in its file, the language model's in weights.hip).
#include "weights.hpp"

int vit_finalize(cr_ctx* c, hipStream_t st);
int calli_finalize(cr_ctx* c, hipStream_t st);
int llm_finalize(cr_ctx* c, hipStream_t st);

extern "C" int cr_finalize(cr_ctx* c, void* stream) {
    if (!c) return cr_fail(CR_ERR_ARG, "cr_finalize: null context");
    if (c->borrowed) return cr_fail(CR_ERR_STATE, "cr_finalize: this context borrows its weights (cr_share_weights); finalize the owner");
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (w_find(c, "vision_model.embeddings.patch_embedding.weight")) CR_TRY(vit_finalize(c, st));
    if (w_find(c, "normed_emb.weight")) CR_TRY(calli_finalize(c, st));
    // (w1 / w3 are released once interleaved: a context finalized before still has its language model -- a reloaded wqkv / wo / w2 / LM head
    //  needs its decode-layout copy rebuilt just the same)
    if (w_find(c, "language_model.model.layers.0.feed_forward.w1.weight") || w_find(c, "derived.w13.0")) CR_TRY(llm_finalize(c, st));
    CR_HIP(hipStreamSynchronize(st));
    c->finalized = true;
    cr_bump_gen(c);
    return CR_OK;
}

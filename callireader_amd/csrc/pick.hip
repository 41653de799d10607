// What follows the LM head in a prefill and in a decode step (pick.hpp: HeadBufs, pick_rows): the greedy pick kernel, and the order in which the constraint
// masks, the pick (greedy or sampled), the token scores and the beam step run over the call's logits rows.  pick_rows builds seqstate.hpp's views once -- the
// call's rows and the cache's per-sequence state -- and every launch behind it takes those two.
#include "constrain.hpp"
#include "kv.hpp"
#include "logprobs.hpp"

namespace {

// RepetitionPenaltyLogitsProcessor (published 4.45.2 semantics) + argmax (first max wins) + append the id (+ its stop check).
// One workgroup of 1024 per row.  The steps are pick.hpp's and SeqState::append, shared with the sampling pick (sample.hip).
__global__ __launch_bounds__(1024) void pick_kernel(Rows r, SeqState s, int len_add) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int seq = r.seq(row);
    if (s.beam_row(seq)) return;                              // a beam row: beam.hip picks for it
    float* lg = r.row(row);
    const int ng = s.ngen[seq];
    if (r.penalty != 1.0f && ng > 0) apply_penalty(lg, s.hist(seq), ng, r.penalty, tid, r.orig_row(row));
    argmax_row(lg, r.vocab, tid, bv, bi);
    if (tid == 0) s.append(seq, bi[0], ng, len_add);
}

}  // namespace

void HeadBufs::carve(Arena& ar) {
    hl = ar.take<bf16>((size_t)n * D);
    lg = ar.take<float>((size_t)n * V);
    score = f.scored ? ar.take<char>(logprobs_scratch_bytes(n, V)) : nullptr;
    lg0 = f.deep ? ar.take<float>((size_t)n * V) : nullptr;
    cand = f.beam_rows ? ar.take<char>(beam_scratch_bytes(n)) : nullptr;
}

BeamLaunch beam_launch(cr_kv* kv, const HeadBufs& h, int len_add, int first_only) {
    return {kv->d_beam, len_add, (float*)h.cand, (int32_t*)(h.cand + (size_t)h.n * 2 * BEAM_MAX * 4), kv->d_bfin, first_only};
}

BeamCache beam_cache(const cr_kv* kv) { return {kv->k, kv->v, (int64_t)kv->n_seqs * NKV * kv->max_tokens * HD, kv->layers, kv->max_tokens}; }

int pick_rows(cr_kv* kv, const HeadBufs& h, const int32_t* d_seqs, float penalty, int len_add, float* out, hipStream_t st, bool prefill) {
    const int n = h.n, V = h.V;
    const Rows r = h.rows(d_seqs, penalty);
    SeqState s = kv_seq_state(kv);
    if (!h.f.beam_rows) s.bgrp = nullptr;                            // beam rows are skipped by the picks and taken by the beam step below
    if (out) CR_HIP(hipMemcpyAsync(out, h.lg, (size_t)n * V * 4, hipMemcpyDeviceToDevice, st));
    if (h.f.constrained) CR_TRY(launch_constrain(r, s, {kv->d_con, (int64_t)kv->con_stride, 1}, st));
    if (h.lg0) CR_HIP(hipMemcpyAsync(h.lg0, h.lg, (size_t)n * V * 4, hipMemcpyDeviceToDevice, st));
    if (h.f.beam_rows == n) {}                                       // nothing but beams: no pick at all
    else if (h.f.sampled) CR_TRY(launch_sample(r, s, {nullptr, 1, len_add, nullptr, nullptr}, st));
    else hipLaunchKernelGGL(pick_kernel, dim3(n), dim3(1024), 0, st, r, s, len_add);
    if (h.f.scored) CR_TRY(launch_logprobs(r, s, {0, h.score, kv->d_lp, kv->d_top_id, kv->d_top_lp}, st));
    if (h.f.beam_rows) CR_TRY(launch_beam_step(r, s, beam_launch(kv, h, len_add, prefill ? 1 : 0), st));
    return CR_OK;
}

// What follows the LM head in a prefill and in a decode step (pick.hpp: HeadBufs, pick_rows): the greedy pick kernel, and the order in which the constraint
// masks, the pick (greedy or sampled), the token scores and the beam step run over the call's logits rows.
#include "constrain.hpp"
#include "kv.hpp"
#include "logprobs.hpp"

namespace {

// RepetitionPenaltyLogitsProcessor (published 4.45.2 semantics) + argmax (first max wins) + append the id (+ its stop check).
// One workgroup of 1024 per row.  The three steps are pick.hpp's, shared with the sampling pick (sample.hip).
__global__ __launch_bounds__(1024) void pick_kernel(float* __restrict__ logits, int64_t ld, int vocab, float penalty,
                                                    int seq0, const int32_t* __restrict__ seqs, int64_t* __restrict__ gen,
                                                    int32_t* __restrict__ ngen, int32_t* __restrict__ lens, int gen_cap, int len_add,
                                                    int32_t* __restrict__ stop, int n_seqs, const float* __restrict__ orig,
                                                    const int32_t* __restrict__ bgrp) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int seq = seqs ? seqs[row] : seq0;
    if (bgrp && bgrp[seq] >= 0) return;                       // a beam row: beam.hip picks for it
    float* lg = logits + (int64_t)row * ld;
    const int ng = ngen[seq];
    int64_t* g = gen + (int64_t)seq * gen_cap;
    if (penalty != 1.0f && ng > 0) apply_penalty(lg, g, ng, penalty, tid, orig ? orig + (int64_t)row * ld : nullptr);
    argmax_row(lg, vocab, tid, bv, bi);
    if (tid == 0) {
        if (ng < gen_cap) {
            g[ng] = bi[0]; ngen[seq] = ng + 1;
            stop_check(stop, n_seqs, seq, bi[0], ng + 1);
        }
        lens[seq] += len_add;
    }
}

}  // namespace

void HeadBufs::carve(Arena& ar) {
    hl = ar.take<bf16>((size_t)n * D);
    lg = ar.take<float>((size_t)n * V);
    score = f.scored ? ar.take<char>(logprobs_scratch_bytes(n, V)) : nullptr;
    lg0 = f.deep ? ar.take<float>((size_t)n * V) : nullptr;
    cand = f.beam_rows ? ar.take<char>(beam_scratch_bytes(n)) : nullptr;
}

BeamLaunch beam_launch(cr_kv* kv, const HeadBufs& h, const int32_t* d_seqs, float penalty, int len_add, int first_only) {
    BeamLaunch p{};
    p.logits = h.lg; p.ld = h.V; p.vocab = h.V; p.penalty = penalty; p.rows = h.n; p.seqs = d_seqs; p.grp = kv->d_bgrp; p.state = kv->d_beam;
    p.gen = kv->d_gen; p.ngen = kv->d_ngen; p.gen_cap = kv->gen_cap; p.lens = kv->d_len; p.len_add = len_add; p.orig = h.lg0;
    p.cand_v = (float*)h.cand; p.cand_i = (int32_t*)(h.cand + (size_t)h.n * 2 * BEAM_MAX * 4); p.fin_ids = kv->d_bfin; p.stop = kv->d_stop; p.n_seqs = kv->n_seqs;
    p.first_only = first_only;
    return p;
}

BeamCache beam_cache(const cr_kv* kv) { return {kv->k, kv->v, (int64_t)kv->n_seqs * NKV * kv->max_tokens * HD, kv->layers, kv->max_tokens}; }

int pick_rows(cr_kv* kv, const HeadBufs& h, const int32_t* d_seqs, float penalty, int len_add, float* out, hipStream_t st, bool prefill) {
    const int n = h.n, V = h.V;
    const Hist hist = kv_hist(kv, d_seqs);
    if (out) CR_HIP(hipMemcpyAsync(out, h.lg, (size_t)n * V * 4, hipMemcpyDeviceToDevice, st));
    if (h.f.constrained) {
        ConstrainLaunch p{h.lg, V, V, n, hist, {kv->d_con_on, kv->d_con, (int64_t)kv->con_stride, 1}};
        CR_TRY(launch_constrain(p, st));
    }
    if (h.lg0) CR_HIP(hipMemcpyAsync(h.lg0, h.lg, (size_t)n * V * 4, hipMemcpyDeviceToDevice, st));
    const int32_t* bgrp = h.f.beam_rows ? kv->d_bgrp : nullptr;      // beam rows are skipped by the picks and taken by the beam step below
    if (h.f.beam_rows == n) {}                                       // nothing but beams: no pick at all
    else if (h.f.sampled) {
        SampleLaunch p{};
        p.logits = h.lg; p.ld = V; p.vocab = V; p.penalty = penalty; p.rows = n; p.h = hist;
        p.temp = kv->d_temp; p.topk = kv->d_topk; p.topp = kv->d_topp; p.seed = kv->d_seed;
        p.append = 1; p.lens = kv->d_len; p.len_add = len_add; p.stop = kv->d_stop; p.n_seqs = kv->n_seqs; p.orig = h.lg0; p.bgrp = bgrp;
        CR_TRY(launch_sample(p, st));
    } else
        hipLaunchKernelGGL(pick_kernel, dim3(n), dim3(1024), 0, st, h.lg, (int64_t)V, V, penalty, 0, d_seqs, kv->d_gen, kv->d_ngen,
                           kv->d_len, kv->gen_cap, len_add, kv->d_stop, kv->n_seqs, h.lg0, bgrp);
    if (h.f.scored) {
        LogprobsLaunch p{h.lg, V, V, n, hist, kv->d_lpn, 0, kv->d_lpdone, h.score, kv->d_lp, kv->d_top_id, kv->d_top_lp};
        CR_TRY(launch_logprobs(p, st));
    }
    if (h.f.beam_rows) CR_TRY(launch_beam_step(beam_launch(kv, h, d_seqs, penalty, len_add, prefill ? 1 : 0), st));
    return CR_OK;
}

// Teacher-forced scores (cr_llm_score_batch): the log-probability of a GIVEN id in every scored row of a prefill-shaped pass, and the row's top-n.
//
//   row j of a sequence's scored rows predicts its target y_j; h_j = {y_0 .. y_{j-1}}, the targets of the sequence's scored rows before it in the call
//   z        = the raw fp32 LM-head row after the repetition penalty over h_j (pick.hpp's arithmetic: v < 0 ? v * p : v / p; an id repeated in h_j is penalised
//              once: every duplicate sees the original score)
//   logprob  = z[y_j] - lse(z);  top-n = the n largest entries of z, logprobs.hip's tie rule
// -- what a greedy generation that happened to produce y_0 .. y_j recorded for y_j (cr_kv_set_logprobs).
//
// Three launches.  score_table_kernel: first[sequence][id] = the ordinal of the first scored row whose target is `id` (integer atomicMin on an INT_MAX-filled
// table), so "id is in h_j" is first[id] < j: one table per sequence serves all of its rows, and nothing is scattered into the logits.  score_chunk_kernel is
// logprobs_chunk_kernel with that test applied in registers as the scores are loaded; score_merge_kernel is logprobs_merge_kernel writing slot j with the
// target's own score penalised the same way.  The chunk and merge bodies are logprobs_dev.hpp's, shared with logprobs.hip: chunks of 4096, 16 scores per
// lane, double accumulation, chunk-order merge, no float atomics -- a row's result is bit-equal to cr_op_logprobs on the host-penalised row, and depends on
// its scores, its history and vocab, not on the tile, the batch or the row index.  penalty == 1 launches no table kernel and reads no table.
#include <limits.h>

#include <vector>

#include "ctx.hpp"
#include "logprobs_dev.hpp"
#include "score.hpp"

namespace {

using namespace lpdev;

__global__ __launch_bounds__(256) void score_table_kernel(const int64_t* __restrict__ tgt, const int32_t* __restrict__ hist, const int32_t* __restrict__ ord,
                                                          int rows, int vocab, int32_t* __restrict__ first) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int64_t y = tgt[r];
    if (y >= 0 && y < vocab) atomicMin(first + (int64_t)hist[r] * vocab + y, ord[r]);
}

// block (chunk, i): row row0 + i of the index block, logits row i
template <bool PEN>
__global__ __launch_bounds__(THREADS) void score_chunk_kernel(ScoreLaunch p, Partials q) {
    const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
    const float* lg = p.logits + (int64_t)row * p.ld;
    float z[PER];
    if (PEN) load_chunk<true>(lg, p.vocab, chunk * CHUNK, tid, z, p.first + (int64_t)p.ix.hist[p.row0 + row] * p.vocab, p.ix.ord[p.row0 + row], p.penalty);
    else load_chunk<false>(lg, p.vocab, chunk * CHUNK, tid, z);
    reduce_chunk(z, p.vocab, chunk * CHUNK, (int64_t)row * q.chunks + chunk, tid, q.pm, q.ps, q.pv, q.pi);
}

__global__ __launch_bounds__(64) void score_merge_kernel(ScoreLaunch p, Partials q) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int64_t slot = (int64_t)p.row0 + row, y = p.ix.tgt[slot];
    float zi = NAN;
    if (y >= 0 && y < p.vocab) {
        zi = p.logits[(int64_t)row * p.ld + y];
        if (p.first && p.first[(int64_t)p.ix.hist[slot] * p.vocab + y] < p.ix.ord[slot]) zi = penalised(zi, p.penalty);
    }
    merge_row(row, q.chunks, p.top_n, slot, zi, lane, q.pm, q.ps, q.pv, q.pi, p.out_lp, p.out_id, p.out_tlp);
}

}  // namespace

int launch_score_table(const ScoreIndex& ix, int rows, int n_hist, int vocab, int32_t* first, hipStream_t st) {
    CR_HIP(hipMemsetD32Async((hipDeviceptr_t)first, INT_MAX, (size_t)n_hist * vocab, st));
    hipLaunchKernelGGL(score_table_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, (const int64_t*)ix.tgt, (const int32_t*)ix.hist, (const int32_t*)ix.ord, rows,
                       vocab, first);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_score_rows(const ScoreLaunch& p, hipStream_t st) {
    const Partials q(p.scratch, p.rows, logprobs_chunks(p.vocab));      // laid out as launch_logprobs lays them out
    hipLaunchKernelGGL(p.first ? score_chunk_kernel<true> : score_chunk_kernel<false>, dim3(q.chunks, p.rows), dim3(THREADS), 0, st, p, q);
    hipLaunchKernelGGL(score_merge_kernel, dim3(p.rows), dim3(64), 0, st, p, q);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

extern "C" int cr_op_score_rows(const float* logits, int n, int vocab, const int64_t* targets_host, const int32_t* row_seq_host, const int32_t* hist_index_host,
                                float penalty, int top_n, float* lp, int32_t* top_ids, float* top_lp, void* stream) {
    if (top_n < 0 || top_n > TOPN) return cr_fail(CR_ERR_ARG, "cr_op_score_rows: top_n %d (want 0..%d)", top_n, TOPN);
    if (!logits || !targets_host || !row_seq_host || !hist_index_host || !lp || (top_n > 0 && (!top_ids || !top_lp)) || n <= 0 || n > 65535 || vocab < TOPN)
        return cr_fail(CR_ERR_ARG, "cr_op_score_rows: bad argument (a null pointer, n outside 1..65535 or vocab < %d)", TOPN);
    if (!(penalty > 0.f) || penalty == INFINITY) return cr_fail(CR_ERR_ARG, "cr_op_score_rows: penalty %g (want a finite value > 0)", penalty);
    int n_hist = 0;
    for (int r = 0; r < n; r++) {
        if (targets_host[r] < 0 || targets_host[r] >= vocab) return cr_fail(CR_ERR_ARG, "cr_op_score_rows: target %lld of row %d outside the vocabulary (%d)", (long long)targets_host[r], r, vocab);
        if (row_seq_host[r] < 0 || row_seq_host[r] >= n || hist_index_host[r] < 0)
            return cr_fail(CR_ERR_ARG, "cr_op_score_rows: row %d names history %d, ordinal %d (want 0..%d, >= 0)", r, row_seq_host[r], hist_index_host[r], n - 1);
        n_hist = row_seq_host[r] + 1 > n_hist ? row_seq_host[r] + 1 : n_hist;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool pen = penalty != 1.0f;
    const size_t sb = (logprobs_scratch_bytes(n, vocab) + 255) & ~(size_t)255, ib = (score_index_words(n) * 8 + 255) & ~(size_t)255;
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, sb + ib + (pen ? (size_t)n_hist * vocab * 4 : 0)) != hipSuccess) return cr_fail(CR_ERR_NOMEM, "cr_op_score_rows: scratch");
    std::vector<int64_t> h(score_index_words(n));
    const ScoreIndex hx = score_index(h.data(), n), dx = score_index((int64_t*)(blk + sb), n);
    for (int r = 0; r < n; r++) { hx.tgt[r] = targets_host[r]; hx.hist[r] = row_seq_host[r]; hx.ord[r] = hist_index_host[r]; }
    int32_t* first = pen ? (int32_t*)(blk + sb + ib) : nullptr;
    int rc = hipMemcpyAsync(dx.tgt, h.data(), h.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess ? CR_OK : cr_fail(CR_ERR_HIP, "cr_op_score_rows: index copy");
    if (rc == CR_OK && pen) rc = launch_score_table(dx, n, n_hist, vocab, first, st);
    if (rc == CR_OK) rc = launch_score_rows(ScoreLaunch{logits, vocab, vocab, n, 0, dx, first, penalty, top_n, blk, lp, top_ids, top_lp}, st);
    hipStreamSynchronize(st);
    hipFree(blk);
    return rc;
}

// Token scores (cr_kv_set_logprobs): the log-probability of the id a pick has just appended and the top-n alternatives of the row it chose from.
//
//   z        = the fp32 score row the pick left in `lg`: the LM-head logits AFTER the repetition penalty and before anything else.  For a greedy row this
//              is transformers' scores[t]; for a sampled row it is the same row, i.e. BEFORE temperature / top-k / top-p (transformers' scores for
//              do_sample=True are the warped ones): a confidence describes the model, not the warper.
//   lse      = m + log(sum_i exp(z_i - m)), m = max_i z_i; -inf entries contribute 0
//   logprob  = z[id] - lse
//   top-n    = the n largest entries of z (1 <= n <= 8), descending, an exact tie broken towards the LOWER id (argmax_row's rule: top_ids[0] of a
//              greedy row is its id), as (id, z - lse)
//   A row holding NaN or +inf gives NaN log-probabilities (ids unspecified).
//
// Two launches.  logprobs_chunk_kernel: a row is split into chunks of CHUNK = 4096 scores -- the chunk count is a function of vocab alone -- one
// workgroup of 256 threads each (23 per row at vocab 92 553: 1472 workgroups at 64 rows, where the pick has 64), every lane holding 16 scores from
// four 16-byte loads.  A chunk produces its online-softmax pair (m, s = sum exp(z - m)) and its own top-8: waves reduce by __shfl_xor, the four waves
// through LDS.  logprobs_merge_kernel: one wave per row merges the chunks IN CHUNK ORDER and writes the sequence's slot t = ngen - 1.
// Element i of a row always lands on the same lane of the same chunk, every partial sum is formed in an order fixed by that placement, and no float
// atomic is used: a row's result depends on its scores and on vocab, not on the row index, the number of rows, the slot or the stream.
// (A row starts at row * vocab floats, 4-byte aligned only when vocab % 4 != 0: the 16-byte loads are declared 4-byte aligned, which gfx950's global
// loads allow, so that the placement does not move with the row's alignment.)
//
// Precision: exp is the accurate expf (<= 1 ulp), the terms are accumulated in double from the first add on, the merge and the logarithm run in double,
// and the results are rounded to fp32 once.  What remains: that rounding (half an ulp of a value below 128: 3.8e-6), the fp32 rounding of z - m
// (weighted by the term's share of the sum: below 5e-7 for |z| <= 32) and expf's ulp (1.2e-7 relative): under 5e-6 absolute in all.
#include "ctx.hpp"
#include "logprobs_dev.hpp"
#include "pick.hpp"

namespace {

using namespace lpdev;

// Partials of one (row, chunk), logprobs_dev.hpp reduce_chunk.  seqs NULL: every row is scored (cr_op_logprobs); else rows whose sequence has scores off exit.
__global__ __launch_bounds__(THREADS) void logprobs_chunk_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int chunks,
                                                                 const int32_t* __restrict__ seqs, const int32_t* __restrict__ lpn,
                                                                 float* __restrict__ pm, double* __restrict__ ps, float* __restrict__ pv,
                                                                 int32_t* __restrict__ pi) {
    const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
    if (seqs && lpn[seqs[row]] <= 0) return;
    float z[PER];
    load_chunk<false>(logits + (int64_t)row * ld, vocab, chunk * CHUNK, tid, z);
    reduce_chunk(z, vocab, chunk * CHUNK, (int64_t)row * chunks + chunk, tid, pm, ps, pv, pi);
}

// One wave per row: lse from the chunk pairs in chunk order, the row's top-n from the chunks' candidates, the picked id's score (logprobs_dev.hpp merge_row).
// Cache rows (seqs given): the slot is t = ngen[seq] - 1, the id gen[seq][t]; a sequence whose history is full appended nothing, so nothing is scored
// (done[seq] counts the slots written).  Op rows (seqs NULL): slot `row`, id ids[row], n = top_n.
__global__ __launch_bounds__(64) void logprobs_merge_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int chunks,
                                                           const int32_t* __restrict__ seqs, const int32_t* __restrict__ lpn, int top_n,
                                                           const int64_t* __restrict__ gen, const int32_t* __restrict__ ngen, int gen_cap,
                                                           int32_t* __restrict__ done, const float* __restrict__ pm, const double* __restrict__ ps,
                                                           const float* __restrict__ pv, const int32_t* __restrict__ pi, float* __restrict__ out_lp,
                                                           int32_t* __restrict__ out_id, float* __restrict__ out_tlp) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int n = top_n;
    int64_t slot = row, id;
    if (seqs) {
        const int seq = seqs[row];
        n = lpn[seq];
        if (n <= 0) return;
        const int t = ngen[seq] - 1;
        if (t < 0 || t != done[seq]) return;                  // nothing was appended by this launch's pick
        id = gen[(int64_t)seq * gen_cap + t];
        slot = (int64_t)seq * gen_cap + t;
        if (lane == 0) done[seq] = t + 1;
    } else {
        id = gen[row];
    }
    const float zi = (id >= 0 && id < vocab) ? logits[(int64_t)row * ld + id] : NAN;
    merge_row(row, chunks, n, slot, zi, lane, pm, ps, pv, pi, out_lp, out_id, out_tlp);
}

// cr_kv_fanout: wave j merges the partials of the ONE row (partial row 0) for sequence dsts.seq[j], as logprobs_merge_kernel does for a cache row
__global__ __launch_bounds__(64) void logprobs_fan_merge_kernel(const float* __restrict__ row, int vocab, int chunks, FanSeqs dsts, const int32_t* __restrict__ lpn,
                                                               const int64_t* __restrict__ gen, const int32_t* __restrict__ ngen, int gen_cap,
                                                               int32_t* __restrict__ done, const float* __restrict__ pm, const double* __restrict__ ps,
                                                               const float* __restrict__ pv, const int32_t* __restrict__ pi, float* __restrict__ out_lp,
                                                               int32_t* __restrict__ out_id, float* __restrict__ out_tlp) {
    const int seq = dsts.seq[blockIdx.x], lane = threadIdx.x;
    const int n = lpn[seq];
    if (n <= 0) return;
    const int t = ngen[seq] - 1;
    if (t < 0 || t != done[seq]) return;
    const int64_t id = gen[(int64_t)seq * gen_cap + t];
    const int64_t slot = (int64_t)seq * gen_cap + t;
    if (lane == 0) done[seq] = t + 1;
    const float zi = (id >= 0 && id < vocab) ? row[id] : NAN;
    merge_row(0, chunks, n, slot, zi, lane, pm, ps, pv, pi, out_lp, out_id, out_tlp);
}

__global__ __launch_bounds__(64) void set_logprobs_kernel(int32_t* __restrict__ lpn, int32_t* __restrict__ done, int seq, int top_n) {
    if (threadIdx.x == 0) { lpn[seq] = top_n; done[seq] = 0; }
}

}  // namespace

int logprobs_chunks(int vocab) { return (vocab + CHUNK - 1) / CHUNK; }

size_t logprobs_scratch_bytes(int rows, int vocab) {
    const size_t rc = (size_t)rows * logprobs_chunks(vocab);
    return 256 + rc * 8 + rc * 4 + rc * TOPN * 8;
}

int launch_logprobs(const LogprobsLaunch& p, hipStream_t st) {
    const int chunks = logprobs_chunks(p.vocab);
    const size_t rc = (size_t)p.rows * chunks;
    double* ps = (double*)(((uintptr_t)p.scratch + 255) & ~(uintptr_t)255);
    float* pm = (float*)(ps + rc);
    float* pv = pm + rc;
    int32_t* pi = (int32_t*)(pv + rc * TOPN);
    hipLaunchKernelGGL(logprobs_chunk_kernel, dim3(chunks, p.rows), dim3(THREADS), 0, st, p.logits, p.ld, p.vocab, chunks, p.h.seqs, p.lpn, pm, ps, pv, pi);
    hipLaunchKernelGGL(logprobs_merge_kernel, dim3(p.rows), dim3(64), 0, st, p.logits, p.ld, p.vocab, chunks, p.h.seqs, p.lpn, p.top_n, (const int64_t*)p.h.gen,
                       (const int32_t*)p.h.ngen, p.h.gen_cap, p.done, (const float*)pm, (const double*)ps, (const float*)pv, (const int32_t*)pi, p.out_lp, p.out_id,
                       p.out_tlp);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_logprobs_fan(const float* row, int vocab, const FanSeqs& dsts, const LogprobsLaunch& p, hipStream_t st) {
    const int chunks = logprobs_chunks(vocab);
    double* ps = (double*)(((uintptr_t)p.scratch + 255) & ~(uintptr_t)255);
    float* pm = (float*)(ps + chunks);
    float* pv = pm + chunks;
    int32_t* pi = (int32_t*)(pv + (size_t)chunks * TOPN);
    hipLaunchKernelGGL(logprobs_chunk_kernel, dim3(chunks, 1), dim3(THREADS), 0, st, row, (int64_t)vocab, vocab, chunks, (const int32_t*)nullptr, p.lpn, pm, ps, pv, pi);
    hipLaunchKernelGGL(logprobs_fan_merge_kernel, dim3(dsts.n), dim3(64), 0, st, row, vocab, chunks, dsts, p.lpn, (const int64_t*)p.h.gen, (const int32_t*)p.h.ngen,
                       p.h.gen_cap, p.done, (const float*)pm, (const double*)ps, (const float*)pv, (const int32_t*)pi, p.out_lp, p.out_id, p.out_tlp);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_set_logprobs(int32_t* lpn, int32_t* done, int seq, int top_n, hipStream_t st) {
    hipLaunchKernelGGL(set_logprobs_kernel, dim3(1), dim3(64), 0, st, lpn, done, seq, top_n);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

extern "C" int cr_op_logprobs(const float* logits, int n, int vocab, const int64_t* ids, int top_n, float* lp, int32_t* top_ids, float* top_lp,
                              void* stream) {
    if (top_n < 1 || top_n > TOPN) return cr_fail(CR_ERR_ARG, "cr_op_logprobs: top_n %d (want 1..%d)", top_n, TOPN);
    if (!logits || !ids || !lp || !top_ids || !top_lp || n <= 0 || n > 65535 || vocab < TOPN)
        return cr_fail(CR_ERR_ARG, "cr_op_logprobs: bad argument (a null pointer, n outside 1..65535 or vocab < %d)", TOPN);
    hipStream_t st = (hipStream_t)stream;
    void* scratch = nullptr;
    if (hipMalloc(&scratch, logprobs_scratch_bytes(n, vocab)) != hipSuccess) return cr_fail(CR_ERR_NOMEM, "cr_op_logprobs: scratch");
    const LogprobsLaunch p{logits, vocab, vocab, n, {nullptr, const_cast<int64_t*>(ids), nullptr, 0}, nullptr, top_n, nullptr, scratch, lp, top_ids, top_lp};
    const int rc = launch_logprobs(p, st);
    hipStreamSynchronize(st);
    hipFree(scratch);
    return rc;
}

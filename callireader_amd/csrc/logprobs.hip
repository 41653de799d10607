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

// Partials of one (row, chunk), logprobs_dev.hpp reduce_chunk.  Op rows (s.lpn NULL): every row is scored; else rows whose sequence has scores off exit.
__global__ __launch_bounds__(THREADS) void logprobs_chunk_kernel(Rows r, SeqState s, Partials q) {
    const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
    if (s.lpn && s.lpn[r.seq(row)] <= 0) return;
    float z[PER];
    load_chunk<false>(r.row(row), r.vocab, chunk * CHUNK, tid, z);
    reduce_chunk(z, r.vocab, chunk * CHUNK, (int64_t)row * q.chunks + chunk, tid, q.pm, q.ps, q.pv, q.pi);
}

// The slot of the id that the pick of this launch has just appended to `seq`, and the id; < 0 when there is none: a sequence whose history is full appended
// nothing, so nothing is scored (lpdone[seq] counts the slots written)
__device__ __forceinline__ int64_t scored_slot(const SeqState& s, int seq, int lane, int64_t& id) {
    const int t = s.ngen[seq] - 1;
    if (t < 0 || t != s.lpdone[seq]) return -1;
    id = s.hist(seq)[t];
    if (lane == 0) s.lpdone[seq] = t + 1;
    return (int64_t)seq * s.gen_cap + t;
}

// One wave per row: lse from the chunk pairs in chunk order, the row's top-n from the chunks' candidates, the picked id's score (logprobs_dev.hpp merge_row).
// Cache rows: the sequence's own count of alternatives and scored_slot.  Op rows (s.lpn NULL): slot `row`, id gen[row], n = top_n.
__global__ __launch_bounds__(64) void logprobs_merge_kernel(Rows r, SeqState s, LogprobsLaunch p, Partials q) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int n = p.top_n;
    int64_t slot = row, id;
    if (s.lpn) {
        const int seq = r.seq(row);
        n = s.lpn[seq];
        if (n <= 0) return;
        slot = scored_slot(s, seq, lane, id);
        if (slot < 0) return;
    } else {
        id = s.gen[row];
    }
    const float zi = (id >= 0 && id < r.vocab) ? r.row(row)[id] : NAN;
    merge_row(row, q.chunks, n, slot, zi, lane, q.pm, q.ps, q.pv, q.pi, p.out_lp, p.out_id, p.out_tlp);
}

// cr_kv_fanout: wave j merges the partials of the ONE row (partial row 0) for sequence dsts.seq[j], as logprobs_merge_kernel does for a cache row
__global__ __launch_bounds__(64) void logprobs_fan_merge_kernel(const float* __restrict__ row, int vocab, FanSeqs dsts, SeqState s, LogprobsLaunch p, Partials q) {
    const int seq = dsts.seq[blockIdx.x], lane = threadIdx.x;
    const int n = s.lpn[seq];
    if (n <= 0) return;
    int64_t id;
    const int64_t slot = scored_slot(s, seq, lane, id);
    if (slot < 0) return;
    const float zi = (id >= 0 && id < vocab) ? row[id] : NAN;
    merge_row(0, q.chunks, n, slot, zi, lane, q.pm, q.ps, q.pv, q.pi, p.out_lp, p.out_id, p.out_tlp);
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

int launch_logprobs(const Rows& r, const SeqState& s, const LogprobsLaunch& p, hipStream_t st) {
    const Partials q(p.scratch, r.n, logprobs_chunks(r.vocab));
    hipLaunchKernelGGL(logprobs_chunk_kernel, dim3(q.chunks, r.n), dim3(THREADS), 0, st, r, s, q);
    hipLaunchKernelGGL(logprobs_merge_kernel, dim3(r.n), dim3(64), 0, st, r, s, p, q);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_logprobs_fan(const float* row, int vocab, const FanSeqs& dsts, const SeqState& s, const LogprobsLaunch& p, hipStream_t st) {
    const Partials q(p.scratch, 1, logprobs_chunks(vocab));
    // the one row as an op row: scored whatever a sequence's switch says
    hipLaunchKernelGGL(logprobs_chunk_kernel, dim3(q.chunks, 1), dim3(THREADS), 0, st, Rows{const_cast<float*>(row), vocab, vocab, 1, nullptr, nullptr, 1.0f}, SeqState{}, q);
    hipLaunchKernelGGL(logprobs_fan_merge_kernel, dim3(dsts.n), dim3(64), 0, st, row, vocab, dsts, s, p, q);
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
    SeqState s{};                                            // op rows: the id of row r is ids[r]
    s.gen = const_cast<int64_t*>(ids); s.gen_cap = 1;
    const int rc = launch_logprobs({const_cast<float*>(logits), vocab, vocab, n, nullptr, nullptr, 1.0f}, s, {top_n, scratch, lp, top_ids, top_lp}, st);
    hipStreamSynchronize(st);
    hipFree(scratch);
    return rc;
}

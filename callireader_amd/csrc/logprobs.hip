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
#include <float.h>

#include "ctx.hpp"
#include "logprobs.hpp"

namespace {

constexpr int CHUNK = 4096, THREADS = 256, PER = CHUNK / THREADS, TOPN = LOGPROBS_MAX_TOP;
static_assert(PER == 16 && TOPN == 8, "logprobs.hip: 16 scores per lane, 8 alternatives");

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// (value, id) order of the alternatives: larger value first, the lower id on an exact tie.  NaN compares false either way.
__device__ __forceinline__ bool before(float v, int i, float v2, int i2) { return v > v2 || (v == v2 && i < i2); }

__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int i2 = __shfl_xor(i, o, 64);
        if (before(v2, i2, v, i)) { v = v2; i = i2; }
    }
}

// Partials of one (row, chunk): pm = chunk maximum, ps = sum of exp(z - pm) over the chunk's entries above -inf (0 for a chunk of -inf), pv / pi = its top-8 in order
// (missing entries: -inf with id INT_MAX, which sort last).  seqs NULL: every row is scored (cr_op_logprobs); else rows whose sequence has scores off exit.
__global__ __launch_bounds__(THREADS) void logprobs_chunk_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int chunks,
                                                                 const int32_t* __restrict__ seqs, const int32_t* __restrict__ lpn,
                                                                 float* __restrict__ pm, double* __restrict__ ps, float* __restrict__ pv,
                                                                 int32_t* __restrict__ pi) {
    __shared__ float sm[4];
    __shared__ double ss[4];
    __shared__ float sv[4];
    __shared__ int si[4];
    const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (seqs && lpn[seqs[row]] <= 0) return;
    const float* lg = logits + (int64_t)row * ld;
    const int base = chunk * CHUNK;
    float z[PER];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i0 = base + (k * THREADS + tid) * 4;
        if (i0 + 3 < vocab) {
            const f32x4u q = *(const f32x4u*)(lg + i0);
            z[4 * k] = q.x; z[4 * k + 1] = q.y; z[4 * k + 2] = q.z; z[4 * k + 3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) z[4 * k + e] = i0 + e < vocab ? lg[i0 + e] : -INFINITY;
        }
    }
    // chunk maximum (a NaN score is skipped here and poisons the sum below)
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < PER; j++) m = z[j] > m ? z[j] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float m2 = __shfl_xor(m, o, 64); m = m2 > m ? m2 : m; }
    if (lane == 0) sm[w] = m;
    __syncthreads();
    m = sm[0];
#pragma unroll
    for (int k = 1; k < 4; k++) m = sm[k] > m ? sm[k] : m;
    // sum of exp(z - m): lane order, then the xor tree, then the four waves in order
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < PER; j++)
        if (z[j] != -INFINITY) s += (double)expf(z[j] - m);    // (ids past the row's end were loaded as -inf)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) ss[w] = s;
    // the chunk's top-8: round r finds the best (value, id) that comes strictly after round r - 1's winner
    float pvv = INFINITY; int pii = -1;
    const int64_t po = ((int64_t)row * chunks + chunk) * TOPN;
    for (int r = 0; r < TOPN; r++) {
        float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int i = base + ((j >> 2) * THREADS + tid) * 4 + (j & 3);
            if (i < vocab && before(pvv, pii, z[j], i) && before(z[j], i, bv, bi)) { bv = z[j]; bi = i; }
        }
        wave_best(bv, bi);
        __syncthreads();                                      // round r - 1's readers are done with sv / si
        if (lane == 0) { sv[w] = bv; si[w] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int k = 1; k < 4; k++) if (before(sv[k], si[k], bv, bi)) { bv = sv[k]; bi = si[k]; }
        if (tid == 0) { pv[po + r] = bv; pi[po + r] = bi; }
        pvv = bv; pii = bi;
    }
    if (tid == 0) {
        pm[(int64_t)row * chunks + chunk] = m;
        ps[(int64_t)row * chunks + chunk] = ss[0] + ss[1] + ss[2] + ss[3];
    }
}

// One wave per row: lse from the chunk pairs in chunk order, the row's top-n from the chunks' candidates, the picked id's score.
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
    const float* m_ = pm + (int64_t)row * chunks;
    const double* s_ = ps + (int64_t)row * chunks;
    float M = -INFINITY;
    for (int c = 0; c < chunks; c++) M = m_[c] > M ? m_[c] : M;
    double S = 0.0;
    for (int c = 0; c < chunks; c++)
        if (s_[c] != 0.0) S += s_[c] * exp((double)m_[c] - (double)M);                        // (a chunk of -inf holds (-inf, 0): skipped)
    const double lse = (double)M + log(S);
    // candidates: chunks * 8, lane l holds l, l + 64, ...
    const int ncand = chunks * TOPN;
    const float* cv = pv + (int64_t)row * ncand;
    const int32_t* ci = pi + (int64_t)row * ncand;
    float pvv = INFINITY; int pii = -1;
    for (int r = 0; r < n; r++) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int j = lane; j < ncand; j += 64) {
            const float v = cv[j]; const int i = ci[j];
            if (before(pvv, pii, v, i) && before(v, i, bv, bi)) { bv = v; bi = i; }
        }
        wave_best(bv, bi);
        if (lane == 0) {
            out_id[slot * TOPN + r] = bi == 0x7fffffff ? -1 : bi;
            out_tlp[slot * TOPN + r] = (float)((double)bv - lse);
        }
        pvv = bv; pii = bi;
    }
    if (lane == 0) {
        for (int r = n; r < TOPN; r++) { out_id[slot * TOPN + r] = -1; out_tlp[slot * TOPN + r] = -INFINITY; }
        const float zi = (id >= 0 && id < vocab) ? logits[(int64_t)row * ld + id] : NAN;
        out_lp[slot] = (float)((double)zi - lse);
    }
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

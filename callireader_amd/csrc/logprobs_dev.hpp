// Device code shared by the score kernels of logprobs.hip (the id a pick has just appended) and score.hip (the given targets of cr_llm_score_batch): the
// chunk reduction and the chunk-order merge.  One placement and one summation order -- chunks of 4096 scores, 16 per lane, double accumulation, the merge in
// chunk order -- so that a row's result is the same bits from either file.  logprobs.hip's header describes the scheme and its precision.
#pragma once
#include <float.h>

#include "common.hpp"
#include "logprobs.hpp"

namespace lpdev {

constexpr int CHUNK = 4096, THREADS = 256, PER = CHUNK / THREADS, TOPN = LOGPROBS_MAX_TOP;
static_assert(PER == 16 && TOPN == 8, "logprobs_dev.hpp: 16 scores per lane, 8 alternatives");

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));

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

// The chunk partials of `rows` rows in a launch's scratch (logprobs_scratch_bytes): per (row, chunk) the maximum, the sum and the top-8 as (value, id)
struct Partials {
    int chunks;                          // of a row (logprobs_chunks(vocab))
    float* pm; double* ps; float* pv; int32_t* pi;
    Partials(void* scratch, int rows, int chunks) : chunks(chunks) {
        const size_t rc = (size_t)rows * chunks;
        ps = (double*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
        pm = (float*)(ps + rc); pv = pm + rc; pi = (int32_t*)(pv + rc * TOPN);
    }
};

// RepetitionPenaltyLogitsProcessor on one score, pick.hpp apply_penalty's arithmetic
__device__ __forceinline__ float penalised(float v, float penalty) { return v < 0.f ? v * penalty : v / penalty; }

// The 16 scores of this lane of chunk `chunk` of the row lg[0, vocab): element base + (k * 256 + tid) * 4 + e, ids past the row's end as -inf.
// PEN: score i is penalised where first[i] < j (score.hip: `first` = for every id the ordinal of the first scored row of the sequence whose target it is,
// INT_MAX for an id that is nobody's target) -- in registers, the row in memory stays raw.
template <bool PEN>
__device__ __forceinline__ void load_chunk(const float* __restrict__ lg, int vocab, int base, int tid, float (&z)[PER], const int32_t* __restrict__ first = nullptr,
                                           int j = 0, float penalty = 1.0f) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i0 = base + (k * THREADS + tid) * 4;
        if (i0 + 3 < vocab) {
            const f32x4u q = *(const f32x4u*)(lg + i0);
            z[4 * k] = q.x; z[4 * k + 1] = q.y; z[4 * k + 2] = q.z; z[4 * k + 3] = q.w;
            if (PEN) {
                const i32x4u f = *(const i32x4u*)(first + i0);
#pragma unroll
                for (int e = 0; e < 4; e++) if (f[e] < j) z[4 * k + e] = penalised(z[4 * k + e], penalty);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float v = -INFINITY;
                if (i0 + e < vocab) {
                    v = lg[i0 + e];
                    if (PEN && first[i0 + e] < j) v = penalised(v, penalty);
                }
                z[4 * k + e] = v;
            }
        }
    }
}

// Partials of one (row, chunk) from the lane's 16 scores: pm = chunk maximum, ps = sum of exp(z - pm) over the chunk's entries above -inf (0 for a chunk of
// -inf), pv / pi = its top-8 in order (missing entries: -inf with id INT_MAX, which sort last).  Every thread of the 256-thread workgroup calls it.
__device__ __forceinline__ void reduce_chunk(const float (&z)[PER], int vocab, int base, int64_t part /* row * chunks + chunk */, int tid,
                                             float* __restrict__ pm, double* __restrict__ ps, float* __restrict__ pv, int32_t* __restrict__ pi) {
    __shared__ float sm[4];
    __shared__ double ss[4];
    __shared__ float sv[4];
    __shared__ int si[4];
    const int lane = tid & 63, w = tid >> 6;
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
    const int64_t po = part * TOPN;
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
        pm[part] = m;
        ps[part] = ss[0] + ss[1] + ss[2] + ss[3];
    }
}

// One wave merges the partials of row `row` IN CHUNK ORDER and writes slot `slot`: out_lp = zi - lse (zi = the scored id's entry of the row), the n best of
// the chunks' candidates as (id, z - lse) into out_id / out_tlp [slot][8], entries n..8 as id -1 and -inf (out_id / out_tlp may be NULL when n == 0).
__device__ __forceinline__ void merge_row(int64_t row, int chunks, int n, int64_t slot, float zi, int lane, const float* __restrict__ pm,
                                          const double* __restrict__ ps, const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                          float* __restrict__ out_lp, int32_t* __restrict__ out_id, float* __restrict__ out_tlp) {
    const float* m_ = pm + row * chunks;
    const double* s_ = ps + row * chunks;
    float M = -INFINITY;
    for (int c = 0; c < chunks; c++) M = m_[c] > M ? m_[c] : M;
    double S = 0.0;
    for (int c = 0; c < chunks; c++)
        if (s_[c] != 0.0) S += s_[c] * exp((double)m_[c] - (double)M);                        // (a chunk of -inf holds (-inf, 0): skipped)
    const double lse = (double)M + log(S);
    // candidates: chunks * 8, lane l holds l, l + 64, ...
    const int ncand = chunks * TOPN;
    const float* cv = pv + row * ncand;
    const int32_t* ci = pi + row * ncand;
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
        if (out_id)
            for (int r = n; r < TOPN; r++) { out_id[slot * TOPN + r] = -1; out_tlp[slot * TOPN + r] = -INFINITY; }
        out_lp[slot] = (float)((double)zi - lse);
    }
}

}  // namespace lpdev

// Beam search between two decode steps (cr_kv_set_beam): transformers' deterministic _beam_search (do_sample=False, one returned sequence, no groups or
// constraints) for groups of B = 2..8 consecutive sequences of a cache, all state on the device.  g = ids generated before the step, K = 2 B.
//
//   beam_cand_kernel    one workgroup of 1024 per beam row: lp = log_softmax(logits) in fp32, the repetition penalty over the beam's own ids ON lp (every lp is
//                       <= 0, so a penalised entry is lp * penalty; pick.hpp's gather, the > 4096-id form included), acc = running score + lp, and the row's own
//                       K largest acc in descending order, an exact tie towards the lower id.  The global top K of B x vocab is a subset of the rows' top K.
//   beam_select_kernel  one wave per group: merges the B * K candidates (tie: the lower flattened index b * vocab + id), then one lane does the bookkeeping --
//                       a candidate finishes on EOS or when g + 1 == max_new; the first B that do not finish are the next running beams; a finishing one among
//                       the first B enters the B finished slots with acc / (g + 1) ** length_penalty unless the slots are full under early_stopping=True or the
//                       early-stop heuristic is already satisfied; the group stops when the slots are full under early_stopping=True, when
//                       run[0] / L ** length_penalty <= the worst finished score (L = max_new for 'never' with a positive penalty, else g + 1), or when every
//                       candidate finished (the length limit) -- and the wave copies the new hypotheses' ids into their slots.  A group that stops is pushed
//                       onto the cache's finished queue like a sequence that cr_kv_set_stop stopped.
//   beam_reorder_kernel sequence j of a group takes the cache rows [from, length) and the id history of its source beam, K and V, every layer and KV head.
//                       In place, and safe without staging: a thread owns one 16-byte column of one (layer, head, K|V, position) for ALL beams of the group; it
//                       loads the B source values into registers, then stores the B destinations.  No other thread reads or writes those addresses, and a
//                       thread's loads all precede its stores, so a source that is also a destination is read before it is overwritten.  A beam whose source
//                       is itself moves nothing.  Traffic: 128 KiB (32 layers x 8 heads x K, V x 256 bytes) read and as much written per cached position
//                       and beam whose source changed.  A step moves every GENERATED position of such a beam, so its cost grows with the generated length
//                       g: up to rows x g x 128 KiB each way -- 0.5 GB each way for 64 rows at g = 64, but 8.4 GB at g = 1000 if every beam changed source,
//                       which is the order of the 14.7 GB of weights the step streams.  DESIGN 13 has the measured step; the copy is not optimised further
//                       here (no sharing of cache rows between beams, no per-step indirection instead of the copy: DESIGN 13 names both as follow-ups).
//                       The grid runs over the groups of the launch (their first rows), not over all its rows.
//
// No float atomics; a row's sums run in an order that depends on vocab alone (thread t adds elements t, t + 1024, ... in order, then a fixed tree), so a
// group's result does not depend on the launch it runs in.  Precision of lp: double accumulation of expf terms, the logarithm in double, one fp32 rounding:
// within 5e-6 of the float64 log-softmax for |z| <= 32 (logprobs.hip's bound, by the same argument).
#include <float.h>

#include <vector>

#include "beam.hpp"
#include "ctx.hpp"
#include "pick.hpp"

namespace {

constexpr int KMAX = 2 * BEAM_MAX;

// (value, index) order of candidates: larger value first, the lower index on an exact tie.  NaN compares false either way.
__device__ __forceinline__ bool before(float v, int64_t i, float v2, int64_t i2) { return v > v2 || (v == v2 && i < i2); }

__global__ __launch_bounds__(1024) void beam_cand_kernel(Rows rw, SeqState s, BeamLaunch p) {
    __shared__ float sf[1024];
    __shared__ double sd[1024];
    __shared__ int si[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int seq = rw.seq(row);
    const int f = s.bgrp[seq];
    if (f < 0) return;
    const BeamState* bs = p.state + f;
    if (bs->done) return;
    const int V = rw.vocab, K = 2 * bs->B;
    const float run = bs->run[seq - f];
    float* lg = rw.row(row);
    float* og = rw.orig_row(row);
    // maximum
    float m = -INFINITY;
    for (int i = tid; i < V; i += 1024) { const float z = lg[i]; m = z > m ? z : m; }
    sf[tid] = m;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) sf[tid] = sf[tid + o] > sf[tid] ? sf[tid + o] : sf[tid];
        __syncthreads();
    }
    m = sf[0];
    // sum of exp(z - m) over the entries above -inf: thread order, then a fixed tree
    double sum = 0.0;
    for (int i = tid; i < V; i += 1024) { const float z = lg[i]; if (z != -INFINITY) sum += (double)expf(z - m); }
    sd[tid] = sum;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) sd[tid] += sd[tid + o];
        __syncthreads();
    }
    const double lse = (double)m + log(sd[0]);
    for (int i = tid; i < V; i += 1024) {
        const float l = (float)((double)lg[i] - lse);
        lg[i] = l;
        if (og) og[i] = l;
    }
    __syncthreads();
    const int ng = s.ngen[seq] < s.gen_cap ? s.ngen[seq] : s.gen_cap;
    if (rw.penalty != 1.0f && ng > 0) apply_penalty(lg, s.hist(seq), ng, rw.penalty, tid, og);
    // the row's K largest acc = run + lp: round r finds the best (value, id) strictly after round r - 1's winner
    float pv = INFINITY; int pi = -1;
    for (int r = 0; r < K; r++) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < V; i += 1024) {
            const float v = run + lg[i];
            if (before(pv, pi, v, i) && before(v, i, bv, bi)) { bv = v; bi = i; }
        }
        sf[tid] = bv; si[tid] = bi;
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if (tid < o && before(sf[tid + o], si[tid + o], sf[tid], si[tid])) { sf[tid] = sf[tid + o]; si[tid] = si[tid + o]; }
            __syncthreads();
        }
        pv = sf[0]; pi = si[0];
        if (tid == 0) { p.cand_v[row * KMAX + r] = pv; p.cand_i[row * KMAX + r] = pi; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void beam_select_kernel(Rows rw, SeqState s, BeamLaunch p) {
    __shared__ float tv[KMAX];
    __shared__ int tb[KMAX], ti[KMAX];
    __shared__ int ncopy, cp_phys[BEAM_MAX], cp_src[BEAM_MAX], cp_id[BEAM_MAX];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int seq = rw.seq(row);
    const int f = s.bgrp[seq];
    if (f < 0 || seq != f) return;
    BeamState* bs = p.state + f;
    const int B = bs->B, K = 2 * B, nrows = p.first_only ? 1 : B;
    if (bs->done) {
        if (lane == 0) {
            bs->skip = 1;
            if (s.len) for (int j = 0; j < nrows; j++) s.len[f + j] += p.len_add;
        }
        return;
    }
    // merge: lane l holds candidates l and l + 64 of the group's nrows * K
    float cv[2]; int64_t cx[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const int c = lane + 64 * e;
        cv[e] = -INFINITY; cx[e] = INT64_MAX;
        if (c < nrows * K) {
            const int b = c / K, k = c % K;
            const int id = p.cand_i[(row + b) * KMAX + k];
            if (id != 0x7fffffff) { cv[e] = p.cand_v[(row + b) * KMAX + k]; cx[e] = (int64_t)b * rw.vocab + id; }
        }
    }
    float pv = INFINITY; int64_t px = -1;
    for (int r = 0; r < K; r++) {
        float bv = -INFINITY; int64_t bx = INT64_MAX;
#pragma unroll
        for (int e = 0; e < 2; e++)
            if (before(pv, px, cv[e], cx[e]) && before(cv[e], cx[e], bv, bx)) { bv = cv[e]; bx = cx[e]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64);
            const int64_t x2 = __shfl_xor(bx, o, 64);
            if (before(v2, x2, bv, bx)) { bv = v2; bx = x2; }
        }
        pv = bv; px = bx;
        if (lane == 0) {
            const bool have = bx != INT64_MAX;
            tv[r] = bv; tb[r] = have ? (int)(bx / rw.vocab) : 0; ti[r] = have ? (int)(bx % rw.vocab) : 0;
        }
    }
    __syncthreads();
    const int g = bs->g;
    if (lane == 0) {
        const int eos = bs->eos, max_new = bs->max_new, early = bs->early;
        const float lp = bs->lp;
        const bool lim = g + 1 >= max_new;
        const float denom = (float)pow((double)(g + 1), (double)lp);
        const bool eligible = !(bs->n_fin == B && early == 1) && bs->heur_ok;
        float run[BEAM_MAX]; int src[BEAM_MAX], nid[BEAM_MAX];
        int nr = 0, nfinishing = 0, nc = 0;
        for (int k = 0; k < K; k++) {
            const bool fin = lim || ti[k] == eos;
            if (!fin) {
                if (nr < B) { run[nr] = tv[k]; src[nr] = tb[k]; nid[nr] = ti[k]; nr++; }
                continue;
            }
            nfinishing++;
            if (k >= B || !eligible) continue;
            const float score = tv[k] / denom;
            if (!(score > -1.0e9f)) continue;                            // loses to an empty slot
            int n = bs->n_fin, pos, phys;
            if (n < B) { pos = n; phys = n; bs->n_fin = n + 1; }
            else if (score > bs->fin_score[B - 1]) { pos = B - 1; phys = bs->fin_phys[B - 1]; }
            else continue;
            while (pos > 0 && bs->fin_score[pos - 1] < score) {
                bs->fin_score[pos] = bs->fin_score[pos - 1]; bs->fin_len[pos] = bs->fin_len[pos - 1]; bs->fin_phys[pos] = bs->fin_phys[pos - 1];
                pos--;
            }
            bs->fin_score[pos] = score; bs->fin_len[pos] = g + 1; bs->fin_phys[pos] = phys;
            cp_phys[nc] = phys; cp_src[nc] = tb[k]; cp_id[nc] = ti[k]; nc++;
        }
        // fewer than B candidates go on (the length limit): the finishing ones fill up, in order, as transformers' acc - 1e9 ranks them
        for (int k = 0; k < K && nr < B; k++)
            if (lim || ti[k] == eos) { run[nr] = tv[k] + -1.0e9f; src[nr] = tb[k]; nid[nr] = ti[k]; nr++; }
        for (int j = 0; j < B; j++) { bs->run[j] = run[j]; bs->next_src[j] = src[j]; bs->next_id[j] = nid[j]; }
        const int L = (early == 2 && lp > 0.f) ? max_new : g + 1;
        const float best = run[0] / (float)pow((double)L, (double)lp);
        const float worst = bs->n_fin == B ? bs->fin_score[B - 1] : -1.0e9f;
        const int heur = bs->heur_ok && best > worst;
        const int stop = !heur || (bs->n_fin == B && early == 1) || nfinishing == K;
        bs->heur_ok = heur; bs->g = g + 1; bs->skip = 0; bs->done = stop;
        if (s.len) for (int j = 0; j < nrows; j++) s.len[f + j] += p.len_add;
        if (stop) s.stop.record(f, bs->n_fin > 0 ? bs->fin_len[0] : g + 1);
        ncopy = nc;
    }
    __syncthreads();
    // the new hypotheses' ids: the source beam's history + the id.  In order: a later one of the same step may take the row of an earlier one
    for (int c = 0; c < ncopy; c++) {
        int64_t* dst = p.fin_ids + (int64_t)(f + cp_phys[c]) * s.gen_cap;
        const int64_t* srcp = s.hist(f + cp_src[c]);
        for (int i = lane; i < g && i < s.gen_cap; i += 64) dst[i] = srcp[i];
        if (lane == 0 && g < s.gen_cap) dst[g] = cp_id[c];
        __syncthreads();
    }
}

constexpr int REORDER_GROUPS = 32;      // groups per launch of the re-order (their first rows travel by value)
struct BeamGroups { int row[REORDER_GROUPS]; };

// grid (position chunks of 16, layers * 16 + 1, groups), 256 threads: thread = (position, 16-byte column) of one (layer, KV head, K | V); the last y moves the ids
__global__ __launch_bounds__(256) void beam_reorder_kernel(Rows rw, SeqState s, BeamLaunch p, BeamCache c, BeamGroups gr, int append) {
    const int row = gr.row[blockIdx.z], tid = threadIdx.x;
    const int f = rw.seq(row);                         // the group's first sequence
    BeamState* bs = p.state + f;
    if (bs->skip && append) return;
    const int B = bs->B;
    int src[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; j++) src[j] = j < B ? bs->next_src[j] : j;
    const int y = blockIdx.y;
    if (y == c.layers * 16) {
        if (blockIdx.x != 0) return;
        const int n_old = append ? bs->g - 1 : s.ngen[f + src[0]];      // (without a step every beam of the group holds as many ids)
        for (int i = tid; i < n_old && i < s.gen_cap; i += 256) {
            int64_t r[BEAM_MAX];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; j++) if (j < B) r[j] = s.hist(f + src[j])[i];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; j++) if (j < B && src[j] != j) s.hist(f + j)[i] = r[j];
        }
        if (tid < B) {
            if (append && n_old < s.gen_cap) { s.hist(f + tid)[n_old] = bs->next_id[tid]; s.ngen[f + tid] = n_old + 1; }
            if (!append) s.ngen[f + tid] = n_old;
            if (p.first_only && s.len) {                                 // the fan-out: the prompt's length for every beam (len[f] is not written here)
                s.len[f + tid] = s.len[f];
                if (tid == 0) bs->prompt = s.len[f];
                if (p.share && tid > 0 && s.len[f] >= 256) { s.pfx_src[f + tid] = f; s.pfx_len[f + tid] = s.len[f] & ~255; }      // the shared fan-out
            }
        }
        return;
    }
    if (!c.k) return;
    const int len = s.len[f], from = p.first_only ? (p.share ? len & ~255 : 0) : bs->prompt;
    const int pos = from + blockIdx.x * 16 + (tid >> 4), col = tid & 15;
    if (pos >= len) return;
    const int layer = y >> 4, h = (y >> 1) & 7;
    bf16* base = ((y & 1) ? c.v : c.k) + (int64_t)layer * c.per_layer;
    uint4 r[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; j++)
        if (j < B && src[j] != j) r[j] = *(const uint4*)(base + (((int64_t)(f + src[j]) * 8 + h) * c.max_tokens + pos) * 128 + col * 8);
#pragma unroll
    for (int j = 0; j < BEAM_MAX; j++)
        if (j < B && src[j] != j) *(uint4*)(base + (((int64_t)(f + j) * 8 + h) * c.max_tokens + pos) * 128 + col * 8) = r[j];
}

__global__ __launch_bounds__(64) void set_beam_kernel(BeamState* state, int32_t* grp, int first, int B, float lp, int early, int eos, int max_new) {
    if (threadIdx.x != 0) return;
    BeamState s{};
    s.B = B; s.eos = eos; s.max_new = max_new; s.early = early; s.heur_ok = 1; s.lp = lp;
    for (int j = 0; j < BEAM_MAX; j++) { s.run[j] = j == 0 ? 0.f : -1.0e9f; s.fin_score[j] = -1.0e9f; s.next_src[j] = j; }
    state[first] = s;
    for (int j = 0; j < B; j++) grp[first + j] = first;
}

}  // namespace

size_t beam_scratch_bytes(int rows) { return (size_t)rows * KMAX * 8; }

int launch_beam_step(const Rows& r, const SeqState& s, const BeamLaunch& p, hipStream_t st) {
    hipLaunchKernelGGL(beam_cand_kernel, dim3(r.n), dim3(1024), 0, st, r, s, p);
    hipLaunchKernelGGL(beam_select_kernel, dim3(r.n), dim3(64), 0, st, r, s, p);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_beam_reorder(const Rows& r, const SeqState& s, const BeamLaunch& p, const BeamCache& c, const int* first_rows, int n_groups, int max_span, int append, hipStream_t st) {
    const int chunks = max_span > 0 ? (max_span + 15) / 16 : 1;
    for (int g0 = 0; g0 < n_groups; g0 += REORDER_GROUPS) {
        const int n = n_groups - g0 < REORDER_GROUPS ? n_groups - g0 : REORDER_GROUPS;
        BeamGroups gr{};
        for (int i = 0; i < n; i++) gr.row[i] = first_rows[g0 + i];
        hipLaunchKernelGGL(beam_reorder_kernel, dim3(chunks, c.layers * 16 + 1, n), dim3(256), 0, st, r, s, p, c, gr, append);
    }
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_set_beam(BeamState* state, int32_t* grp, int first, int B, float lp, int early, int eos, int max_new, hipStream_t st) {
    hipLaunchKernelGGL(set_beam_kernel, dim3(1), dim3(64), 0, st, state, grp, first, B, lp, early, eos, max_new);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

extern "C" int cr_op_beam_step(float* logits, int n, int vocab, int64_t* history, int hist_cap, int32_t* hist_len, float penalty, const int32_t* group,
                               void* state, int64_t* fin_ids, void* stream) {
    if (!logits || !history || !hist_len || !group || !state || !fin_ids || n <= 0 || n > 65535 || vocab < 2 * BEAM_MAX || hist_cap <= 0 || !(penalty > 0.f))
        return cr_fail(CR_ERR_ARG, "cr_op_beam_step: bad argument (a null pointer, n outside 1..65535, vocab < %d, hist_cap <= 0 or penalty <= 0)", 2 * BEAM_MAX);
    hipStream_t st = (hipStream_t)stream;
    const bool deep = hist_cap > 4096 && penalty != 1.0f;
    char* scratch = nullptr;
    const size_t cand = (beam_scratch_bytes(n) + 255) & ~(size_t)255;
    if (hipMalloc((void**)&scratch, cand + (deep ? (size_t)n * vocab * 4 : 0)) != hipSuccess) return cr_fail(CR_ERR_NOMEM, "cr_op_beam_step: scratch");
    const Rows r{logits, vocab, vocab, n, nullptr, deep ? (float*)(scratch + cand) : nullptr, penalty};
    SeqState s{};                                            // row = sequence; no cached lengths and no finished queue
    s.gen = history; s.ngen = hist_len; s.gen_cap = hist_cap; s.bgrp = const_cast<int32_t*>(group);
    const BeamLaunch p{(BeamState*)state, 0, (float*)scratch, (int32_t*)(scratch + (size_t)n * KMAX * 4), fin_ids, 0};
    int rc = launch_beam_step(r, s, p, st);
    if (rc == CR_OK) {      // the groups' first rows: the entry cannot see the device array, so it reads it back once (a test entry)
        std::vector<int32_t> hg(n);
        if (hipMemcpyAsync(hg.data(), group, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = CR_ERR_HIP;
        std::vector<int> firsts;
        for (int i = 0; i < n && rc == CR_OK; i++) if (hg[i] == i) firsts.push_back(i);
        if (rc == CR_OK && !firsts.empty()) rc = launch_beam_reorder(r, s, p, BeamCache{}, firsts.data(), (int)firsts.size(), 0, 1, st);
    }
    hipStreamSynchronize(st);
    hipFree(scratch);
    return rc;
}

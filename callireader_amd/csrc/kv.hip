// The KV cache object: struct cr_kv (kv.hpp) and every cr_kv_* entry point -- alloc and free, the three ways of forgetting a sequence (reset, truncate, fork),
// the per-sequence settings (stop, sampling, token scores, constraints, beams) and the readers.
//
// The per-sequence device state is described by seqstate.hpp's SeqState (kv.hpp: kv_seq_state builds it from a cache); every kernel here takes it by value.
// "Forget a sequence" is defined once per side: kv_clear_state on the device, Seq::clear (kv.hpp) on the host.
//   kv_reset_kernel     sequences [s0, s0 + n) get the cleared state with no cached position (cr_kv_reset).
//   kv_truncate_kernel  state only: the listed sequences hold n_tokens cached positions and nothing else that cr_kv_reset forgets.  Cache rows are not touched:
//                       rows at positions >= n_tokens are dead and the next append overwrites them.
//   kv_fork_kernel      the prefix [0, n_tokens) of one sequence to up to 64 others.  The cache is [layers][n_seqs][8][max_tokens][128] bf16, so the prefix of one
//                       (layer, KV head, K|V) is ONE contiguous run of n_tokens * 256 bytes: blockIdx.y names the run, blockIdx.x a 16 KiB tile of it.  A thread
//                       loads four 16-byte pieces of the source (all four in flight before the first store) and stores them to every destination, so the source
//                       is read once however many branches there are: traffic (1 + n_dst) * layers * 16 * n_tokens * 256 bytes.  The grid follows the byte
//                       count; positions >= n_tokens of a destination are never written.  The first workgroup also writes the destinations' state, which no
//                       other workgroup reads.  src is never a destination (checked on the host), so no address is both read and written.
//   kv_fanout_state_kernel  cr_kv_fanout, behind kv_fork_kernel: the destinations take the source's sampling parameters, stop criteria and score setting, and
//                       each its own seed; sample.hip's fan-out pick and logprobs.hip's fan-out merge then give each its first id and that id's scores.
// These four use no atomics of any kind; plain vector stores only.
#include <algorithm>
#include <initializer_list>

#include "constrain.hpp"
#include "kv.hpp"
#include "logprobs.hpp"

namespace {

constexpr int KV_FORK_MAX = 64;        // destinations of one fork (the batched decode takes 64 rows)
constexpr int FORK_THREADS = 256, FORK_PIECES = 4, FORK_TILE = FORK_THREADS * FORK_PIECES;      // 16-byte pieces per workgroup

// The sequences a launch writes, by value: no staging buffer, so calls on different streams never share one
struct KvSeqs { int32_t n; int32_t seq[KV_FORK_MAX]; };

// the cleared state: length n_tokens, no ids, no criteria and no stop, greedy, scores off, constraints off
__device__ __forceinline__ void kv_clear_state(const SeqState& s, int seq, int n_tokens) {
    s.len[seq] = n_tokens;
    s.ngen[seq] = 0;
    *s.stop.at(seq) = 0;                            // not stopped
    *s.stop.eos(seq) = -1;                          // no EOS id
    *s.stop.budget(seq) = 0;                        // no budget
    s.temp[seq] = 0.f;                              // greedy
    if (s.lpn) { s.lpn[seq] = 0; s.lpdone[seq] = 0; }
    if (s.con_on) s.con_on[seq] = 0;
    if (s.pfx_src) { s.pfx_src[seq] = -1; s.pfx_len[seq] = 0; }      // its own rows again (the host has given the count back at the source)
}

// ring: every sequence of the cache goes, and the finished ring starts over
__global__ __launch_bounds__(256) void kv_reset_kernel(SeqState s, int s0, int n, int ring) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) kv_clear_state(s, s0 + i, 0);
    if (ring && blockIdx.x == 0 && threadIdx.x == 0) *s.stop.count() = 0;
}

// pfx_len > 0: the sequences keep reading rows [0, pfx_len) of pfx_src (a sharer truncated at or above its shared length)
__global__ __launch_bounds__(64) void kv_truncate_kernel(SeqState s, KvSeqs seqs, int n_tokens, int pfx_src, int pfx_len) {
    if ((int)threadIdx.x >= seqs.n) return;
    kv_clear_state(s, seqs.seq[threadIdx.x], n_tokens);
    if (pfx_len > 0) { s.pfx_src[seqs.seq[threadIdx.x]] = pfx_src; s.pfx_len[seqs.seq[threadIdx.x]] = pfx_len; }
}

// from > 0 (cr_kv_fork_shared; a multiple of 256): only positions [from, n_tokens) are copied -- fewer than 256 -- and the destinations read rows [0, from) of src
// from then on (pfx_src / pfx_len); rows [0, from) of a destination are not written.
__global__ __launch_bounds__(FORK_THREADS) void kv_fork_kernel(SeqState s, BeamCache c, int src, KvSeqs dsts, int n_tokens, int from) {
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < dsts.n) {
        kv_clear_state(s, dsts.seq[tid], n_tokens);
        if (from > 0) { s.pfx_src[dsts.seq[tid]] = src; s.pfx_len[dsts.seq[tid]] = from; }
    }
    const int run = blockIdx.y;                     // (layer, KV head, K|V)
    const int layer = run >> 4, head = (run >> 1) & 7;
    bf16* base = ((run & 1) ? c.v : c.k) + (int64_t)layer * c.per_layer + (int64_t)head * c.max_tokens * 128;
    const int64_t per_seq = (int64_t)8 * c.max_tokens * 128;
    const int pieces = n_tokens * 16;               // 16-byte pieces of the run (max_tokens <= 32768: fits an int)
    const int p0 = from * 16 + blockIdx.x * FORK_TILE + tid;
    const uint4* sp = (const uint4*)(base + src * per_seq);
    uint4 r[FORK_PIECES];
#pragma unroll
    for (int u = 0; u < FORK_PIECES; u++) {
        const int p = p0 + u * FORK_THREADS;
        if (p < pieces) r[u] = sp[p];
    }
    for (int j = 0; j < dsts.n; j++) {
        uint4* dp = (uint4*)(base + dsts.seq[j] * per_seq);
#pragma unroll
        for (int u = 0; u < FORK_PIECES; u++) {
            const int p = p0 + u * FORK_THREADS;
            if (p < pieces) dp[p] = r[u];
        }
    }
}

// cr_kv_fanout's state, after the fork's cleared state: destination j samples as src does, with seeds.s[j]; it stops where src stops (the criteria only: it
// has no id and no stop yet); it records scores as src does.  One thread per destination.
struct FanSeeds { uint64_t s[FAN_MAX]; };
__global__ __launch_bounds__(64) void kv_fanout_state_kernel(SeqState s, int src, FanSeqs dsts, FanSeeds seeds) {
    const int j = threadIdx.x;
    if (j >= dsts.n) return;
    const int d = dsts.seq[j];
    s.temp[d] = s.temp[src]; s.topk[d] = s.topk[src]; s.topp[d] = s.topp[src]; s.seed[d] = seeds.s[j];
    *s.stop.eos(d) = *s.stop.eos(src);
    *s.stop.budget(d) = *s.stop.budget(src);
    if (s.lpn) { s.lpn[d] = s.lpn[src]; s.lpdone[d] = 0; }
}

// cr_kv_set_stop: install the criteria of `seq` and apply them to the ids it has generated already (a call after the prefill sees its first id).
// A sequence that has stopped keeps its first stop (pushed once); only the criteria are replaced.  One workgroup.
__global__ __launch_bounds__(256) void set_stop_kernel(SeqState s, int seq, int eos, int budget) {
    __shared__ int first;
    if (threadIdx.x == 0) first = 0x7fffffff;
    __syncthreads();
    const int ng = s.ngen[seq];
    if (eos >= 0)
        for (int i = threadIdx.x; i < ng; i += 256)
            if (s.hist(seq)[i] == eos) atomicMin(&first, i + 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        *s.stop.eos(seq) = eos;
        *s.stop.budget(seq) = budget;
        int at = first <= ng ? first : 0;
        if (budget > 0 && ng >= budget && (at == 0 || at > budget)) at = budget;
        if (at) s.stop.record(seq, at);
    }
}

// cr_kv_set_sampling: one sequence's sampling state
__global__ __launch_bounds__(64) void set_sampling_kernel(SeqState s, int seq, float t, int k, float p, uint64_t sd) {
    if (threadIdx.x == 0) { s.temp[seq] = t; s.topk[seq] = k; s.topp[seq] = p; s.seed[seq] = sd; }
}

// one device block of the cache, recorded as owned
template <class T> bool kv_malloc(cr_kv* kv, T** p, size_t bytes) {
    if (hipMalloc((void**)p, bytes) != hipSuccess) return false;
    kv->owned.push_back(*p);
    return true;
}

// The device blocks of a feature, allocated by the first call that switches it on: all of them or none (a failure rolls back, clears the error and leaves the
// pointers null: CR_ERR_NOMEM, the message is the caller's).  fill >= 0: the block starts as that byte throughout.  The call synchronises `st` --
// once per cache: the blocks are in place before a call on any other stream.
struct Block { void** p; size_t bytes; int fill; };
int kv_lazy_blocks(cr_kv* kv, std::initializer_list<Block> blocks, hipStream_t st) {
    const size_t had = kv->owned.size();
    for (const Block& b : blocks)
        if (!kv_malloc(kv, b.p, b.bytes)) {
            (void)hipGetLastError();
            for (; kv->owned.size() > had; kv->owned.pop_back()) { void* p = kv->owned.back(); hipFree(p); }
            for (const Block& r : blocks) *r.p = nullptr;
            return CR_ERR_NOMEM;
        }
    for (const Block& b : blocks)
        if (b.fill >= 0) CR_HIP(hipMemsetAsync(*b.p, b.fill, b.bytes, st));
    CR_HIP(hipStreamSynchronize(st));
    return CR_OK;
}

// the beam blocks of a cache
int beam_alloc(cr_kv* kv, hipStream_t st) {
    if (kv->d_beam) return CR_OK;
    const size_t N = kv->n_seqs;
    const int r = kv_lazy_blocks(kv, {{(void**)&kv->d_beam, N * sizeof(BeamState), 0}, {(void**)&kv->d_bgrp, N * 4, 0xff},
                                      {(void**)&kv->d_bfin, N * kv->gen_cap * 8, -1}}, st);
    return r == CR_ERR_NOMEM ? cr_fail(CR_ERR_NOMEM, "beam search: %zu bytes of beam state", N * (sizeof(BeamState) + 4 + (size_t)kv->gen_cap * 8)) : r;
}

// One fork launch: positions [from, n_tokens) of src to the destinations, their cleared state, and with from > 0 their share record (device and host)
int launch_fork(cr_kv* kv, int src, const KvSeqs& d, int n_tokens, int from, hipStream_t st) {
    if (from > 0) CR_TRY(kv_share_alloc(kv, st));
    const int pieces = (n_tokens - from) * 16;
    hipLaunchKernelGGL(kv_fork_kernel, dim3(std::max((pieces + FORK_TILE - 1) / FORK_TILE, 1), kv->layers * 16), dim3(FORK_THREADS), 0, st, kv_seq_state(kv), beam_cache(kv),
                       src, d, n_tokens, from);
    CR_HIP(hipGetLastError());
    for (int j = 0; j < d.n; j++) {
        Seq& t = kv->seq[d.seq[j]];
        kv_release_share(kv, d.seq[j]);
        t.clear(n_tokens);
        if (from > 0) { t.pfx_src = src; t.pfx_len = from; kv->seq[src].sharers++; }
    }
    return CR_OK;
}

// what every fork refuses of shares, before anything is enqueued: a source that itself reads a shared prompt, a destination whose rows others read
int fork_share_ok(const cr_kv* kv, const char* who, int src, const KvSeqs& d) {
    CR_TRY(kv_refuse_sharer(kv, src, who, "fork from the sequence it shares with, or from an unshared copy (cr_kv_fork)"));
    for (int j = 0; j < d.n; j++)
        if (kv->seq[d.seq[j]].sharers > 0)
            return cr_fail(CR_ERR_STATE, "%s: destination %d holds the prompt that %d other sequences share (cr_kv_reset them first)", who, d.seq[j], kv->seq[d.seq[j]].sharers);
    return CR_OK;
}

}  // namespace

int kv_share_floor(const cr_kv* kv, int seq) {
    int floor = 0;
    if (kv->seq[seq].sharers > 0)
        for (const Seq& q : kv->seq) if (q.pfx_src == seq) floor = std::max(floor, q.pfx_len);
    return floor;
}

void kv_release_share(cr_kv* kv, int seq) {
    Seq& q = kv->seq[seq];
    if (q.pfx_src >= 0) kv->seq[q.pfx_src].sharers--;
    q.pfx_src = -1; q.pfx_len = 0;
}

int kv_share_alloc(cr_kv* kv, hipStream_t st) {
    if (kv->d_pfx_src) return CR_OK;
    const size_t N = kv->n_seqs;
    const int r = kv_lazy_blocks(kv, {{(void**)&kv->d_pfx_src, N * 4, 0xff}, {(void**)&kv->d_pfx_len, N * 4, 0}}, st);
    return r == CR_ERR_NOMEM ? cr_fail(CR_ERR_NOMEM, "shared prompts: %zu bytes of share records", N * 8) : r;
}

int kv_refuse_sharer(const cr_kv* kv, int seq, const char* who, const char* alt) {
    const Seq& q = kv->seq[seq];
    if (q.pfx_src < 0) return CR_OK;
    return cr_fail(CR_ERR_STATE, "%s: sequence %d reads the first %d cached positions of sequence %d (cr_kv_fork_shared): %s", who, seq, q.pfx_len, q.pfx_src, alt);
}

RowFeatures kv_scan_rows(const cr_kv* kv, const int32_t* seqs, int n, float penalty) {
    RowFeatures f{};
    for (int i = 0; i < n; i++) {
        const Seq& s = kv->seq[seqs[i]];
        f.sampled |= s.sampled; f.scored |= s.scored; f.constrained |= s.constrained;
        f.deep |= penalty != 1.0f && s.ngen > 4096;
        f.beam_rows += s.bgrp >= 0;
        f.shares |= s.pfx_src >= 0;
    }
    return f;
}

extern "C" {

int cr_kv_alloc(cr_ctx* c, int n_seqs, int max_tokens, cr_kv** out) { return cr_kv_alloc_ex(c, n_seqs, max_tokens, CR_KV_BF16, out); }

int cr_kv_alloc_ex(cr_ctx* c, int n_seqs, int max_tokens, int format, cr_kv** out) {
    if (format != CR_KV_BF16 && format != CR_KV_E4M3)
        return cr_fail(CR_ERR_ARG, "cr_kv_alloc_ex: unknown cache format %d (CR_KV_BF16 = 0, CR_KV_E4M3 = 1)", format);
    if (!c || !out || n_seqs <= 0 || max_tokens <= 0) return cr_fail(CR_ERR_ARG, "cr_kv_alloc: bad argument (null context or output, or a size <= 0)");
    if (max_tokens > c->d.max_pos) return cr_fail(CR_ERR_ARG, "cr_kv_alloc: max_tokens %d exceeds the RoPE table (%d rows)", max_tokens, c->d.max_pos);
    CR_HIP(hipSetDevice(c->device));
    cr_kv* kv = new cr_kv();
    kv->ctx = c; kv->n_seqs = n_seqs; kv->max_tokens = max_tokens; kv->gen_cap = max_tokens; kv->layers = c->d.llm_layers; kv->fmt = format;
    const size_t rows = (size_t)kv->layers * n_seqs * NKV * max_tokens;
    const size_t bytes = rows * HD * (format == CR_KV_E4M3 ? 1 : 2);
    const bool data_ok = format == CR_KV_E4M3
        ? kv_malloc(kv, &kv->k8, bytes) && kv_malloc(kv, &kv->v8, bytes) && kv_malloc(kv, &kv->ks, rows * 4) && kv_malloc(kv, &kv->vs, rows * 4)
        : kv_malloc(kv, &kv->k, bytes) && kv_malloc(kv, &kv->v, bytes);
    if (!data_ok || !kv_malloc(kv, &kv->d_len, n_seqs * 4) || !kv_malloc(kv, &kv->d_ngen, n_seqs * 4) ||
        !kv_malloc(kv, &kv->d_stop, StopView::words(n_seqs) * 4) || !kv_malloc(kv, &kv->d_samp, (size_t)n_seqs * 24) ||
        !kv_malloc(kv, &kv->d_gen, (size_t)n_seqs * kv->gen_cap * 8)) {
        cr_kv_free(kv);
        return cr_fail(CR_ERR_NOMEM, "cr_kv_alloc: %zu bytes per K/V", bytes);
    }
    CR_HIP(hipMemset(kv->d_len, 0, n_seqs * 4));
    CR_HIP(hipMemset(kv->d_ngen, 0, n_seqs * 4));
    const StopView sv{kv->d_stop, n_seqs};
    CR_HIP(hipMemset(kv->d_stop, 0, StopView::words(n_seqs) * 4));                   // nothing finished, nobody stopped, no budget
    CR_HIP(hipMemset(sv.eos(0), 0xff, (size_t)n_seqs * 4));                          // no EOS id
    kv->d_seed = (uint64_t*)kv->d_samp; kv->d_temp = (float*)(kv->d_seed + n_seqs); kv->d_topk = (int32_t*)(kv->d_temp + n_seqs);
    kv->d_topp = (float*)(kv->d_topk + n_seqs);
    CR_HIP(hipMemset(kv->d_samp, 0, (size_t)n_seqs * 24));                           // greedy
    kv->seq.assign(n_seqs, Seq{});
    *out = kv;
    return CR_OK;
}

int cr_kv_free(cr_kv* kv) {
    if (!kv) return CR_OK;
    hipDeviceSynchronize();
    for (void* p : kv->owned) hipFree(p);
    delete kv;
    return CR_OK;
}

int cr_kv_length(const cr_kv* kv, int seq) { return (kv && seq >= 0 && seq < kv->n_seqs) ? kv->seq[seq].len : -1; }

int cr_kv_format(const cr_kv* kv) { return kv ? kv->fmt : cr_fail(CR_ERR_ARG, "cr_kv_format: null cache"); }

int cr_kv_reset(cr_kv* kv, int seq, void* stream) {
    if (!kv || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_reset: bad sequence");
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int s0 = seq < 0 ? 0 : seq, n = seq < 0 ? kv->n_seqs : 1;
    if (seq >= 0) {
        // shared prompts: a source goes after its sharers.  Dissolving a beam group releases its members' shares first (they read the group's first sequence), so
        // resetting any sequence of a group works as it always did; members that shared hold no prompt of their own and go with it
        const int f = kv->seq[seq].bgrp, B = f >= 0 ? kv->seq[f].bnum : 0;
        int outside = 0, inside = 0;
        for (int t = 0; t < kv->n_seqs; t++)
            if (kv->seq[t].pfx_src >= 0 && (kv->seq[t].pfx_src == seq || (f >= 0 && kv->seq[t].pfx_src >= f && kv->seq[t].pfx_src < f + B)))
                (f >= 0 && t >= f && t < f + B ? inside : outside)++;
        if (outside)
            return cr_fail(CR_ERR_STATE, "cr_kv_reset: %d other sequences read the prompt of sequence %d (cr_kv_fork_shared): reset them first", outside, seq);
        if (inside) { s0 = f; n = B; }
    }
    hipLaunchKernelGGL(kv_reset_kernel, dim3(std::min((n + 255) / 256, 1024)), dim3(256), 0, st, kv_seq_state(kv), s0, n, seq < 0 ? 1 : 0);
    CR_HIP(hipGetLastError());
    for (int s = s0; s < s0 + n; s++) { kv_release_share(kv, s); kv->seq[s].clear(0); }
    if (seq < 0) for (Seq& q : kv->seq) q.sharers = 0;
    if (kv->d_beam)                                                                     // a beam group goes as a whole with any of its sequences
        for (int s = s0; s < s0 + n; s++) {
            const int f = kv->seq[s].bgrp;
            if (f < 0) continue;
            const int B = kv->seq[f].bnum;
            CR_HIP(hipMemsetAsync(kv->d_bgrp + f, 0xff, (size_t)B * 4, st));
            CR_HIP(hipMemsetAsync(StopView{kv->d_stop, kv->n_seqs}.at(f), 0, 4, st));       // the group's stop record sits at its first sequence
            for (int j = 0; j < B; j++) kv->seq[f + j].bgrp = -1;
            kv->seq[f].bnum = 0;
        }
    return CR_OK;
}

int cr_kv_truncate(cr_kv* kv, int seq, int n_tokens, void* stream) {
    if (!kv || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_truncate: bad sequence");
    Seq& q = kv->seq[seq];
    if (n_tokens < 0 || n_tokens > q.len) return cr_fail(CR_ERR_ARG, "cr_kv_truncate: n_tokens %d outside 0..%d, the tokens sequence %d holds", n_tokens, q.len, seq);
    if (q.bgrp >= 0) return cr_fail(CR_ERR_STATE, "cr_kv_truncate: sequence %d belongs to the beam group of sequence %d (cr_kv_reset dissolves the group)", seq, q.bgrp);
    if (n_tokens == 0) return cr_kv_reset(kv, seq, stream);
    if (n_tokens < q.pfx_len)
        return cr_fail(CR_ERR_STATE, "cr_kv_truncate: sequence %d reads the first %d cached positions of sequence %d (cr_kv_fork_shared) and cannot be cut to %d, "
                       "below them (cr_kv_reset gives the share up)", seq, q.pfx_len, q.pfx_src, n_tokens);
    if (n_tokens < kv_share_floor(kv, seq))
        return cr_fail(CR_ERR_STATE, "cr_kv_truncate: %d other sequences read the first %d cached positions of sequence %d (cr_kv_fork_shared): not below them (reset "
                       "the sharers first)", q.sharers, kv_share_floor(kv, seq), seq);
    CR_HIP(hipSetDevice(kv->ctx->device));
    KvSeqs one{};
    one.n = 1; one.seq[0] = seq;
    const int psrc = q.pfx_src, plen = q.pfx_len;      // a sharer cut at or above its shared length keeps its share
    hipLaunchKernelGGL(kv_truncate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kv_seq_state(kv), one, n_tokens, psrc, plen);
    CR_HIP(hipGetLastError());
    q.clear(n_tokens);
    q.pfx_src = psrc; q.pfx_len = plen;
    return CR_OK;
}

// cr_kv_fork and cr_kv_fork_shared: one set of checks, one launch
static int kv_fork(const char* who, bool shared, cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, int n_tokens, void* stream) {
    if (!kv || !dsts_host || src < 0 || src >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "%s: bad argument (null cache or destinations, or a source out of range)", who);
    if (kv->fmt != CR_KV_BF16) return cr_fail(CR_ERR_ARG, "%s: the fork copies bf16 rows only (an e4m3 cache keeps no bf16 prefix for a continued prefill to read)", who);
    if (n_dst < 1 || n_dst > kv->n_seqs - 1 || n_dst > KV_FORK_MAX)
        return cr_fail(CR_ERR_ARG, "%s: %d destinations (want 1..%d)", who, n_dst, kv->n_seqs - 1 < KV_FORK_MAX ? kv->n_seqs - 1 : KV_FORK_MAX);
    if (n_tokens < 1 || n_tokens > kv->seq[src].len)
        return cr_fail(CR_ERR_ARG, "%s: n_tokens %d outside 1..%d, the tokens sequence %d holds", who, n_tokens, kv->seq[src].len, src);
    KvSeqs d{};
    d.n = n_dst;
    for (int j = 0; j < n_dst; j++) {
        const int s = dsts_host[j];
        if (s < 0 || s >= kv->n_seqs || s == src) return cr_fail(CR_ERR_ARG, "%s: destination %d (want 0..%d, not the source %d)", who, s, kv->n_seqs - 1, src);
        for (int i = 0; i < j; i++) if (dsts_host[i] == s) return cr_fail(CR_ERR_ARG, "%s: destination %d listed twice", who, s);
        d.seq[j] = s;
    }
    if (kv->seq[src].bgrp >= 0) return cr_fail(CR_ERR_STATE, "%s: the source %d belongs to the beam group of sequence %d", who, src, kv->seq[src].bgrp);
    for (int j = 0; j < n_dst; j++)
        if (kv->seq[d.seq[j]].bgrp >= 0)
            return cr_fail(CR_ERR_STATE, "%s: destination %d belongs to the beam group of sequence %d", who, d.seq[j], kv->seq[d.seq[j]].bgrp);
    CR_TRY(fork_share_ok(kv, who, src, d));
    CR_HIP(hipSetDevice(kv->ctx->device));
    // bf16 cache [layers][n_seqs][8][max_tokens][128] (k, v): positions [0, n_tokens) of `src` go to every destination, every layer, KV head, K and V, and the
    // destinations get the truncate's state -- one launch.  Shared: positions [n_tokens & ~255, n_tokens) only, the rest is read from src
    return launch_fork(kv, src, d, n_tokens, shared ? n_tokens & ~255 : 0, (hipStream_t)stream);
}

int cr_kv_fork(cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, int n_tokens, void* stream) {
    return kv_fork("cr_kv_fork", false, kv, src, dsts_host, n_dst, n_tokens, stream);
}

int cr_kv_fork_shared(cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, int n_tokens, void* stream) {
    return kv_fork("cr_kv_fork_shared", true, kv, src, dsts_host, n_dst, n_tokens, stream);
}

int cr_kv_set_prefix_sharing(cr_kv* kv, int on) {
    if (!kv) return cr_fail(CR_ERR_ARG, "cr_kv_set_prefix_sharing: null cache");
    if (on && kv->fmt != CR_KV_BF16)
        return cr_fail(CR_ERR_ARG, "cr_kv_set_prefix_sharing: an e4m3 cache (the shared fork moves bf16 rows and the e4m3 decode kernel has no group form: use a bf16 cache)");
    for (int s = 0; s < kv->n_seqs; s++)
        if (kv->seq[s].len != 0 || kv->seq[s].pfx_src >= 0 || kv->seq[s].sharers != 0)
            return cr_fail(CR_ERR_STATE, "cr_kv_set_prefix_sharing: sequence %d holds tokens or a share (switch the mode on an empty cache: cr_kv_reset(-1) first)", s);
    kv->share_mode = on != 0;
    return CR_OK;
}


int cr_kv_fanout(cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, const uint64_t* seeds_host, const float* last_logits, void* stream) {
    if (!kv || !dsts_host || src < 0 || src >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_fanout: bad argument (null cache or destinations, or a source out of range)");
    if (n_dst < 1 || n_dst > kv->n_seqs - 1 || n_dst > FAN_MAX)
        return cr_fail(CR_ERR_ARG, "cr_kv_fanout: %d destinations (want 1..%d)", n_dst, kv->n_seqs - 1 < FAN_MAX ? kv->n_seqs - 1 : FAN_MAX);
    KvSeqs d{};
    FanSeqs f{};
    d.n = f.n = n_dst;
    for (int j = 0; j < n_dst; j++) {
        const int s = dsts_host[j];
        if (s < 0 || s >= kv->n_seqs || s == src) return cr_fail(CR_ERR_ARG, "cr_kv_fanout: destination %d (want 0..%d, not the source %d)", s, kv->n_seqs - 1, src);
        for (int i = 0; i < j; i++) if (dsts_host[i] == s) return cr_fail(CR_ERR_ARG, "cr_kv_fanout: destination %d listed twice", s);
        d.seq[j] = f.seq[j] = s;
    }
    if (kv->fmt != CR_KV_BF16) return cr_fail(CR_ERR_ARG, "cr_kv_fanout: the copy moves bf16 rows only, as cr_kv_fork's (an e4m3 cache is not fanned out)");
    if (!seeds_host || !last_logits) return cr_fail(CR_ERR_ARG, "cr_kv_fanout: null seeds or last_logits");
    const Seq q = kv->seq[src];
    if (q.bgrp >= 0) return cr_fail(CR_ERR_STATE, "cr_kv_fanout: the source %d belongs to the beam group of sequence %d", src, q.bgrp);
    for (int j = 0; j < n_dst; j++)
        if (kv->seq[d.seq[j]].bgrp >= 0)
            return cr_fail(CR_ERR_STATE, "cr_kv_fanout: destination %d belongs to the beam group of sequence %d", d.seq[j], kv->seq[d.seq[j]].bgrp);
    CR_TRY(fork_share_ok(kv, "cr_kv_fanout", src, d));
    if (!q.sampled) return cr_fail(CR_ERR_STATE, "cr_kv_fanout: the source %d does not sample (cr_kv_set_sampling with a temperature > 0 before its prefill)", src);
    if (q.constrained) return cr_fail(CR_ERR_STATE, "cr_kv_fanout: the source %d carries logits constraints (its last row is not what its pick chose from)", src);
    if (q.ngen != 1 || q.len < 1)
        return cr_fail(CR_ERR_STATE, "cr_kv_fanout: the source %d holds %d generated ids and %d tokens (want the state right behind its prefill: one id)", src, q.ngen, q.len);
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int V = kv->ctx->d.vocab;
    if (q.scored && !kv->d_fan) {
        const int r = kv_lazy_blocks(kv, {{&kv->d_fan, logprobs_scratch_bytes(1, V), -1}}, st);
        if (r == CR_ERR_NOMEM) return cr_fail(CR_ERR_NOMEM, "cr_kv_fanout: %zu bytes of score partials", logprobs_scratch_bytes(1, V));
        CR_TRY(r);
    }
    // the prefix: kv_fork_kernel as cr_kv_fork launches it (the source read once, rows >= q.len of a destination not written, the cleared state); with
    // cr_kv_set_prefix_sharing on, as cr_kv_fork_shared launches it
    CR_TRY(launch_fork(kv, src, d, q.len, kv->share_mode ? q.len & ~255 : 0, st));
    const SeqState s = kv_seq_state(kv);
    FanSeeds seeds{};
    for (int j = 0; j < n_dst; j++) seeds.s[j] = seeds_host[j];
    hipLaunchKernelGGL(kv_fanout_state_kernel, dim3(1), dim3(64), 0, st, s, src, f, seeds);
    CR_HIP(hipGetLastError());
    CR_TRY(launch_sample_fan(last_logits, V, f, s, st));
    if (q.scored) CR_TRY(launch_logprobs_fan(last_logits, V, f, s, {0, kv->d_fan, kv->d_lp, kv->d_top_id, kv->d_top_lp}, st));
    for (int j = 0; j < n_dst; j++) {
        Seq& t = kv->seq[d.seq[j]];      // (launch_fork has cleared it to q.len tokens)
        t.ngen = 1; t.sampled = true; t.scored = q.scored;
    }
    return CR_OK;
}

int cr_kv_set_stop(cr_kv* kv, int seq, int eos_id, int max_new, void* stream) {
    if (!kv || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_set_stop: bad sequence");
    if (max_new > kv->max_tokens - kv->seq[seq].len)
        return cr_fail(CR_ERR_ARG, "cr_kv_set_stop: budget %d exceeds what the cache leaves after %d tokens (%d)", max_new, kv->seq[seq].len, kv->max_tokens);
    if (eos_id >= kv->ctx->d.vocab) return cr_fail(CR_ERR_ARG, "cr_kv_set_stop: EOS id %d outside the vocabulary", eos_id);
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipLaunchKernelGGL(set_stop_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, kv_seq_state(kv), seq, eos_id < 0 ? -1 : eos_id, max_new > 0 ? max_new : 0);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int cr_kv_set_sampling(cr_kv* kv, int seq, float temperature, int top_k, float top_p, uint64_t seed, void* stream) {
    if (!(temperature >= 0.f && temperature <= 3.402823466e38f) || top_k < 0 || !(top_p >= 0.f && top_p <= 1.f))
        return cr_fail(CR_ERR_ARG, "cr_kv_set_sampling: temperature %g, top_k %d, top_p %g (want a finite temperature >= 0, top_k >= 0, 0 <= top_p <= 1)",
                       temperature, top_k, top_p);
    if (!kv || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_set_sampling: bad sequence");
    if (temperature > 0.f && kv->seq[seq].bgrp >= 0) return cr_fail(CR_ERR_ARG, "cr_kv_set_sampling: sequence %d belongs to a beam group (no beam sampling)", seq);
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipLaunchKernelGGL(set_sampling_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kv_seq_state(kv), seq, temperature, top_k, top_p, seed);
    CR_HIP(hipGetLastError());
    kv->seq[seq].sampled = temperature > 0.f;
    return CR_OK;
}

int cr_kv_set_logprobs(cr_kv* kv, int seq, int top_n, void* stream) {
    if (top_n < 0 || top_n > LOGPROBS_MAX_TOP) return cr_fail(CR_ERR_ARG, "cr_kv_set_logprobs: top_n %d (want 0 = off, or 1..%d)", top_n, LOGPROBS_MAX_TOP);
    if (!kv || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_set_logprobs: bad sequence");
    if (top_n > 0 && kv->seq[seq].bgrp >= 0) return cr_fail(CR_ERR_ARG, "cr_kv_set_logprobs: sequence %d belongs to a beam group (no token scores with beams)", seq);
    if (top_n > 0 && kv->seq[seq].ngen != 0)
        return cr_fail(CR_ERR_STATE, "cr_kv_set_logprobs: sequence %d has generated %d ids already (switch scores on after cr_kv_reset and before the prefill)",
                       seq, kv->seq[seq].ngen);
    if (!kv->d_lpn && top_n == 0) return CR_OK;                                         // never switched on: nothing to switch off
    CR_HIP(hipSetDevice(kv->ctx->device));
    if (!kv->d_lpn) {
        const size_t N = kv->n_seqs, slots = N * kv->gen_cap;
        const int r = kv_lazy_blocks(kv, {{(void**)&kv->d_lpn, N * 8, 0}, {(void**)&kv->d_lp, slots * 4, -1},
                                          {(void**)&kv->d_top_id, slots * LOGPROBS_MAX_TOP * 4, -1}, {(void**)&kv->d_top_lp, slots * LOGPROBS_MAX_TOP * 4, -1}},
                                     (hipStream_t)stream);
        if (r == CR_ERR_NOMEM) return cr_fail(CR_ERR_NOMEM, "cr_kv_set_logprobs: %zu bytes of token scores", slots * (4 + 8 * LOGPROBS_MAX_TOP));
        CR_TRY(r);
        kv->d_lpdone = kv->d_lpn + N;
    }
    CR_TRY(launch_set_logprobs(kv->d_lpn, kv->d_lpdone, seq, top_n, (hipStream_t)stream));
    kv->seq[seq].scored = top_n > 0;
    return CR_OK;
}

int cr_kv_set_constraints(cr_kv* kv, int seq, const cr_constraints* c, void* stream) {
    if (c) CR_TRY(con_check(c, -1, "cr_kv_set_constraints"));                           // the values first: no cache and no device needed
    if (!kv || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_set_constraints: bad sequence");
    if (c) CR_TRY(con_check(c, kv->ctx->d.vocab, "cr_kv_set_constraints"));
    if (c && kv->seq[seq].bgrp >= 0) return cr_fail(CR_ERR_STATE, "cr_kv_set_constraints: sequence %d belongs to a beam group (no constraints with beams)", seq);
    if (!kv->d_con && !c) return CR_OK;                                                 // never switched on: nothing to switch off
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int V = kv->ctx->d.vocab;
    if (!kv->d_con) {
        const size_t N = kv->n_seqs, stride = con_block_ints(V);
        const int r = kv_lazy_blocks(kv, {{(void**)&kv->d_con_on, N * 4, 0}, {(void**)&kv->d_con, N * stride * 4, -1}}, st);
        if (r == CR_ERR_NOMEM) return cr_fail(CR_ERR_NOMEM, "cr_kv_set_constraints: %zu bytes of constraint blocks", N * (stride + 1) * 4);
        CR_TRY(r);
        kv->con_stride = stride;
    }
    if (!c) {
        CR_HIP(hipMemsetAsync(kv->d_con_on + seq, 0, 4, st));
        kv->seq[seq].constrained = false;
        return CR_OK;
    }
    std::vector<int32_t> blk;
    con_pack(c, V, blk);
    CR_HIP(hipMemcpyAsync(kv->d_con + (size_t)seq * kv->con_stride, blk.data(), blk.size() * 4, hipMemcpyHostToDevice, st));   // pageable source: staged before return
    CR_HIP(hipMemsetAsync(kv->d_con_on + seq, 1, 4, st));                               // != 0: on
    kv->seq[seq].constrained = true;
    return CR_OK;
}

int cr_kv_logprobs(cr_kv* kv, int seq, float* lp, int32_t* top_ids, float* top_lp, int max, void* stream) {
    if (!kv || !lp || !top_ids || !top_lp || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_logprobs: bad argument");
    if (!kv->d_lpn || !kv->seq[seq].scored) return cr_fail(CR_ERR_STATE, "cr_kv_logprobs: sequence %d has token scores switched off (cr_kv_set_logprobs)", seq);
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int n = kv->seq[seq].ngen < max ? kv->seq[seq].ngen : max;
    const size_t at = (size_t)seq * kv->gen_cap;
    if (n > 0) {
        CR_HIP(hipMemcpyAsync(lp, kv->d_lp + at, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        CR_HIP(hipMemcpyAsync(top_ids, kv->d_top_id + at * LOGPROBS_MAX_TOP, (size_t)n * LOGPROBS_MAX_TOP * 4, hipMemcpyDeviceToHost, st));
        CR_HIP(hipMemcpyAsync(top_lp, kv->d_top_lp + at * LOGPROBS_MAX_TOP, (size_t)n * LOGPROBS_MAX_TOP * 4, hipMemcpyDeviceToHost, st));
    }
    CR_HIP(hipStreamSynchronize(st));
    return n;
}

int cr_kv_set_beam(cr_kv* kv, int first_seq, int num_beams, float length_penalty, int early_stopping, int eos_id, int max_new, void* stream) {
    if (num_beams < 2 || num_beams > BEAM_MAX) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: num_beams %d (want 2..%d)", num_beams, BEAM_MAX);
    if (early_stopping < 0 || early_stopping > 2 || !(length_penalty >= -3.402823466e38f && length_penalty <= 3.402823466e38f))
        return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: early_stopping %d (0 False, 1 True, 2 'never') / length_penalty %g (finite)", early_stopping, length_penalty);
    if (!kv || first_seq < 0 || first_seq + num_beams > kv->n_seqs)
        return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: a group of %d from sequence %d runs past the cache's sequences", num_beams, first_seq);
    if (kv->fmt != CR_KV_BF16) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: beam search needs a bf16 cache (the re-order does not move e4m3 rows and scales)");
    if (eos_id >= kv->ctx->d.vocab) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: EOS id %d outside the vocabulary", eos_id);
    if (kv->ctx->d.vocab < 2 * BEAM_MAX) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: vocabulary of %d ids", kv->ctx->d.vocab);
    if (max_new < 1 || max_new > kv->max_tokens) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: max_new %d (want 1..max_tokens = %d)", max_new, kv->max_tokens);
    for (int j = 0; j < num_beams; j++) {
        const int s = first_seq + j;
        const Seq& q = kv->seq[s];
        if (q.sampled || q.scored) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: sequence %d samples or records token scores", s);
        if (q.constrained) return cr_fail(CR_ERR_STATE, "cr_kv_set_beam: sequence %d has logits constraints (no constraints with beams: cr_kv_set_constraints(NULL) first)", s);
        if (q.bgrp >= 0) return cr_fail(CR_ERR_ARG, "cr_kv_set_beam: sequence %d already belongs to the group of %d (cr_kv_reset first)", s, q.bgrp);
        if (q.len != 0 || q.ngen != 0) return cr_fail(CR_ERR_STATE, "cr_kv_set_beam: sequence %d holds tokens (call after cr_kv_reset, before the prefill)", s);
    }
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CR_TRY(beam_alloc(kv, st));
    CR_TRY(launch_set_beam(kv->d_beam, kv->d_bgrp, first_seq, num_beams, length_penalty, early_stopping, eos_id < 0 ? -1 : eos_id, max_new, st));
    for (int j = 0; j < num_beams; j++) kv->seq[first_seq + j].bgrp = first_seq;
    kv->seq[first_seq].bnum = num_beams;
    return CR_OK;
}

int cr_kv_beam_result(cr_kv* kv, int first_seq, int64_t* out_host, int max, float* score, int32_t* length, int32_t* done, void* stream) {
    if (!kv || !out_host || !score || !length || !done || first_seq < 0 || first_seq >= kv->n_seqs || max < 0) return cr_fail(CR_ERR_ARG, "cr_kv_beam_result: bad argument");
    if (!kv->d_beam || kv->seq[first_seq].bgrp != first_seq) return cr_fail(CR_ERR_STATE, "cr_kv_beam_result: sequence %d is not the first of a beam group", first_seq);
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    BeamState s;
    CR_HIP(hipMemcpyAsync(&s, kv->d_beam + first_seq, sizeof(s), hipMemcpyDeviceToHost, st));
    CR_HIP(hipStreamSynchronize(st));
    *done = s.done;
    *score = s.n_fin > 0 ? s.fin_score[0] : -1.0e9f;
    *length = s.n_fin > 0 ? s.fin_len[0] : 0;
    const int n = *length < max ? *length : max;
    if (n > 0) {
        CR_HIP(hipMemcpyAsync(out_host, kv->d_bfin + (size_t)(first_seq + s.fin_phys[0]) * kv->gen_cap, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        CR_HIP(hipStreamSynchronize(st));
    }
    return n;
}

int cr_kv_beam_reorder(cr_kv* kv, int first_seq, int num_beams, const int32_t* src_host, int from, void* stream) {
    if (num_beams < 2 || num_beams > BEAM_MAX) return cr_fail(CR_ERR_ARG, "cr_kv_beam_reorder: num_beams %d (want 2..%d)", num_beams, BEAM_MAX);
    if (!kv || !src_host || first_seq < 0 || first_seq + num_beams > kv->n_seqs || from < 0) return cr_fail(CR_ERR_ARG, "cr_kv_beam_reorder: bad argument");
    if (kv->fmt != CR_KV_BF16) return cr_fail(CR_ERR_ARG, "cr_kv_beam_reorder: the re-order moves bf16 rows only");
    BeamState tmp{};
    tmp.B = num_beams; tmp.prompt = from;
    for (int j = 0; j < BEAM_MAX; j++) {
        tmp.next_src[j] = j < num_beams ? src_host[j] : j;
        if (tmp.next_src[j] < 0 || (j < num_beams && tmp.next_src[j] >= num_beams)) return cr_fail(CR_ERR_ARG, "cr_kv_beam_reorder: source %d of beam %d", tmp.next_src[j], j);
    }
    const Seq& first = kv->seq[first_seq];
    for (int j = 0; j < num_beams; j++) {
        const Seq& q = kv->seq[first_seq + j];
        if (q.bgrp >= 0)
            return cr_fail(CR_ERR_STATE, "cr_kv_beam_reorder: sequence %d belongs to a live beam group (the entry is for plain sequences: it would overwrite the group's state)", first_seq + j);
        if (q.len != first.len || q.ngen != first.ngen)
            return cr_fail(CR_ERR_ARG, "cr_kv_beam_reorder: sequences %d and %d hold different counts of tokens or ids", first_seq, first_seq + j);
    }
    if (from > first.len) return cr_fail(CR_ERR_ARG, "cr_kv_beam_reorder: from %d past the %d cached tokens", from, first.len);
    for (int j = 0; j < num_beams; j++)
        if (from < kv->seq[first_seq + j].pfx_len || from < kv_share_floor(kv, first_seq + j))
            return cr_fail(CR_ERR_STATE, "cr_kv_beam_reorder: from %d lies inside a shared prompt of sequence %d (cr_kv_fork_shared): those rows are not moved", from, first_seq + j);
    CR_HIP(hipSetDevice(kv->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CR_TRY(beam_alloc(kv, st));
    // the slot of a sequence that is in no group is free: cr_kv_set_beam initialises it whole (pageable source: staged before the call returns)
    CR_HIP(hipMemcpyAsync(kv->d_beam + first_seq, &tmp, sizeof(tmp), hipMemcpyHostToDevice, st));
    const int row = first_seq;                 // no seqs: a row is its sequence
    return launch_beam_reorder(Rows{}, kv_seq_state(kv), {kv->d_beam}, beam_cache(kv), &row, 1, first.len - from, 0, st);
}

int cr_kv_poll_finished(cr_kv* kv, int32_t* host_out, int max, void* stream) {
    if (!kv || !host_out) return cr_fail(CR_ERR_ARG, "cr_kv_poll_finished: bad argument");
    const int need = (int)StopView::polled(kv->n_seqs);
    if (max < need) return cr_fail(CR_ERR_ARG, "cr_kv_poll_finished: %d int32 of room, %d needed", max, need);
    CR_HIP(hipSetDevice(kv->ctx->device));
    CR_HIP(hipMemcpyAsync(host_out, kv->d_stop, (size_t)need * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return CR_OK;
}

int cr_kv_read(cr_kv* kv, int layer, int seq, int pos, int which, void* out, void* stream) {
    if (!kv || !out || layer < 0 || layer >= kv->layers || seq < 0 || seq >= kv->n_seqs || pos < 0 || pos >= kv->max_tokens || (which != 0 && which != 1))
        return cr_fail(CR_ERR_ARG, "cr_kv_read: bad argument");
    if (kv->fmt != CR_KV_BF16) return cr_fail(CR_ERR_ARG, "cr_kv_read: the cache holds e4m3 rows, not bf16 (format %d): read them with cr_kv_read_e4m3", kv->fmt);
    CR_HIP(hipSetDevice(kv->ctx->device));
    const bf16* base = (which ? kv->v : kv->k) + (((int64_t)layer * kv->n_seqs + seq) * NKV * kv->max_tokens + pos) * HD;
    CR_HIP(hipMemcpy2DAsync(out, HD * 2, base, (size_t)kv->max_tokens * HD * 2, HD * 2, NKV, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CR_OK;
}

int cr_kv_read_e4m3(cr_kv* kv, int layer, int seq, int pos, int which, uint8_t* q_out, float* s_out, void* stream) {
    if (!kv || !q_out || !s_out || layer < 0 || layer >= kv->layers || seq < 0 || seq >= kv->n_seqs || pos < 0 || pos >= kv->max_tokens ||
        (which != 0 && which != 1))
        return cr_fail(CR_ERR_ARG, "cr_kv_read_e4m3: bad argument");
    if (kv->fmt != CR_KV_E4M3) return cr_fail(CR_ERR_ARG, "cr_kv_read_e4m3: the cache holds bf16 rows (format %d): read them with cr_kv_read", kv->fmt);
    CR_HIP(hipSetDevice(kv->ctx->device));
    const int64_t row = ((int64_t)layer * kv->n_seqs + seq) * NKV * kv->max_tokens + pos;
    CR_HIP(hipMemcpy2DAsync(q_out, HD, (which ? kv->v8 : kv->k8) + row * HD, (size_t)kv->max_tokens * HD, HD, NKV, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    CR_HIP(hipMemcpy2DAsync(s_out, 4, (which ? kv->vs : kv->ks) + row, (size_t)kv->max_tokens * 4, 4, NKV, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CR_OK;
}

int cr_kv_generated(cr_kv* kv, int seq, int64_t* out_host, int max, void* stream) {
    if (!kv || !out_host || seq < 0 || seq >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_kv_generated: bad argument");
    const int n = kv->seq[seq].ngen < max ? kv->seq[seq].ngen : max;
    if (n > 0) CR_HIP(hipMemcpyAsync(out_host, kv->d_gen + (size_t)seq * kv->gen_cap, (size_t)n * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    CR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return n;
}

}  // extern "C"

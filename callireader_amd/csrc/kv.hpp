// The KV cache object (kv.hip): struct cr_kv behind the cr_kv_* entry points, its per-sequence host record and what a prefill / decode call asks of it
#pragma once
#include <vector>

#include "beam.hpp"
#include "ctx.hpp"
#include "pick.hpp"

// InternLM2.5-7B: hidden size, head dimension, query heads, KV heads, width of the fused wqkv output.  A cache row is [NKV][max_tokens][HD].
constexpr int D = 4096, HD = 128, NH = 32, NKV = 8, QKV = 6144;

// What the host knows of one sequence: it mirrors the device state, so that an entry point checks its arguments and chooses its launches without a read-back
struct Seq {
    int len = 0, ngen = 0;                                       // tokens cached, ids generated
    bool sampled = false, scored = false, constrained = false;   // temperature > 0 / d_lpn != 0 / d_con_on != 0
    int bgrp = -1, bnum = 0;                                     // first sequence of its beam group (< 0: none); at that first sequence, the group's size
    // shared prompt (cr_kv_fork_shared): this sequence reads cache rows [0, pfx_len) of sequence pfx_src (< 0: its own; pfx_len a multiple of 256), and `sharers`
    // live sequences read this one's.  A sequence's own share goes with clear() (the caller gives the count back at the source first: kv_release_share); the
    // count belongs to the source's rows, not to its state, and stays.
    int pfx_src = -1, pfx_len = 0, sharers = 0;
    // the cleared state with n_tokens cached positions: the host side of kv.hip's kv_clear_state (the device side, over seqstate.hpp's SeqState), what reset, truncate and fork restore.  A new per-sequence
    // flag is cleared in these two places.  (Group membership goes by the group: cr_kv_reset dissolves it, truncate and fork refuse a member.)
    void clear(int n_tokens) { len = n_tokens; ngen = 0; sampled = scored = constrained = false; pfx_src = -1; pfx_len = 0; }
};

struct cr_kv {
    cr_ctx* ctx;
    int n_seqs, max_tokens, gen_cap, layers;
    int fmt;             // CR_KV_BF16 | CR_KV_E4M3 (cr_kv_alloc_ex), fixed for the cache's lifetime
    bf16* k;             // [layers][n_seqs][8][max_tokens][128]  (bf16 caches only)
    bf16* v;
    // e4m3 caches: one row = the 128 values of (layer, seq, KV head, position) as OCP e4m3fn bytes + one fp32 scale (max|x| / 448, 1 for a zero row)
    unsigned char* k8;   // [layers][n_seqs][8][max_tokens][128]
    unsigned char* v8;
    float* ks;           // [layers][n_seqs][8][max_tokens]: a wave's 64 keys read 256 contiguous bytes of scales
    float* vs;
    int32_t* d_len;      // [n_seqs] tokens cached
    int32_t* d_ngen;     // [n_seqs] ids generated
    int64_t* d_gen;      // [n_seqs][gen_cap]; gen_cap = max_tokens: every generated id costs a cached token, so the cache fills first
    // stop tracking (cr_kv_set_stop / cr_kv_poll_finished), one block of StopView::words(n_seqs) int32: seqstate.hpp's StopView has the layout
    int32_t* d_stop;
    // sampling state (cr_kv_set_sampling), one block: temperature float[n] (<= 0: greedy), top_k int32[n], top_p float[n], seed uint64[n];
    // Seq::sampled mirrors "temperature > 0" on the host: a launch whose rows are all greedy keeps pick_kernel
    char* d_samp;
    float* d_temp; int32_t* d_topk; float* d_topp; uint64_t* d_seed;
    // token scores (cr_kv_set_logprobs; logprobs.hip), allocated by the first call that switches a sequence on: d_lpn int32[n] = alternatives per sequence
    // (0: off), d_lpdone int32[n] = slots written, d_lp [n][gen_cap] fp32, d_top_id [n][gen_cap][8] int32, d_top_lp [n][gen_cap][8] fp32, indexed like
    // d_gen.  Seq::scored mirrors d_lpn on the host: a launch whose rows are all off launches nothing new
    int32_t *d_lpn = nullptr, *d_lpdone = nullptr, *d_top_id = nullptr;
    float *d_lp = nullptr, *d_top_lp = nullptr;
    // logits constraints (cr_kv_set_constraints; constrain.hip), allocated by the first call that switches a sequence on: d_con_on int32[n] (0: off), d_con
    // [n][con_stride] int32 = one block per sequence (constrain.hpp).  Seq::constrained mirrors d_con_on on the host: a launch whose rows are all off launches
    // nothing new
    int32_t *d_con_on = nullptr, *d_con = nullptr;
    size_t con_stride = 0;
    // beam groups (cr_kv_set_beam; beam.hip), allocated by the first call: d_beam BeamState[n] (a group's state at its first sequence), d_bgrp int32[n] = first
    // sequence of the sequence's group (< 0: none), d_bfin [n][gen_cap] ids of the finished slots.  Seq::bgrp / bnum mirror the group and its size on the host:
    // a launch without a group launches nothing new
    // cr_kv_fanout's score partials of its one logits row (logprobs_scratch_bytes(1, vocab)), allocated by the first fan-out of a sequence that records scores
    void* d_fan = nullptr;
    // shared prompts (cr_kv_set_prefix_sharing / cr_kv_fork_shared), allocated by the first call that shares: d_pfx_src int32[n] (-1: none), d_pfx_len int32[n].
    // Seq::pfx_src / pfx_len mirror them on the host: a launch without a sharer launches nothing new.  share_mode: cr_kv_fanout and a beam group's fan-out share
    bool share_mode = false;
    int32_t *d_pfx_src = nullptr, *d_pfx_len = nullptr;
    BeamState* d_beam = nullptr;
    int32_t* d_bgrp = nullptr;
    int64_t* d_bfin = nullptr;
    std::vector<Seq> seq;
    std::vector<void*> owned;      // every device block of the cache, recorded where it is allocated: cr_kv_free frees this list
};

// the per-sequence device state of the cache as every kernel takes it (seqstate.hpp): built once per call
inline SeqState kv_seq_state(const cr_kv* kv) {
    return {kv->d_len, kv->d_ngen, kv->d_gen, kv->gen_cap, {kv->d_stop, kv->n_seqs}, kv->d_temp, kv->d_topk, kv->d_topp, kv->d_seed, kv->d_lpn, kv->d_lpdone,
            kv->d_con_on, kv->d_bgrp, kv->d_pfx_src, kv->d_pfx_len};
}

// which features the rows seqs[0 .. n) (host) of a prefill / decode call use: scanned once per call, kept in the call's HeadBufs
RowFeatures kv_scan_rows(const cr_kv* kv, const int32_t* seqs, int n, float penalty);

// Shared prompts (kv.hip).  kv_share_floor: the largest pfx_len among the live sharers of `seq` (0: none) -- rows below it must not be rewritten.
// kv_release_share: the host side of giving up seq's share (the device side is kv_clear_state's).  kv_share_alloc: the two device arrays, by the first call that
// shares.  kv_refuse_sharer: CR_ERR_STATE with `alt` (the unshared alternative) if seq reads a shared prompt, else CR_OK.
int kv_share_floor(const cr_kv* kv, int seq);
void kv_release_share(cr_kv* kv, int seq);
int kv_share_alloc(cr_kv* kv, hipStream_t st);
int kv_refuse_sharer(const cr_kv* kv, int seq, const char* who, const char* alt);

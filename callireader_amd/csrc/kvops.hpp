// Cache operations between turns (kvops.hip): the kernels behind cr_kv_truncate / cr_kv_fork
#pragma once
#include "common.hpp"

constexpr int KV_FORK_MAX = 64;        // destinations of one fork (the batched decode takes 64 rows)

// The per-sequence device state of a cache that cr_kv_reset clears (llm.hip: cr_kv).  lpn / lpdone are NULL while no sequence has switched scores on,
// con_on while none has switched constraints on.
struct KvState {
    int32_t* len; int32_t* ngen;
    int32_t* stop; int n_seqs;         // the stop block: [1 + n + s] stop count, [1 + 2n + s] EOS id, [1 + 3n + s] budget
    float* temp;                       // sampling temperature (0: greedy)
    int32_t* lpn; int32_t* lpdone;
    int32_t* con_on;                   // logits constraints (0: off)
};
// The sequences a launch writes, by value: no staging buffer, so calls on different streams never share one
struct KvSeqs { int32_t n; int32_t seq[KV_FORK_MAX]; };

// every listed sequence: length n_tokens, no ids, no criteria and no stop, greedy, scores off, constraints off
int launch_kv_truncate(const KvState& s, const KvSeqs& seqs, int n_tokens, hipStream_t st);
// bf16 cache [layers][n_seqs][8][max_tokens][128] (k, v): positions [0, n_tokens) of `src` go to every listed sequence, every layer, KV head, K and V, and the
// listed sequences get launch_kv_truncate's state -- one launch.  per_layer = n_seqs * 8 * max_tokens * 128 elements.
int launch_kv_fork(const KvState& s, bf16* k, bf16* v, int64_t per_layer, int layers, int max_tokens, int src, const KvSeqs& dsts, int n_tokens, hipStream_t st);
// bytes the fork reads (once) for n_tokens positions of one sequence; it writes n_dst times as many
inline size_t kv_fork_bytes(int layers, int n_tokens) { return (size_t)layers * 8 * 2 * n_tokens * 256; }

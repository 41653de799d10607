// What a KV cache knows of each sequence on the device, described once: the views that every kernel behind the LM head takes by value.  A new per-sequence
// field is added to SeqState (and to kv.hpp's builder) and cleared in kv.hip's kv_clear_state; the stop rule and the append rule live here and nowhere else.
// An entry that works on plain arrays (cr_op_*) fills the fields it has and leaves the others null.
#pragma once
#include "common.hpp"

// The stop block of a cache (kv.hpp: cr_kv::d_stop; include/callireader_hip.h: cr_kv_poll_finished), n = the cache's sequences:
//   [0] finished count (monotonic), [1, 1 + n) ring of finished sequence indices (entry k at 1 + k % n), [1 + n, 1 + 2n) stop count per sequence
//   (0 = not stopped), [1 + 2n, 1 + 3n) EOS id (< 0: none), [1 + 3n, 1 + 4n) budget (<= 0: none).
// The only code that knows this layout.  p NULL: no stop tracking (cr_op_beam_step).
struct StopView {
    int32_t* p; int n;
    static constexpr size_t words(int n) { return 1 + (size_t)4 * n; }       // the block
    static constexpr size_t polled(int n) { return 1 + (size_t)2 * n; }      // its prefix that cr_kv_poll_finished copies out: count, ring, stop counts
    __host__ __device__ int32_t* count() const { return p; }
    __host__ __device__ int32_t* ring(int k) const { return p + 1 + k % n; }
    __host__ __device__ int32_t* at(int seq) const { return p + 1 + n + seq; }
    __host__ __device__ int32_t* eos(int seq) const { return p + 1 + 2 * n + seq; }
    __host__ __device__ int32_t* budget(int seq) const { return p + 1 + 3 * n + seq; }
    // The first stop of `seq` (a beam group: of its first sequence), at its `count`-th id: recorded once, and the sequence pushed onto the finished ring.
    // Returns whether this call recorded it.  One thread per sequence per launch.
    __device__ bool record(int seq, int count) const {
        if (!p || *at(seq) != 0) return false;
        *at(seq) = count;
        *ring(atomicAdd(p, 1)) = seq;
        return true;
    }
    // cr_kv_set_stop's criteria against the id `seq` has just appended (its `count`-th): the EOS id, or the count reaching the budget.  Returns whether the
    // id stopped the sequence.
    __device__ bool check(int seq, int64_t id, int count) const {
        if (!p) return false;
        const int e = *eos(seq), b = *budget(seq);
        return ((e >= 0 && id == e) || (b > 0 && count >= b)) && record(seq, count);
    }
};
static_assert(StopView::polled(5) == 1 + 5 + 5 && StopView::words(5) == StopView::polled(5) + 2 * 5, "the stop block: count, ring[n], stop count[n] | EOS[n], budget[n]");

// Per-sequence state, every array indexed by the sequence.  lpn / lpdone are NULL while no sequence has switched scores on, con_on while none has switched
// constraints on, bgrp while there is no beam group, pfx_src / pfx_len while no sequence has shared a prompt (cr_kv_fork_shared).
struct SeqState {
    int32_t* len; int32_t* ngen;           // tokens cached, ids generated
    int64_t* gen; int gen_cap;             // id histories [.][gen_cap]
    StopView stop;
    float* temp; int32_t* topk; float* topp; uint64_t* seed;      // sampling (temperature <= 0: greedy)
    int32_t* lpn; int32_t* lpdone;         // token scores: alternatives per sequence (0: off), slots written
    int32_t* con_on;                       // logits constraints (0: off)
    int32_t* bgrp;                         // first sequence of the sequence's beam group (< 0: none)
    int32_t* pfx_src; int32_t* pfx_len;    // shared prompt: the sequence whose cache rows [0, pfx_len) this one reads (< 0: its own), a multiple of 256
    __device__ int64_t* hist(int seq) const { return gen + (int64_t)seq * gen_cap; }
    __device__ bool beam_row(int seq) const { return bgrp && bgrp[seq] >= 0; }
    // Append `id` to `seq`, which held ng ids: the history slot, the count, the stop check; the cached length grows by len_add whether or not the history
    // had room.  One thread per sequence per launch.
    __device__ void append(int seq, int64_t id, int ng, int len_add) const {
        if (ng < gen_cap) {
            hist(seq)[ng] = id; ngen[seq] = ng + 1;
            stop.check(seq, id, ng + 1);
        }
        len[seq] += len_add;
    }
};

// The logits rows of one launch, [n][ld] fp32: row r belongs to sequence seqs[r] (device; NULL: r itself).  orig (may be NULL): the rows before the penalty,
// for histories of more than 4096 ids (pick.hpp: apply_penalty).
struct Rows {
    float* logits; int64_t ld; int vocab; int n;
    const int32_t* seqs; float* orig; float penalty;
    __device__ int seq(int r) const { return seqs ? seqs[r] : r; }
    __device__ float* row(int r) const { return logits + (int64_t)r * ld; }
    __device__ float* orig_row(int r) const { return orig ? orig + (int64_t)r * ld : nullptr; }
};

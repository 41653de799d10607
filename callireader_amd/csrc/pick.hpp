// Token choice shared by the greedy pick (pick.hip pick_kernel) and the sampling pick (sample.hip): the repetition penalty and the first-max-wins argmax
// run the same device code in both kernels, so a greedy row gets the same bits from either; both append through seqstate.hpp's SeqState::append, where the
// per-sequence device state, the append rule and the stop check are described.
#pragma once
#include "seqstate.hpp"

// RepetitionPenaltyLogitsProcessor (published 4.45.2 semantics) in place over the `ng` ids of history g.  Every thread of a 1024-thread workgroup
// calls it.  The scores are gathered first, then scattered: duplicates of an id all see the ORIGINAL score.  Up to 4096 ids the gather stays in
// registers; a longer history (a cache of more than 4096 tokens) needs `orig`, an untouched copy of the row that the caller made before the
// launch: every id then reads its original score from there, whatever has been scattered into lg already (duplicates write the same value).
// orig == NULL with ng > 4096 penalises the first 4096 ids only -- the callers pass a copy whenever a history can be that long.
__device__ __forceinline__ void apply_penalty(float* __restrict__ lg, const int64_t* __restrict__ g, int ng, float penalty, int tid,
                                              const float* __restrict__ orig = nullptr) {
    if (ng > 4096 && orig) {
        for (int h = tid; h < ng; h += 1024) {
            const int64_t id = g[h];
            const float v = orig[id];
            lg[id] = v < 0.f ? v * penalty : v / penalty;
        }
        __syncthreads();
        return;
    }
    float sv[4]; int64_t si[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int h = tid + k * 1024;
        si[k] = h < ng ? g[h] : -1;
        sv[k] = si[k] >= 0 ? lg[si[k]] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (si[k] >= 0) lg[si[k]] = sv[k] < 0.f ? sv[k] * penalty : sv[k] / penalty;
    __syncthreads();
}

// Argmax of lg[0, vocab), the first maximum winning; every thread of a 1024-thread workgroup calls it, the result is bi[0] after the call.
__device__ __forceinline__ void argmax_row(const float* __restrict__ lg, int vocab, int tid, float* bv, int* bi) {
    float best = -INFINITY; int besti = 0x7fffffff;
    for (int c = tid; c < vocab; c += 1024) {
        const float v = lg[c];
        if (v > best) { best = v; besti = c; }
    }
    bv[tid] = best; bi[tid] = besti;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) {
            const float v2 = bv[tid + o]; const int i2 = bi[tid + o];
            if (v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid])) { bv[tid] = v2; bi[tid] = i2; }
        }
        __syncthreads();
    }
}

// Sampling pick (sample.hip) over the rows r (modified in place: penalty).  A row's sequence indexes the history and the sampling state of s; a row whose
// temperature is not > 0 is greedy (pick_kernel's result), a row whose sequence is in a beam group is left untouched (beam.hip picks for it).  step NULL:
// step = ngen[seq]; else step[row].  append != 0: the id is appended as pick_kernel appends it (the cached length grows by len_add).  out_ids / out_kept (may
// be NULL): the id and the size of the kept set of each row (0 for a greedy row).
struct SampleLaunch { const int32_t* step; int append, len_add; int64_t* out_ids; int32_t* out_kept; };
int launch_sample(const Rows& r, const SeqState& s, const SampleLaunch& p, hipStream_t st);

// The sequences of one cr_kv_fanout, by value in the launches that take them (no staging buffer)
constexpr int FAN_MAX = 63;
struct FanSeqs { int32_t n; int32_t seq[FAN_MAX]; };
// cr_kv_fanout's picks, one launch (sample.hip sample_fan_kernel): sequence dsts.seq[j], which holds no id yet, draws its first id from the one fp32 `row`
// [vocab] (read only) with its own sampling state -- sample_kernel's thresholds and draw at step 0 -- and appends it with the stop check; the cached lengths are not
// advanced.
int launch_sample_fan(const float* row, int vocab, const FanSeqs& dsts, const SeqState& s, hipStream_t st);

// ---- what follows the LM head in a prefill / decode call (pick.hip; host) ----
struct cr_kv; struct Arena; struct BeamLaunch; struct BeamCache;

// which features the rows of a call use (kv.hip: kv_scan_rows): a call without a row that uses a feature launches nothing for it
struct RowFeatures {
    bool sampled, scored, constrained;      // a row samples / has token scores on / has logits constraints
    bool deep; int beam_rows;               // a row has more than 4096 ids under a penalty: the pick needs an untouched copy of the rows / rows in a beam group
    bool shares;                            // a row reads a shared prompt (cr_kv_fork_shared): the decode attention takes its group form for the shared splits
};

// The LM head's n rows of a prefill / decode call, carved after the layer buffers
struct HeadBufs {
    int n, V;
    RowFeatures f;
    bf16* hl;               // the normalised rows
    float* lg;              // their logits [n][V]
    void* score;            // f.scored: logprobs.hip's scratch
    float* lg0;             // f.deep: the rows before the penalty, for the pick
    char* cand;             // f.beam_rows: beam.hip's candidate scratch
    void carve(Arena& ar);
    Rows rows(const int32_t* d_seqs, float penalty) const { return {lg, V, V, n, d_seqs, lg0, penalty}; }
};

// The logits h.lg out to the caller (`out`, may be NULL), then the constraint masks of the rows that have any (the pick, the penalty's copy h.lg0 and the scores
// all see the masked row, the caller the raw one), then the pick (greedy or sampled; none if every row is a beam row) appends every row's id and adds len_add to
// its cached length, then the scores of the rows the pick has just chosen from (h.lg: the penalised rows it left) go into the sequences' slots, then the beam step
int pick_rows(cr_kv* kv, const HeadBufs& h, const int32_t* d_seqs, float penalty, int len_add, float* out, hipStream_t st, bool prefill);
// The beam step of the launch's groups, after the picks of its other rows: candidates and select on the logits rows (first_only: a prefill, which holds a
// group's first sequence only), and in a decode step the re-order behind them (the prefill's follows its set_len_kernel)
BeamLaunch beam_launch(cr_kv* kv, const HeadBufs& h, int len_add, int first_only);
BeamCache beam_cache(const cr_kv* kv);

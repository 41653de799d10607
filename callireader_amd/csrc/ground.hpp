// Grounding (ground.hip): attention probability mass per grounded row over spans of key positions, summed inside the kernel -- no probability is ever
// stored.  Behind cr_llm_ground_batch (llm.hip: launched per layer from prefill_layers, right after RoPE + split) and the test entry cr_op_span_mass (api.hip).
#pragma once
#include <vector>

#include "common.hpp"

constexpr int GROUND_MAX_SPANS = 1024;      // spans per sequence
constexpr int GROUND_ROWS = 32;             // grounded rows of ONE sequence per workgroup (one wave: the query sits on the lane)
constexpr int GROUND_GROUP_HEADS = 4;       // query heads per KV head: a wave holds the whole GQA group's queries

// The index arrays of a grounding call: one block of ints, laid out the same on the host and on the device
struct GroundIndex {
    int32_t *row_q, *row_pos, *row_seq;     // per grounded row (slot r of mass): its row in q, its position, its sequence's ordinal in the call
    int32_t* group;                         // per workgroup, 4 ints: first grounded row, rows (1..32), cache slot, sequence ordinal
    int32_t* span_off;                      // [n + 1]: sequence i owns spans span_off[i] .. span_off[i + 1]
    int32_t* spans;                         // (start, end) pairs
};
inline size_t ground_index_ints(int R, int G, int n, int total) { return 3 * (size_t)R + 4 * (size_t)G + (size_t)n + 1 + 2 * (size_t)total; }
inline GroundIndex ground_index(int32_t* p, int R, int G, int n, int total) {
    (void)total;
    return {p, p + R, p + 2 * (size_t)R, p + 3 * (size_t)R, p + 3 * (size_t)R + 4 * (size_t)G, p + 3 * (size_t)R + 4 * (size_t)G + n + 1};
}

// One sequence of a grounding call as the host sees it: its grounded rows in row order (so in position order) and its spans
struct GroundSeq {
    int slot;
    std::vector<int32_t> row_q, row_pos;
    const int32_t* spans;                   // (start, end) pairs, sorted by start, non-overlapping
    int n_spans;
};
// 0 when the spans are sorted by start, non-overlapping, not reversed and inside [0, limit); else 1 + the index of the first offender
int ground_check_spans(const int32_t* spans, int count, int limit);
int ground_groups(const std::vector<GroundSeq>& seqs);
// fills h (ground_index_ints(R, G, n, total) ints)
void ground_fill_index(const std::vector<GroundSeq>& seqs, int32_t* h);

struct SpanMassParams {
    const bf16* q;              // roped queries [row][H][128]
    const bf16* k;              // one layer's K cache [slot][H / 4][max_tokens][128]
    int H, max_tokens;
    float s_div;                // bf16-rounded scores are divided by it (the prefill attention's DIV arithmetic)
    int R, G, W;                // grounded rows, workgroups per KV head, columns of a partial row (>= every sequence's span count)
    GroundIndex ix;             // device
    float* partial;             // [H / 4][R][W] fp32: one layer's sums over a KV head's 4 query heads
    float* mass;                // [R][mass_ld] fp32
    int mass_ld;
    int first, last;            // first: mass starts from 0 (no read); last: the sum is multiplied by scale
    float scale;
};
inline size_t span_mass_partial_floats(int H, int R, int W) { return (size_t)(H / GROUND_GROUP_HEADS) * R * W; }
// mass (+)= this layer's sum over all heads; columns from a row's own sequence's span count up to mass_ld are written 0.  Two launches.
int launch_span_mass(const SpanMassParams& p, hipStream_t stream);

// Draft-verified greedy decoding (draft.hip): what follows the LM head in a cr_llm_decode_draft step, whose rows hold several consecutive positions of one sequence
#pragma once
#include "common.hpp"
#include "pick.hpp"

constexpr int DRAFT_MAX = 7;             // drafted ids per sequence and step: a window is 1 + DRAFT_MAX rows at the most
constexpr int DRAFT_MAX_ROWS = 64;       // rows per step: the K-sliced decode GEMMs, whose bits do not depend on the batch, end there

// The index block of a step with n sequences in M rows, one device allocation laid out the same on the host: first what the host fills (the drafted ids, then per
// row its offset inside its sequence's window, then per sequence its first row and its window), then what the kernels leave (per row the pick, per sequence the
// count of ids appended)
struct DraftIndex {
    int64_t* ids;                        // [n][DRAFT_MAX]
    int32_t *off, *row0, *klen;          // [M], [n], [n]
    int32_t *picks, *app;                // [M], [n]
};
inline size_t draft_index_words(int n, int M) { return (size_t)n * DRAFT_MAX + ((size_t)2 * M + 3 * n + 1) / 2; }      // int64 words
inline size_t draft_index_host_words(int n, int M) { return (size_t)n * DRAFT_MAX + ((size_t)M + 2 * n + 1) / 2; }     // ... of which the host fills these
inline DraftIndex draft_index(int64_t* p, int n, int M) {
    int32_t* q = (int32_t*)(p + (size_t)n * DRAFT_MAX);
    return {p, q, q + M, q + M + n, q + M + 2 * n, q + 2 * M + 2 * n};
}

// What the draft stage alone owns, beside the step's rows (seqs [rows]: a window's rows name the same cache slot) and the cache's per-sequence state
struct DraftLaunch {
    int n;                               // sequences of the step
    DraftIndex ix;
    bool windows;                        // some sequence has a window: the rows carry offsets (else ix.off is not read, as in a plain step)
};
// the drafted ids behind every sequence's history (slots past its count: dead until the accept step counts them in) -- before the rows are embedded
int launch_draft_stage(const Rows& r, const SeqState& s, const DraftLaunch& p, hipStream_t st);
// every row's greedy pick over its sequence's history plus the drafted ids before the row, then per sequence the accepted prefix: ids, counts, lengths, stops
int launch_draft_pick_accept(const Rows& r, const SeqState& s, const DraftLaunch& p, hipStream_t st);

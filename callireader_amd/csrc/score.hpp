// Teacher-forced scores (score.hip): the kernels behind cr_llm_score_batch / cr_op_score_rows
#pragma once
#include "common.hpp"

constexpr int SCORE_HEAD_ROWS = 256;      // rows per LM-head tile of cr_llm_score_batch: 95 MB of fp32 logits at vocab 92 553

// The per-row index block of `rows` scored rows, one device allocation laid out the same on the host: tgt[r] = the id scored in row r, hist[r] = which
// history (table) the row belongs to, ord[r] = its ordinal j among that history's rows
struct ScoreIndex { int64_t* tgt; int32_t *hist, *ord; };
inline size_t score_index_words(int rows) { return (size_t)rows * 2; }      // int64 words
inline ScoreIndex score_index(int64_t* p, int rows) { return {p, (int32_t*)(p + rows), (int32_t*)(p + rows) + rows}; }

// first [n_hist][vocab] int32: every entry INT_MAX, then first[hist[r]][tgt[r]] = min over the rows r of ord[r] -- the ordinal of the first scored row of a
// history whose target is the id.  Row j of a history is penalised at exactly the ids with first < j: the targets of the rows before it, each once.
int launch_score_table(const ScoreIndex& ix, int rows, int n_hist, int vocab, int32_t* first, hipStream_t st);

// Scores of rows [row0, row0 + rows) of the index block, whose raw fp32 logits are logits[0 .. rows)[ld] (not modified): with z = the row after the repetition
// penalty over its history (first == NULL: penalty 1, z is the row), out_lp[row0 + i] = z[tgt] - lse(z), out_id / out_tlp [row0 + i][8] = the top_n largest
// entries of z (may be NULL when top_n == 0).  scratch: logprobs_scratch_bytes(rows, vocab).  logprobs.hip's placement and summation order: a row's result is
// bit-equal to launch_logprobs on the penalised row and depends on vocab alone, not on rows, row0 or the row's place in the launch.
struct ScoreLaunch {
    const float* logits; int64_t ld; int vocab; int rows; int row0;
    ScoreIndex ix; const int32_t* first; float penalty; int top_n;
    void* scratch; float* out_lp; int32_t* out_id; float* out_tlp;
};
int launch_score_rows(const ScoreLaunch& p, hipStream_t st);

// Token scores (logprobs.hip): the kernels behind cr_kv_set_logprobs / cr_op_logprobs
#pragma once
#include "seqstate.hpp"

constexpr int LOGPROBS_MAX_TOP = 8;

// chunks of 4096 scores a row of `vocab` is split into
int logprobs_chunks(int vocab);
// bytes of device scratch launch_logprobs needs for `rows` rows (the chunk partials)
size_t logprobs_scratch_bytes(int rows, int vocab);
// Scores of the rows r that a pick has just chosen from.  Cache rows (s.lpn given): rows whose lpn[seq] is 0 are skipped; the others write slot
// t = ngen[seq] - 1 of out_lp [n_seqs][gen_cap] / out_id, out_tlp [n_seqs][gen_cap][8] with lpn[seq] alternatives, for the id gen[seq][t], and advance
// lpdone[seq].  Op rows (s.lpn NULL, gen_cap 1): every row is scored with top_n alternatives for the id gen[row] into out_*[row].
struct LogprobsLaunch { int top_n; void* scratch; float* out_lp; int32_t* out_id; float* out_tlp; };
int launch_logprobs(const Rows& r, const SeqState& s, const LogprobsLaunch& p, hipStream_t st);
int launch_set_logprobs(int32_t* lpn, int32_t* done, int seq, int top_n, hipStream_t st);
// cr_kv_fanout's scores: the one fp32 `row` [vocab] is reduced once (logprobs_chunk_kernel, one row) and merged once per sequence of `dsts` that has scores on
// (lpn > 0) into the slot of the id its pick has just appended -- what launch_logprobs writes for a row of these bits.  scratch: logprobs_scratch_bytes(1, vocab).
struct FanSeqs;
int launch_logprobs_fan(const float* row, int vocab, const FanSeqs& dsts, const SeqState& s, const LogprobsLaunch& p, hipStream_t st);

// Beam search (beam.hip): the kernels behind cr_kv_set_beam / cr_op_beam_step
#pragma once
#include "seqstate.hpp"

constexpr int BEAM_MAX = 8;            // num_beams 2..8, K = 2 * num_beams candidates per step

// Device state of one beam group: 64 four-byte words at the index of the group's FIRST sequence (cr_op_beam_step: its first row).  The layout is part
// of the ABI (include/callireader_hip.h, cr_op_beam_step).
struct BeamState {
    int32_t B, eos, max_new, early;    // num_beams; EOS id (< 0: none); max_new_tokens; early_stopping 0 False, 1 True, 2 'never'
    int32_t g;                         // ids generated per running beam so far
    int32_t done;                      // the group has stopped: later steps change nothing of it
    int32_t skip;                      // set by a step's select kernel when it found `done` on entry: that step's re-order moves nothing
    int32_t heur_ok;                   // transformers' is_early_stop_heuristic_unsatisfied (sticky)
    int32_t n_fin;                     // finished slots in use
    int32_t prompt;                    // prompt length (cache positions below it are never re-ordered after the fan-out)
    float lp;                          // length_penalty
    int32_t pad[5];
    float run[BEAM_MAX];               // running scores, descending
    float fin_score[BEAM_MAX];         // finished slots, best first (-1e9: empty)
    int32_t fin_len[BEAM_MAX];         // ... their lengths
    int32_t fin_phys[BEAM_MAX];        // ... the row of fin_ids (relative to the group's first) that holds their ids
    int32_t next_src[BEAM_MAX];        // the step's running beams: source beam ...
    int32_t next_id[BEAM_MAX];         // ... and new id
};
static_assert(sizeof(BeamState) == 256, "BeamState is 64 words");

// One step over the rows r of fp32 logits (turned into penalised log-probabilities in place; r.orig: scratch, not a copy).  s.bgrp[seq] is the first sequence of
// the row's beam group, or < 0 for a row that is no beam (left alone).  A group's rows are consecutive, in beam order, from its first sequence's row;
// first_only: the launch holds only the group's first row (the prefill: step 0, whose candidates all come from that row).  s.len (may be NULL): every sequence
// of a group gets len_add; s.stop (may be null): the cache's finished queue.  What the stage alone owns:
struct BeamLaunch {
    BeamState* state;
    int len_add;
    float* cand_v; int32_t* cand_i;                // [rows][2 * BEAM_MAX] scratch: the rows' own candidates
    int64_t* fin_ids;                              // [.][gen_cap] ids of the finished slots, row = first sequence + fin_phys
    int first_only;
    int share;                                     // with first_only (the fan-out of a cache in cr_kv_set_prefix_sharing mode): the group's other sequences take positions
                                                   // [len & ~255, len) only and read the rest from the first (s.pfx_src / s.pfx_len, set here)
};
// bf16 cache [layers][n_seqs][8][max_tokens][128] for the re-order (k NULL: id histories only) and for kv.hip's fork
struct BeamCache { bf16* k; bf16* v; int64_t per_layer; int layers, max_tokens; };

size_t beam_scratch_bytes(int rows);
// candidates + select
int launch_beam_step(const Rows& r, const SeqState& s, const BeamLaunch& p, hipStream_t st);
// re-order: sequence f + j of every group takes cache positions [from, s.len[f]) and the id history of f + next_src[j]; from = 0 with p.first_only (the
// fan-out, which also gives the group's other sequences the first one's length; with p.share, from = s.len[f] & ~255), else the group's prompt length.  The launch runs over the groups only:
// first_rows[0 .. n_groups) (host) = the launch row of each group's first sequence; max_span = the most positions any of them moves.
// append: the step's new ids go onto the histories (a step); 0: the histories' own counts are kept (cr_kv_beam_reorder).
int launch_beam_reorder(const Rows& r, const SeqState& s, const BeamLaunch& p, const BeamCache& c, const int* first_rows, int n_groups, int max_span, int append, hipStream_t st);
int launch_set_beam(BeamState* state, int32_t* grp, int first, int B, float lp, int early, int eos, int max_new, hipStream_t st);

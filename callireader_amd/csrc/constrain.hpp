// Logits constraints (constrain.hip): the kernel behind cr_kv_set_constraints / cr_op_constrain
#pragma once
#include <vector>

#include "../../include/callireader_hip.h"
#include "seqstate.hpp"

// Limits of the MULTI-token entries of bad_words (one-token entries live in the static mask and have none): words per sequence, ids per word, ids in all
constexpr int CON_MAX_WORDS = 256;
constexpr int CON_MAX_WORD_LEN = 16;
constexpr int CON_MAX_WORD_IDS = 4096;
// the kernel keeps a row's ban mask in LDS, one bit per id: 60 KiB of the 64 KiB a workgroup may ask for
constexpr int CON_MAX_VOCAB = 60 * 1024 * 8;
constexpr int CON_HDR = 8;             // header words of a block: N, m, EOS id, multi-token words, has static mask, has begin mask, 0, 0

// One sequence's block of int32 words: header [CON_HDR], static mask [mw], begin mask [mw], word offsets [CON_MAX_WORDS + 1], word ids [CON_MAX_WORD_IDS];
// mw = ceil(vocab / 32), bit (id & 31) of word (id >> 5), the bits past vocab in the last word always 0.
inline size_t con_block_ints(int vocab) { return (size_t)CON_HDR + 2 * (size_t)((vocab + 31) / 32) + CON_MAX_WORDS + 1 + CON_MAX_WORD_IDS; }

// The blocks behind SeqState::con_on: con_on[s] != 0 means sequence s is constrained by block s (per_seq) or by the one block there is (cr_op_constrain:
// every row, con_on = {1})
struct ConTables { const int32_t* blk; int64_t stride; int per_seq; };

// Host side, no device call.  con_check: CR_OK or CR_ERR_ARG with the message set; vocab < 0 checks everything that needs no vocabulary.
int con_check(const cr_constraints* c, int vocab, const char* who);
// the block of a checked cr_constraints, cut behind the last word id in use (what has to be uploaded)
void con_pack(const cr_constraints* c, int vocab, std::vector<int32_t>& blk);

// the rows r in place: the banned ids of every constrained row become -inf; a row's sequence indexes the history (ngen clamped to gen_cap) and the tables
int launch_constrain(const Rows& r, const SeqState& s, const ConTables& t, hipStream_t st);

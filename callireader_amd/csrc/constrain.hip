// Logits constraints of a greedy sequence, as masks in front of the pick: transformers' NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor,
// SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and MinNewTokensLengthLogitsProcessor (and a whitelist, the complement of a
// SuppressTokens list).  One workgroup of 1024 threads per logits row (as pick_kernel), launched by pick_rows (pick.hip) between the copy of the raw row to the
// caller and the pick.
//
// Order: every constraint writes -inf, and the repetition penalty maps -inf to -inf for any penalty > 0 (-inf * p = -inf), so masking before the penalty
// gives the row transformers' processor list gives in whatever order _get_logits_processor puts them; the masks themselves are a union and commute.
//
// A row builds its ban set as a bitmask in LDS (one bit per id, ceil(vocab / 32) words: 11.6 KB at vocab 92553):
//   1. the sequence's static mask (suppress_tokens, one-id bad words, the whitelist's complement; built on the host at set time), OR the begin mask while the
//      sequence has generated nothing -- two coalesced reads of the sequence's block;
//   2. the EOS id while ng < min_new_tokens;
//   3. no_repeat_ngram_size N: thread i of every 1024 compares g[i .. i + N - 2] with the history's last N - 1 ids and bans g[i + N - 1] (atomicOr on LDS;
//      the whole history, also past the 4096 ids the penalty keeps in registers).  The ids come from global memory: the tail is N - 1 ids that every
//      thread reads (cached), the window slides by one id per thread (coalesced);
//   4. multi-id bad words: one thread per word compares its prefix with the history's tail.  A word of L ids is looked at from ng >= L on, not from
//      ng >= L - 1 where its prefix would fit: SequenceBiasLogitsProcessor (NoBadWords' base) skips a word "longer than the context", and its result is
//      the one kept here;
//   5. a popcount of the mask: when it equals vocab (nothing survives) bit 0 is cleared, id 0 keeps its raw value and the pick is 0 -- torch.argmax's answer
//      on an all -inf row.  (argmax_row alone would leave 0x7fffffff, and the next step's embedding gather would read far outside the table.)
//   6. one coalesced pass over the row that stores -inf where the bit is set.  Nothing else of the row is read or written: unbanned values keep their bits.
// No float atomics, no scratch: a handful of scalars per thread; LDS = the mask + 16 partial counts.  The result depends only on (constraints, history).
#include <string.h>

#include "constrain.hpp"
#include "ctx.hpp"

namespace {

__global__ __launch_bounds__(1024) void constrain_kernel(Rows r, SeqState s, ConTables t) {
    extern __shared__ uint32_t ban[];      // [mw]
    __shared__ int cnt[16];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int seq = r.seq(row), vocab = r.vocab;
    const int cs = t.per_seq ? seq : 0;
    if (!s.con_on[cs]) return;                // the whole workgroup: an unconstrained row is left untouched
    const int32_t* blk = t.blk + (int64_t)cs * t.stride;
    const int mw = (vocab + 31) >> 5;
    const int N = blk[0], m = blk[1], eos = blk[2], n_words = blk[3], has_mask = blk[4], has_begin = blk[5];
    const uint32_t* mask = (const uint32_t*)(blk + CON_HDR);
    const uint32_t* bmask = mask + mw;
    const int32_t* woff = blk + CON_HDR + 2 * mw;
    const int32_t* wids = woff + CON_MAX_WORDS + 1;
    int ng = s.ngen[seq];
    ng = ng < s.gen_cap ? ng : s.gen_cap;
    const int64_t* __restrict__ g = s.hist(seq);
    const bool begin = has_begin && ng == 0;
    for (int w = tid; w < mw; w += 1024) {
        uint32_t u = has_mask ? mask[w] : 0u;
        if (begin) u |= bmask[w];
        ban[w] = u;
    }
    __syncthreads();
    if (tid == 0 && eos >= 0 && eos < vocab && ng < m) atomicOr(&ban[eos >> 5], 1u << (eos & 31));
    if (N > 0) {
        const int64_t* tail = g + (ng - N + 1);                 // read only when the loop runs: ng >= N
        for (int i = tid; i <= ng - N; i += 1024) {
            bool eq = true;
            for (int j = 0; j < N - 1; j++)
                if (g[i + j] != tail[j]) { eq = false; break; }
            const int64_t id = g[i + N - 1];
            if (eq && id >= 0 && id < vocab) atomicOr(&ban[id >> 5], 1u << (id & 31));
        }
    }
    for (int w = tid; w < n_words; w += 1024) {
        const int o = woff[w], L = woff[w + 1] - o;
        if (L < 2 || ng < L) continue;                          // transformers ignores a word longer than the context (see above)
        bool eq = true;
        for (int j = 0; j < L - 1; j++)
            if (g[ng - (L - 1) + j] != (int64_t)wids[o + j]) { eq = false; break; }
        const int id = wids[o + L - 1];
        if (eq && id >= 0 && id < vocab) atomicOr(&ban[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    int c = 0;
    for (int w = tid; w < mw; w += 1024) c += __popc(ban[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wv] = c;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < 16; k++) total += cnt[k];
        if (total >= vocab) ban[0] &= ~1u;                      // nothing survives: id 0 keeps its raw value
    }
    __syncthreads();
    float* __restrict__ lg = r.row(row);
    for (int i = tid; i < vocab; i += 1024)
        if ((ban[i >> 5] >> (i & 31)) & 1u) lg[i] = -INFINITY;
}

int bad_ids(const int32_t* ids, int n, int vocab) {             // index of the first id outside [0, vocab) (vocab < 0: only < 0), or -1
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || (vocab >= 0 && ids[i] >= vocab)) return i;
    return -1;
}

}  // namespace

int con_check(const cr_constraints* c, int vocab, const char* who) {
    if (c->no_repeat_ngram_size < 0) return cr_fail(CR_ERR_ARG, "%s: no_repeat_ngram_size %d (want >= 0)", who, c->no_repeat_ngram_size);
    if (c->min_new_tokens < 0) return cr_fail(CR_ERR_ARG, "%s: min_new_tokens %d (want >= 0)", who, c->min_new_tokens);
    if (c->n_suppress < 0 || c->n_begin_suppress < 0 || c->n_bad_words < 0 || (c->n_suppress > 0 && !c->suppress) ||
        (c->n_begin_suppress > 0 && !c->begin_suppress) || (c->n_bad_words > 0 && (!c->bad_word_ids || !c->bad_word_offsets)))
        return cr_fail(CR_ERR_ARG, "%s: a negative count or a missing id array", who);
    if (c->allowed && c->n_allowed < 1) return cr_fail(CR_ERR_ARG, "%s: an empty whitelist (%d ids) permits nothing", who, c->n_allowed);
    if (vocab >= 0 && c->eos_id >= vocab) return cr_fail(CR_ERR_ARG, "%s: EOS id %d outside the vocabulary of %d", who, c->eos_id, vocab);
    if (vocab > CON_MAX_VOCAB) return cr_fail(CR_ERR_ARG, "%s: vocabulary of %d ids (the ban mask in LDS holds %d)", who, vocab, CON_MAX_VOCAB);
    int k;
    if ((k = bad_ids(c->suppress, c->n_suppress, vocab)) >= 0) return cr_fail(CR_ERR_ARG, "%s: suppress id %d outside the vocabulary", who, c->suppress[k]);
    if ((k = bad_ids(c->begin_suppress, c->n_begin_suppress, vocab)) >= 0)
        return cr_fail(CR_ERR_ARG, "%s: begin_suppress id %d outside the vocabulary", who, c->begin_suppress[k]);
    if (c->allowed && (k = bad_ids(c->allowed, c->n_allowed, vocab)) >= 0) return cr_fail(CR_ERR_ARG, "%s: allowed id %d outside the vocabulary", who, c->allowed[k]);
    int words = 0, ids = 0;
    if (c->n_bad_words > 0 && c->bad_word_offsets[0] != 0) return cr_fail(CR_ERR_ARG, "%s: bad_word_offsets[0] = %d (want 0)", who, c->bad_word_offsets[0]);
    for (int w = 0; w < c->n_bad_words; w++) {
        const int o = c->bad_word_offsets[w], L = c->bad_word_offsets[w + 1] - o;
        if (L < 1) return cr_fail(CR_ERR_ARG, "%s: bad word %d is empty (offsets %d, %d)", who, w, o, o + L);
        if ((k = bad_ids(c->bad_word_ids + o, L, vocab)) >= 0) return cr_fail(CR_ERR_ARG, "%s: bad word %d holds id %d outside the vocabulary", who, w, c->bad_word_ids[o + k]);
        if (L == 1) continue;
        if (L > CON_MAX_WORD_LEN) return cr_fail(CR_ERR_ARG, "%s: bad word %d has %d ids (at most %d)", who, w, L, CON_MAX_WORD_LEN);
        words++; ids += L;
        if (words > CON_MAX_WORDS || ids > CON_MAX_WORD_IDS)
            return cr_fail(CR_ERR_ARG, "%s: more than %d bad words of two or more ids, or more than %d ids in them", who, CON_MAX_WORDS, CON_MAX_WORD_IDS);
    }
    return CR_OK;
}

void con_pack(const cr_constraints* c, int vocab, std::vector<int32_t>& blk) {
    const int mw = (vocab + 31) / 32;
    blk.assign(con_block_ints(vocab), 0);
    uint32_t* mask = (uint32_t*)(blk.data() + CON_HDR);
    uint32_t* bmask = mask + mw;
    int32_t* woff = blk.data() + CON_HDR + 2 * mw;
    int32_t* wids = woff + CON_MAX_WORDS + 1;
    bool has_mask = false;
    if (c->allowed) {                                           // the complement of the whitelist; the bits past vocab stay 0
        has_mask = true;
        for (int w = 0; w < mw; w++) mask[w] = 0xffffffffu;
        if (vocab & 31) mask[mw - 1] = (1u << (vocab & 31)) - 1;
        for (int i = 0; i < c->n_allowed; i++) mask[c->allowed[i] >> 5] &= ~(1u << (c->allowed[i] & 31));
    }
    for (int i = 0; i < c->n_suppress; i++) { mask[c->suppress[i] >> 5] |= 1u << (c->suppress[i] & 31); has_mask = true; }
    for (int i = 0; i < c->n_begin_suppress; i++) bmask[c->begin_suppress[i] >> 5] |= 1u << (c->begin_suppress[i] & 31);
    int words = 0, ids = 0;
    for (int w = 0; w < c->n_bad_words; w++) {
        const int o = c->bad_word_offsets[w], L = c->bad_word_offsets[w + 1] - o;
        if (L == 1) { mask[c->bad_word_ids[o] >> 5] |= 1u << (c->bad_word_ids[o] & 31); has_mask = true; continue; }
        memcpy(wids + ids, c->bad_word_ids + o, (size_t)L * 4);
        ids += L;
        woff[++words] = ids;
    }
    blk[0] = c->no_repeat_ngram_size; blk[1] = c->min_new_tokens; blk[2] = c->eos_id < 0 ? -1 : c->eos_id; blk[3] = words;
    blk[4] = has_mask; blk[5] = c->n_begin_suppress > 0;
    blk.resize(con_block_ints(vocab) - CON_MAX_WORD_IDS + ids);
}

int launch_constrain(const Rows& r, const SeqState& s, const ConTables& t, hipStream_t st) {
    hipLaunchKernelGGL(constrain_kernel, dim3(r.n), dim3(1024), (size_t)((r.vocab + 31) / 32) * 4, st, r, s, t);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

extern "C" int cr_op_constrain(const cr_constraints* c, float* logits, int n, int vocab, const int32_t* seqs, const int64_t* history, int hist_cap,
                               const int32_t* hist_len, void* stream) {
    if (!c || !logits || n <= 0 || n > 65535 || vocab <= 0 || !hist_len || hist_cap < 0 || (!history && hist_cap > 0))
        return cr_fail(CR_ERR_ARG, "cr_op_constrain: bad argument");
    CR_TRY(con_check(c, vocab, "cr_op_constrain"));
    std::vector<int32_t> blk;
    con_pack(c, vocab, blk);
    blk.push_back(1);                                           // the `on` word of the one block, behind it
    hipStream_t st = (hipStream_t)stream;
    int32_t* d = nullptr;
    if (hipMalloc((void**)&d, (con_block_ints(vocab) + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return cr_fail(CR_ERR_NOMEM, "cr_op_constrain: %zu bytes of tables", (con_block_ints(vocab) + 1) * 4);
    }
    int32_t* d_on = d + con_block_ints(vocab);
    hipError_t e = hipMemcpyAsync(d, blk.data(), (blk.size() - 1) * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_on, &blk.back(), 4, hipMemcpyHostToDevice, st);
    int r = CR_OK;
    SeqState s{};                                               // the arrays stand for the histories; the one switch is on
    s.gen = const_cast<int64_t*>(history); s.ngen = const_cast<int32_t*>(hist_len); s.gen_cap = hist_cap; s.con_on = d_on;
    if (e == hipSuccess) r = launch_constrain({logits, vocab, vocab, n, seqs, nullptr, 1.0f}, s, {d, 0, 0}, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    hipFree(d);
    if (e != hipSuccess || e2 != hipSuccess) return cr_fail(CR_ERR_HIP, "cr_op_constrain: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return r;
}

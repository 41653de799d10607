/* callireader_hip.h — C ABI of libcallireader_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for CalliReader's image->text hot path.  The reference is pure
 * Python; each entry point replaces the PyTorch module call named next to it
 * (paths relative to the reference repo).  The Python binding a maintainer would
 * add is shown in INTEGRATION.md and shipped as callireader_amd/_binding.py.
 *
 * Conventions
 *   - every pointer argument is a DEVICE pointer owned by the caller unless it is
 *     documented as host; buffers are dense row-major bf16 unless stated;
 *   - every launch takes a hipStream_t (passed as void*); calls only enqueue work,
 *     except cr_create/cr_destroy/cr_load_weight/cr_finalize/cr_kv_alloc/cr_kv_free,
 *     which may allocate and synchronise;
 *   - return value: 0 = CR_OK, negative = error; cr_last_error() returns a
 *     thread-local, NUL-terminated description of the last failure;
 *   - no exceptions cross the ABI, no internal threads, one context per device,
 *     a context is not re-entrant.
 */
#ifndef CALLIREADER_HIP_H
#define CALLIREADER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CR_ABI_VERSION 13  /* 13 (additions that change no existing entry point keep the number: a caller built against the earlier v13 header runs unchanged, and a binding that names a missing symbol fails at load): cr_llm_score_batch, cr_op_score_rows; cr_kv_set_constraints, cr_op_constrain, cr_kv_reset / cr_kv_truncate / cr_kv_fork also switch constraints off; cr_kv_truncate, cr_kv_fork; cr_kv_set_beam, cr_kv_beam_result, cr_kv_beam_reorder, cr_op_beam_step, cr_kv_reset also dissolves beam groups; cr_kv_set_logprobs, cr_kv_logprobs, cr_op_logprobs, cr_kv_reset also switches token scores off; cr_kv_alloc_ex (CR_KV_E4M3 caches), cr_kv_format, cr_kv_read_e4m3, cr_op_decode_attention_e4m3, cr_kv_read refuses e4m3 caches; 12: cr_kv_set_sampling, cr_op_sample, cr_kv_reset clears the sampling state; 11: cr_kv_set_stop, cr_kv_poll_finished, cr_kv_reset clears the stop state, seqs staging per context; 10: cr_op_decode_attention(+_scratch_floats); 9: cr_build_flags, cr_diag_register; 8: cr_op_decode_swizzle, cr_op_decode_gemm flags bit 8, cr_op_gemm bits 18-19; 7: cr_op_decode_gemm; 6: cr_build_id, cr_llm_hidden_probe; 5: cr_share_weights, cr_op_gemm_q8, cr_op_norm_fp8 takes the next linear's bound; 4: cr_enable_fp8_mfma, cr_op_norm_fp8, cr_op_gemm bit 17; 2: cr_orderformer; cr_op_gemm kernel pin and EPI_PARTIAL (epi 7); 3: cr_profile_stats, cr_kv_read, cr_kv_reset takes a stream, cr_enable_fp8_decode, cr_op_quantize_fp8, epi 8 */

enum { CR_OK = 0, CR_ERR_ARG = -1, CR_ERR_HIP = -2, CR_ERR_STATE = -3, CR_ERR_NOMEM = -4 };
enum { CR_BF16 = 0, CR_F32 = 1, CR_I64 = 2, CR_I32 = 3, CR_U8 = 4 /* library-internal: e4m3 weight copies */ };

typedef struct cr_ctx cr_ctx;
typedef struct cr_kv cr_kv;

/* Shapes: InternVL/config.json (vision_config :114-143, llm_config :14-103, downsample_ratio :11),
 * models/perceiver_resampler.py:54-64, InternVL/modeling_internvl_chat.py:157. */
typedef struct cr_model_desc {
    int32_t vit_layers;     /* 24  */
    int32_t rs_depth;       /* 4   */
    int32_t llm_layers;     /* 32  */
    int32_t vocab;          /* 92553 */
    int32_t max_pos;        /* rows of the RoPE tables handed over by the host (<= 32768) */
    float vit_ln_eps;       /* 1e-6 */
    float rms_eps;          /* 1e-5 */
    int32_t reserved[8];
} cr_model_desc;

const char* cr_last_error(void);
int cr_abi_version(void);
/* sha256 (first 16 hex digits) of the .hip / .hpp sources and of this header the library was compiled from, set by
 * callireader_amd/build.py (-DCR_BUILD_ID): lets a log prove which source tree a run used.  "unknown" for a hand build. */
const char* cr_build_id(void);
/* Names of the diagnostic macros any translation unit of this library was compiled with (callireader_amd/csrc/diag.hpp: knock-out / poison / stamp builds
 * made by scripts/build_variant.py, several of which give wrong results by design), space-separated; "" for the product build.  The ctypes binding refuses a
 * library that reports any unless CR_HIP_LIB names it explicitly.  cr_diag_register is how such a translation unit announces itself (load time). */
const char* cr_build_flags(void);
int cr_diag_register(const char* flags);

/* ---- lifetime & weights --------------------------------------------------------------------- */
/* InternVLChatModel.__init__ (InternVL/modeling_internvl_chat.py:136-194) */
int cr_create(int device, const cr_model_desc* desc, cr_ctx** out);
int cr_destroy(cr_ctx* ctx);
/* Two stages in flight (the batched decode of one batch of pages beside the visual stage and prefill of the next; the reference runs
 * page after page, modeling_internvl_chat.py:649-762 -- a throughput arrangement above the same per-page results).  A context is
 * not re-entrant: its stage entry points carve their activations out of one grow-only workspace.  cr_share_weights makes `dst`
 * (fresh from cr_create with the same description) use the weights, derived tensors and fp8 copies of the finalized `src` WITHOUT
 * copying them: a second host thread can then run stages through `dst` on its own stream (own workspace, own profiler) while
 * the first works through `src`.  KV caches (cr_kv_alloc) are plain device state and may be filled through one context and read
 * through the other; ordering between the two streams is the caller's (events).  `src` must outlive `dst`; call again after
 * reloading weights or toggling the fp8 options on `src`.
 * One cache, two contexts at once (continuous batching): a context can prefill some sequences of a cache on its stream while a
 * context that shares its weights decodes OTHER sequences of the same cache on another stream -- prefill and decode touch only the
 * device state of the sequences they are given (the seqs[] staging is per context), and cr_kv_reset / cr_kv_set_stop only that
 * of their sequence.  Each sequence is used by one context at a time, and reusing a sequence (cr_kv_reset, then a prefill through
 * the other context) must be ordered after the last decode step that included it: record an event on the decoding stream after
 * that step and make the prefilling stream wait for it.  A decode must likewise wait for the prefill of a sequence it adds. */
int cr_share_weights(cr_ctx* dst, const cr_ctx* src);
/* One call per checkpoint tensor; `name` is the safetensors key (InternVL/model.safetensors.index.json), or
 *   "calli.mu" / "calli.sigma"  (vocab,1)  — params/gauss_norm_mu_sigma.pth columns (modeling_internvl_chat.py:153-155)
 *   "rope.cos" / "rope.sin"     (max_pos,128) bf16 — InternLM2DynamicNTKScalingRotaryEmbedding cache
 *                                (InternVL/modeling_internlm2.py:213-229), built on the host exactly as the reference does.
 * The library copies (and may re-layout) the data; `src_is_host` selects H2D vs D2D. */
int cr_load_weight(cr_ctx* ctx, const char* name, const void* src, int dtype, const int64_t* shape, int ndim,
                   int src_is_host, void* stream);
/* Build derived tensors once all weights are in (K-padded patch kernel, interleaved w1|w3, L2-normalised VQ table). */
int cr_finalize(cr_ctx* ctx, void* stream);

/* ---- vision ---------------------------------------------------------------------------------- */
/* InternVisionModel.forward(pixel_values).last_hidden_state — InternVL/modeling_intern_vit.py:399-437
 * pixels [T,3,448,448] -> out [T,1025,1024] */
int cr_vit_forward(cr_ctx* ctx, const void* pixels, int T, void* out, void* stream);
/* drop CLS + pixel_shuffle(0.5, v2) + mlp1 — InternVL/modeling_internvl_chat.py:283-297,311-318
 * vit_out [T,1025,1024] -> out [T,256,4096] */
int cr_project(cr_ctx* ctx, const void* vit_out, int T, void* out, void* stream);
/* InternVLChatModel.extract_feature — InternVL/modeling_internvl_chat.py:299-319 (= the two calls above) */
int cr_extract_feature(cr_ctx* ctx, const void* pixels, int T, void* out, void* stream);

/* ---- tile preprocessing (host side of the reference: utils/utils.py:354-478) ------------------------------- */
/* One resize job: crop [sx0,sy0,sw,sh] of the page, Pillow Image.resize((ow,oh)) (default BICUBIC, antialiased),
 * then either mode 0: paste at (left,top) on a white 448x448 canvas = ONE tile `tile0` (load_image_2, :420-452), or
 * mode 1: cut into 448x448 tiles tile0.. row-major, `cols` per row (dynamic_preprocess, :381-417; cols = ow/448). */
typedef struct cr_prep_job {
    int32_t sx0, sy0, sw, sh, ow, oh, mode, tile0, cols, left, top;
} cr_prep_job;
/* page_rgb: device uint8 [H][W][3]; jobs: host array; lut: device bf16 [3][256] = bf16((p/255 - mean_c)/std_c) built by
 * the host with the reference's fp32 expression (build_transform, :354-362); out_tiles: device bf16 [n_tiles,3,448,448].
 * Bit-identical to the reference's PIL/torch pipeline (tests/test_gpu_prep.py). */
int cr_preprocess(cr_ctx* ctx, const void* page_rgb, int H, int W, const cr_prep_job* jobs, int n_jobs, const void* lut,
                  void* out_tiles, int n_tiles, void* stream);

/* ---- CalliAlign ------------------------------------------------------------------------------- */
/* PerceiverResampler.forward — models/perceiver_resampler.py:81-100:  in [T,256,4096] -> out [T,3,4096] */
int cr_resample(cr_ctx* ctx, const void* in, int T, void* out, void* stream);
/* vq_cos_sim — models/similarity.py:9-27:  in [n,4096] -> idx [n] int64, cos [n] bf16 (cos may be NULL) */
int cr_vq(cr_ctx* ctx, const void* in, int n, int64_t* idx, void* cos, void* stream);
/* calli_align tail — InternVL/modeling_internvl_chat.py:602-640.
 * flags bit0 = drop_zero, bit1 = hard_vq (needs cos).  out [n,4096]; *n_out (device int32) = rows kept. */
int cr_denorm(cr_ctx* ctx, const void* in, const int64_t* idx, const void* cos, int n, int flags,
              void* out, int32_t* n_out, void* stream);

/* ---- language model --------------------------------------------------------------------------- */
/* generate_ocr / generate_origin head — InternVL/modeling_internvl_chat.py:1081-1107,1033-1052:
 * out[s] = tok_embeddings[ids[s]], rows with ids == img_id overwritten by vit_embeds (in order),
 * rows with ids == ref_id by ref_embeds.  n_vit / n_ref rows must equal the id counts (checked on the host side). */
int cr_embed_splice(cr_ctx* ctx, const int64_t* ids, int S, const void* vit_embeds, int n_vit, int64_t img_id,
                    const void* ref_embeds, int n_ref, int64_t ref_id, void* out, void* stream);

/* KV cache for `n_seqs` sequences of up to `max_tokens` tokens: replaces the reference's tuple cache grown by
 * torch.cat (InternVL/modeling_internlm2.py:383-388).  The object also keeps, per sequence, the ids generated so
 * far — what transformers' generate() carries as `input_ids` when only inputs_embeds is given — so that the
 * repetition penalty and the next step's input never leave the device. */
int cr_kv_alloc(cr_ctx* ctx, int n_seqs, int max_tokens, cr_kv** out);
/* The same with a cache format (cr_kv_alloc is CR_KV_BF16); an unknown format is CR_ERR_ARG, checked before ctx.
 * CR_KV_E4M3 (an option, OFF by default; a THROUGHPUT option that does not preserve the reference's tokens, like the fp8 weight paths): every cached
 * row -- the 128 values of one (layer, seq, KV head, position), K after RoPE, V as projected -- is kept as OCP e4m3fn bytes with one fp32 scale,
 * quantised from the bf16 row a bf16 cache would hold by the rule of cr_op_quantize_fp8: s = max|x| / 448 (1 for a zero row), q = e4m3fn_rne(x * (1 / s)).
 * 67 584 bytes per cached token instead of 131 072; no bf16 K / V is kept.
 *   - prefill: the prompt attends over its exact bf16 K / V (a per-context staging buffer, one layer at a time) -- its logits and first id are
 *     bit-identical to a bf16 cache's -- and only the e4m3 rows go to the cache.  Hence a prefill into a sequence that already holds tokens is CR_ERR_ARG
 *     on an e4m3 cache (there is no bf16 copy of the prefix): cr_kv_reset the sequence first.
 *   - decode attends over the dequantised cache, the new token's own row included (quantised before it is attended to): score = bf16(bf16(s_k * (q . k^))
 *     / sqrt(128)) with the dot in fp32, output = sum_t bf16(p_t) * s_v,t * v^_t in fp32.  A row's result still depends only on its own key count.
 *   - everything else (ids, lengths, stop tracking, sampling, cr_kv_reset, sharing between contexts) is the format-independent state of the cache; any
 *     context that decodes the cache reads it in its format.  A process run with CR_DECODE_ATTN=0 refuses to decode an e4m3 cache (CR_ERR_ARG). */
enum { CR_KV_BF16 = 0, CR_KV_E4M3 = 1 };
int cr_kv_alloc_ex(cr_ctx* ctx, int n_seqs, int max_tokens, int format, cr_kv** out);
int cr_kv_format(const cr_kv* kv);                     /* CR_KV_BF16 | CR_KV_E4M3, or < 0 */
int cr_kv_free(cr_kv* kv);
int cr_kv_length(const cr_kv* kv, int seq);           /* tokens currently cached (host-side bookkeeping) */
/* Forget sequence `seq` (length 0, no generated ids), or every sequence when seq < 0.  Enqueued on `stream`, no
 * device-wide synchronisation: ordered after earlier work on that stream and before what the caller enqueues next. */
int cr_kv_reset(cr_kv* kv, int seq, void* stream);
/* Roll `seq` back to its first n_tokens cached positions: it keeps positions [0, n_tokens) and forgets everything else that cr_kv_reset forgets -- its
 * generated ids, its stop criteria and stop count, its sampling state (greedy again; a later sampled pick's `step` counts from 0), its token scores (off) and its logits constraints (off).
 * cr_kv_length and the host-side id count follow.  State only: no cache row is touched, rows at positions >= n_tokens are dead and later appends overwrite
 * them.  n_tokens == 0 is cr_kv_reset of the sequence.  What it is for: the next turn of a conversation whose prompt begins with what the cache holds -- cut
 * the speculative rows behind EOS, continue with cr_llm_prefill of the new rows; the repetition penalty of the new turn then sees that turn's ids only, as
 * the processors of a `generate` call do.  Any cache format.  CR_ERR_ARG for n_tokens outside 0..cr_kv_length(seq), CR_ERR_STATE for a member of a live
 * beam group.  Enqueued on `stream`, no device-wide synchronisation.  Added within ABI v13. */
int cr_kv_truncate(cr_kv* kv, int seq, int n_tokens, void* stream);
/* Give the n_dst sequences dsts_host[] (host array) the prefix of `src`: each becomes a sequence that holds cached positions [0, n_tokens) of src -- every
 * layer, KV head, K and V -- and is otherwise as after cr_kv_truncate(dst, n_tokens): no ids, no criteria, greedy, scores off, no constraints.  One launch of the copy kernel
 * of csrc/kvops.hip, which reads the source once however many destinations there are ((1 + n_dst) * layers * 4096 * n_tokens bytes of traffic); rows of a
 * destination at positions >= n_tokens are not written; src is unchanged.  A row's bits do not depend on its sequence, so a destination continued by a
 * prefill computes what src continued by that prefill computes.  CR_ERR_ARG for n_tokens outside 1..cr_kv_length(src), n_dst outside 1..min(n_seqs - 1, 64),
 * a destination equal to src, repeated or out of range, or an e4m3 cache (left out, as for the beam re-order: it keeps no bf16 prefix for a continued
 * prefill to read anyway); CR_ERR_STATE for a beam-group member on either side.  Enqueued on `stream`.  Added within ABI v13. */
int cr_kv_fork(cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, int n_tokens, void* stream);
/* cr_kv_fork without the copy of the prompt: cr_kv_fork's arguments, checks and resulting state, but only positions [n_tokens & ~255, n_tokens) of src are copied
 * (fewer than 256, every layer, KV head, K and V) and every destination records that it READS positions [0, n_tokens & ~255) of src: its share (pfx_src = src,
 * pfx_len = n_tokens & ~255, a multiple of the decode attention's 256-key split).  Rows [0, pfx_len) of a destination are not written.  With n_tokens < 256
 * nothing is shared and the call is cr_kv_fork.  cr_llm_decode then loads each shared 256-key split of src once for all the rows of the call that share it
 * (csrc/attention_decode_group.hip) and runs the per-row arithmetic of the unshared kernel for each: ids, logits and scores are bit-equal to cr_kv_fork's.
 * The first call that shares allocates two int32[n_seqs] arrays and synchronises `stream` once.
 * Lifetime, all CR_ERR_STATE, nothing changes on refusal.  While a source has sharers: cr_kv_reset of it, cr_kv_truncate of it below the largest pfx_len of its
 * sharers, a prefill / scoring / grounding call that would write below that length, and a fork or fan-out INTO it are refused; cr_kv_reset(-1) always goes.
 * cr_kv_reset of a sharer gives its share up; so does a fork or fan-out into it.  Resetting a sequence of a beam group dissolves the group as it always did: its
 * members' shares (cr_kv_set_prefix_sharing) go first, and members that shared are reset with it.  On a sequence that shares: cr_kv_truncate below its pfx_len
 * (at or above keeps the share), a continued prefill, cr_llm_score_batch, cr_llm_ground_batch, cr_llm_decode_draft, and cr_kv_fork / cr_kv_fork_shared /
 * cr_kv_fanout FROM it are refused -- the prefill attention and the draft forms read a sequence's own rows; use cr_kv_fork for those.  Added within ABI v13. */
int cr_kv_fork_shared(cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, int n_tokens, void* stream);
/* Cache-level mode, default off: while on, cr_kv_fanout's copy and the fan-out of a beam group's prompt after its prefill are cr_kv_fork_shared's (the last
 * n & ~255 .. n positions copied, the rest read from the source / the group's first sequence); everything else they do -- state, first ids, scores, lengths -- is
 * unchanged, and so is every result (bit for bit).  Later beam steps re-order positions [prompt length, length) only, which lie past every share.  Accepted only
 * while no sequence of the cache holds tokens or a share (CR_ERR_STATE otherwise); CR_ERR_ARG to switch it on for an e4m3 cache.  Added within ABI v13. */
int cr_kv_set_prefix_sharing(cr_kv* kv, int on);
/* Several sampled answers from one prefill.  `src` has just been prefilled (cr_llm_prefill / cr_llm_prefill_batch) with sampling on: S cached positions, ONE
 * generated id.  Each of the n_dst sequences dsts_host[] (host array) becomes what a lone prefill of the same prompt into it would have left behind
 * cr_kv_set_sampling(dst, src's temperature / top_k / top_p, seeds_host[j]) -- and cr_kv_set_logprobs(dst, src's top_n) if src records scores:
 *   - cache positions [0, S) of every layer, KV head, K and V are src's bits, the cached length is S (positions >= S of a destination are not written);
 *   - it holds one generated id, drawn at step 0 with seeds_host[j] from last_logits (device, [vocab] fp32): the raw last row the prefill of src returned
 *     through its `logits` argument.  The thresholds and the draw are the sampling pick's own code: the id is cr_op_sample's on that row, seed and step.
 *     The first pick sees no history, so no repetition penalty applies, and the row is read only;
 *   - its stop criteria (cr_kv_set_stop) are src's and have been applied to that id: a sequence whose first id is the EOS id, or whose budget is 1, is
 *     pushed onto the finished queue;
 *   - if src records token scores, slot 0 holds the id's log-probability and the row's top-n, bit-equal to what the prefill recorded for src's row.
 * src is not changed.  Launches: the copy kernel of cr_kv_fork (the source read once), one small state kernel, ONE pick launch for all destinations (a
 * workgroup of 1024 each), and with scores one reduction of the row and one merge per destination.  No LM head, no float atomics, enqueued on `stream`
 * with no device-wide synchronisation (the first scored call of a cache allocates its partials and synchronises `stream` once).
 * Checked before anything is enqueued, nothing changes on refusal: CR_ERR_ARG for n_dst outside 1..min(n_seqs - 1, 63), a destination equal to src,
 * repeated or out of range, an e4m3 cache (as for cr_kv_fork), null seeds_host or last_logits; CR_ERR_STATE for a beam-group member on either side, a
 * src that does not sample (temperature 0), that carries logits constraints, or that does not hold exactly one generated id.  Added within ABI v13. */
int cr_kv_fanout(cr_kv* kv, int src, const int32_t* dsts_host, int n_dst, const uint64_t* seeds_host, const float* last_logits, void* stream);
/* One cached position as the reference's tuple cache holds it (InternVL/modeling_internlm2.py:383-388, K after RoPE):
 * out [8 kv heads][128] bf16 (device) = past_key_values[layer][which][seq, :, pos, :]; which 0 = K, 1 = V.  Parity tests.  The slot's OWN memory, with no
 * redirection: below the pfx_len of a sequence that shares (cr_kv_fork_shared) it returns whatever the slot held before, not the source's rows. */
int cr_kv_read(cr_kv* kv, int layer, int seq, int pos, int which, void* out, void* stream);
/* The same position of an e4m3 cache (cr_kv_read refuses one): q_out [8 kv heads][128] e4m3 bytes, s_out [8] fp32 scales (both device).  Parity tests. */
int cr_kv_read_e4m3(cr_kv* kv, int layer, int seq, int pos, int which, uint8_t* q_out, float* s_out, void* stream);
/* Copy the ids generated so far for `seq` into host memory (at most `max`); returns the count, or < 0.  A sequence never holds more than
 * the cache's max_tokens ids (every id costs a cached token; a full cache is cr_llm_decode's CR_ERR_ARG), so max = max_tokens reads them all.
 * Synchronises `stream`. */
int cr_kv_generated(cr_kv* kv, int seq, int64_t* out_host, int max, void* stream);
/* Stop criteria of `seq`, checked by the greedy pick of every later prefill / decode of it (and, at this call, against the ids it has
 * generated already): the first time the sequence appends `eos_id` (< 0: no EOS id) or its generated-id count reaches `max_new`
 * (<= 0: no budget), the count so far (the stop included) is recorded as its stop count and its index is pushed ONCE onto the cache's
 * finished queue.  Nothing else changes: ids, lengths and the host-side counts keep advancing with every step that includes the
 * sequence; ids past the stop are speculative and are the caller's to cut.  Without criteria a step computes exactly what it did
 * before.  cr_kv_reset clears a sequence's criteria and stop; call this once per sequence after it.  CR_ERR_ARG when max_new exceeds
 * what the cache leaves after the tokens cached so far (max_tokens - cr_kv_length(seq)); there is no other limit: a sequence keeps one
 * generated id per prefill / decode call, every call caches at least one token, so the id buffer is sized by max_tokens.
 * Enqueued on `stream`. */
int cr_kv_set_stop(cr_kv* kv, int seq, int eos_id, int max_new, void* stream);
/* Sampling state of `seq` (transformers 4.45.2 _sample with do_sample=True): every later pick of the sequence applies the repetition penalty,
 * then scores / temperature (fp32), top-k (top_k == 0: off; ties at the k-th value kept), top-p (top_p >= 1: off; ascending fp32(1 - top_p)
 * cut of the softmax cumsum, the maximum always kept, every id tied at the boundary value kept) and draws from the softmax of the kept ids by an
 * exponential race: argmax over kept i of z_i - log(-log u_i) (double), lowest id on a tie, with
 *     u_i = ((x >> 8) + 0.5) * 2^-24,   x = word (i % 4) of Philox-4x32-10(counter = {i / 4, step, 0, 0}, key = {seed & 0xffffffff, seed >> 32}),
 *     step = the sequence's generated-id count before the pick (0 for the prefill's pick),
 * so a draw depends only on (seed, step, logits, history), not on the batch, the row or the decode kernels.  temperature == 0 means greedy (the
 * default, what cr_kv_reset restores).  CR_ERR_ARG for a negative, infinite or NaN temperature, top_k < 0, or top_p outside [0, 1] (checked
 * before the cache and sequence).  A finite temperature small enough for logit / temperature to overflow is accepted: those scores are +-inf, a
 * +inf score wins the draw (the lowest such id); NaN scores are never kept, and a row with no kept score above -inf gets the greedy pick's id.  The prefill makes the
 * sequence's first pick: call this after cr_kv_reset and BEFORE the sequence's prefill (cr_kv_set_stop may come after it).  A launch whose rows
 * are all greedy runs the greedy pick exactly as before.  Enqueued on `stream`. */
int cr_kv_set_sampling(cr_kv* kv, int seq, float temperature, int top_k, float top_p, uint64_t seed, void* stream);
/* Token scores of `seq`: top_n = 0 switches them off (the default, and what cr_kv_reset restores), 1..8 on with that many alternatives.  While on, every
 * pick of the sequence (the prefill's is t = 0) is followed by the score kernels (csrc/logprobs.hip), which record for the t-th generated id
 *     z           = the fp32 score row the pick chose from: the LM-head logits AFTER the repetition penalty and before anything else.  For a greedy
 *                   sequence that is transformers' scores[t]; for a sampled one (cr_kv_set_sampling) it is the SAME row, i.e. before temperature /
 *                   top-k / top-p, whereas transformers' scores under do_sample=True are the warped ones: a confidence describes the model, not the warper
 *     lse         = m + log(sum_i exp(z_i - m)), m = max_i z_i, -inf entries contributing 0
 *     logprob[t]  = z[id_t] - lse                        (what compute_transition_scores(normalize_logits=True) returns for greedy search)
 *     top_ids[t][0..n), top_logprobs[t][0..n) = the n largest entries of z, descending, an exact tie broken towards the LOWER id (the greedy pick's
 *                   rule: top_ids[t][0] == id_t for a greedy sequence), as id and z - lse; entries n..8 of a step hold id -1 and -inf
 * A row is summed in an order that depends on vocab alone (fixed chunks of 4096 scores, merged in chunk order, no float atomics): the scores of a
 * sequence are bit-equal whatever batch, row, slot, stream or pipeline computes them.  Accuracy: within 5e-6 absolute of the float64 log-softmax for
 * |z| <= 32 (double accumulation, one fp32 rounding of the result).  A row holding NaN or +inf gives NaN log-probabilities for that step (ids
 * unspecified).  With scores off for every row of a launch nothing is launched or changed; ids and logits never depend on the setting.  The blocks (cr_kv_logprobs' layout, 68 bytes per generated id,
 * max_tokens ids per sequence) are allocated by the first call that switches a sequence of the cache on.  CR_ERR_ARG for top_n outside 0..8 (checked
 * before the cache and sequence), CR_ERR_STATE when switching on a sequence that has generated ids already: call after cr_kv_reset and BEFORE the
 * sequence's prefill.  Cache state like the stop criteria and the sampling state: any cache format, any decode option, a cache shared between
 * contexts.  Enqueued on `stream` (the first switching-on call of a cache also synchronises it).  Added within ABI v13. */
int cr_kv_set_logprobs(cr_kv* kv, int seq, int top_n, void* stream);
/* The twin of cr_kv_generated: copy the scores of the ids generated so far for `seq` into host memory (at most `max` steps): lp [max] fp32, top_ids
 * [max][8] int32, top_lp [max][8] fp32.  Returns the count (cr_kv_generated's), or < 0: CR_ERR_STATE for a sequence whose scores are off.
 * Synchronises `stream`.  Added within ABI v13. */
int cr_kv_logprobs(cr_kv* kv, int seq, float* lp, int32_t* top_ids, float* top_lp, int max, void* stream);
/* Logits constraints of a greedy sequence (csrc/constrain.hip): what transformers' NoRepeatNGram / NoBadWords / SuppressTokens /
 * SuppressTokensAtBegin / MinNewTokensLength processors do, as masks.  All arrays are HOST arrays, read before the call returns. */
typedef struct cr_constraints {
    int32_t no_repeat_ngram_size;          /* N >= 0; 0: off */
    int32_t min_new_tokens;                /* m >= 0: eos_id is banned while fewer than m ids have been generated (max of min_new_tokens / min_length) */
    int32_t eos_id;                        /* the call's EOS id, < 0: none (min_new_tokens then bans nothing) */
    int32_t n_suppress;                    /* suppress_tokens: banned at every step */
    const int32_t* suppress;
    int32_t n_begin_suppress;              /* begin_suppress_tokens: banned at the sequence's first pick only */
    const int32_t* begin_suppress;
    int32_t n_allowed;                     /* whitelist: with allowed != NULL every id NOT listed is banned at every step (n_allowed >= 1) */
    const int32_t* allowed;
    int32_t n_bad_words;                   /* bad_words_ids: word w is bad_word_ids[bad_word_offsets[w] .. bad_word_offsets[w + 1]), offsets[0] = 0 */
    const int32_t* bad_word_ids;
    const int32_t* bad_word_offsets;       /* n_bad_words + 1 entries */
    int32_t reserved[8];                   /* 0 */
} cr_constraints;
/* Constraints of `seq`: before every later pick of the sequence (the prefill's included) one workgroup sets the banned ids of its fp32 score row to -inf, in
 * front of the repetition penalty and the pick (masks commute with the penalty: -inf stays -inf for any penalty > 0, so the result is transformers' whatever
 * order its processor list has).  With g[0 .. ng) = the ids the sequence has generated (the prompt is not seen: the reference generates from inputs_embeds),
 *   - suppress, one-id bad words and the complement of `allowed`: always;   begin_suppress: while ng == 0;   eos_id: while ng < min_new_tokens;
 *   - no_repeat_ngram_size N: g[i + N - 1] for every i in [0, ng - N] with g[i .. i + N - 2] == g[ng - N + 1 .. ng - 1] (N = 1: every generated id), over the
 *     whole history;
 *   - a bad word of L >= 2 ids: its last id when ng >= L and the last L - 1 generated ids equal its first L - 1 (ng >= L, not L - 1: transformers'
 *     SequenceBiasLogitsProcessor ignores a word longer than the ids generated so far, and its result is the one kept);
 *   - a row in which every id would be banned keeps id 0 at its raw value: the pick is id 0, torch.argmax's answer on an all -inf row.
 * The logits a prefill / decode call returns stay the raw rows; token scores (cr_kv_set_logprobs) see the masked, penalised row.  c == NULL switches the
 * sequence off, as cr_kv_reset, cr_kv_truncate and cr_kv_fork do for the sequences they reset.  A launch in which no row is constrained launches nothing.
 * Limits of the bad words of two or more ids: 256 words, 16 ids per word, 4096 ids in all; vocab <= 491520.  Checked BEFORE the cache and any device call:
 * CR_ERR_ARG for N < 0, m < 0, a negative count, a missing array, an id < 0, an empty whitelist or bad word, offsets that do not ascend from 0, or a limit
 * passed; then CR_ERR_ARG for a bad cache / sequence or an id >= vocab; CR_ERR_STATE for a member of a beam group (and cr_kv_set_beam refuses a constrained
 * sequence with CR_ERR_STATE).  Call after cr_kv_reset and BEFORE the prefill.  The blocks (about 41 KB per sequence at vocab 92553) are allocated by the first
 * call that switches a sequence of the cache on, which also synchronises `stream`.  Enqueued on `stream`.  Added within ABI v13. */
int cr_kv_set_constraints(cr_kv* kv, int seq, const cr_constraints* c, void* stream);
/* Beam search (csrc/beam.hip): the `num_beams` (2..8) consecutive sequences first_seq .. first_seq + num_beams - 1 become one beam group that runs the
 * deterministic beam search of transformers 5.x GenerationMixin._beam_search (do_sample=False, one returned sequence, no group / diverse / constrained beams)
 * as `generate(inputs_embeds=...)` drives it, entirely on the device.  With g = ids generated before a step, B = num_beams, K = 2 B, every step
 *   1. lp = log_softmax(logits) in fp32 per running beam, then the repetition penalty over that beam's own generated ids ON lp (lp <= 0: a penalised entry
 *      is lp * penalty) -- not the greedy pick's order (penalty on the raw logits);
 *   2. acc = running score + lp; the K largest of the flattened [B x vocab] in descending order, an exact tie towards the lower flattened index b * vocab + id
 *      (torch.topk leaves ties open).  Running scores start as [0, -1e9, ...]: step 0, the prefill's, takes all candidates from the one prompt row;
 *   3. a candidate finishes when its id is eos_id or g + 1 == max_new;
 *   4. the first B candidates that do not finish are the next running beams (source beam, id, acc);
 *   5. a finishing candidate among the first B of the K enters the B finished slots (initially -1e9) with acc / (g + 1) ** length_penalty, unless the slots
 *      are full and early_stopping is 1, or the early-stop heuristic is already satisfied; the B best are kept;
 *   6. the group stops when early_stopping is 1 and the slots are full, when running score[0] / L ** length_penalty <= the worst finished score (L = max_new
 *      for early_stopping 2 ('never') with length_penalty > 0, else g + 1; while a slot is empty the worst is -1e9), or when all K candidates finished (the
 *      length limit).  A stopped group is pushed onto the finished queue (cr_kv_poll_finished: its first sequence, stop count = the best hypothesis' length);
 *      later steps that include it keep appending cache rows and change nothing else.
 * Between two steps sequence j of the group is given the cache rows and the id history of its source beam (in place; after step 0 the prompt's rows fan out from
 * the first sequence).  A row's bits do not depend on its batch, so a beam whose rows were copied computes what a sequence that generated those ids itself computes.
 * Call after cr_kv_reset and BEFORE the prefill, like the sampling state; cr_kv_reset of any member dissolves the group.  early_stopping: 0 False, 1 True,
 * 2 'never'; eos_id < 0: none.  cr_llm_prefill / cr_llm_prefill_batch take the group's FIRST sequence only (any other member: CR_ERR_ARG); cr_llm_decode takes
 * all num_beams sequences, consecutive and in order in seqs[] (a partial group or force_tokens with a group: CR_ERR_ARG, nothing changes).  Groups and plain greedy
 * or sampled sequences may share a launch; those keep their bits.  The ids of a group's member sequences (cr_kv_generated) are the running beams': internal.
 * CR_ERR_ARG for num_beams outside 2..8, a group that runs past n_seqs, a member that samples, records token scores or belongs to a group already, early_stopping
 * outside 0..2, max_new outside 1..max_tokens, or an e4m3 cache (left out: the re-order moves bf16 rows only); CR_ERR_STATE for a member that holds tokens or ids.
 * The state blocks (256 bytes + 8 max_tokens bytes per sequence) are allocated by the first call on a cache, which also synchronises `stream`.  Enqueued on `stream`. */
int cr_kv_set_beam(cr_kv* kv, int first_seq, int num_beams, float length_penalty, int early_stopping, int eos_id, int max_new, void* stream);
/* The group's best finished hypothesis so far: its ids (EOS included; at most `max`) into host memory, *score = its sequences_scores entry, *length = its id count
 * (0 and -1e9 while no hypothesis has finished), *done = the group has stopped.  Returns the ids copied, or < 0.  Synchronises `stream` like cr_kv_generated. */
int cr_kv_beam_result(cr_kv* kv, int first_seq, int64_t* out_host, int max, float* score, int32_t* length, int32_t* done, void* stream);
/* The re-order kernel alone (test entry), on PLAIN sequences: sequence first_seq + j (j < num_beams) takes cache positions [from, length) and the id history of
 * first_seq + src_host[j] (host array of num_beams entries, each 0 .. num_beams - 1), every layer, KV head, K and V, in place.  The sequences hold the same
 * counts of tokens and ids (CR_ERR_ARG otherwise) and belong to no beam group (CR_ERR_STATE: a live group's state is never touched).  Enqueued on `stream`. */
int cr_kv_beam_reorder(cr_kv* kv, int first_seq, int num_beams, const int32_t* src_host, int from, void* stream);
/* Enqueue on `stream` an asynchronous copy of the finished queue into host_out (caller-owned PINNED memory of max >= 1 + 2 n_seqs
 * int32): host_out[0] = sequences pushed since the last cr_kv_reset(kv, -1) (a running count c), host_out[1 + k % n_seqs] = the
 * k-th of them (the ring holds the last n_seqs: a sequence is pushed again only after a reset, so a caller that releases a sequence
 * only after reading its entry never loses one), host_out[1 + n_seqs + s] = stop count of sequence s (0: not stopped).  The copy
 * reflects the work enqueued on `stream` before it: record an event after the call and read host_out once it has completed --
 * nothing synchronises. */
int cr_kv_poll_finished(cr_kv* kv, int32_t* host_out, int max, void* stream);

/* InternLM2ForCausalLM.forward(inputs_embeds=…, use_cache=True) — InternVL/modeling_internlm2.py:1022-1110 —
 * for ONE sequence `seq`, appended at its current length; then the first greedy pick of
 * transformers 4.45.2 GenerationMixin._sample (RepetitionPenaltyLogitsProcessor over the ids generated so far,
 * argmax with first-max-wins), appended to the sequence's generated ids.
 * embeds [S,4096]; last_logits [vocab] fp32 = raw last-row logits before the penalty (may be NULL).
 * Continued prefill: a sequence that already holds n tokens (an earlier prefill, decode steps) takes the S rows at positions n .. n + S - 1 (RoPE and
 * the causal mask count from n; the rows attend over the n cached tokens and themselves) and holds n + S afterwards: prefill(A) then prefill(B) caches
 * what one prefill of A followed by B caches.  EVERY prefill appends one pick to the generated ids (cr_kv_generated): after two prefills the sequence
 * holds two ids, the first made at the end of A, the second at the end of B with the penalty applied over the first; the stop criteria, the sampling
 * step and the scores count both.  A caller that wants one id per prompt calls cr_kv_reset and prefills the whole prompt, as the chat code does.
 * An e4m3 cache refuses a sequence that already holds tokens (CR_ERR_ARG: it keeps no bf16 prefix for the prefill attention to read). */
int cr_llm_prefill(cr_ctx* ctx, cr_kv* kv, int seq, const void* embeds, int S, float penalty, float* last_logits,
                   void* stream);
/* The same for n sequences at once: embeds is the concatenation [sum(lens), 4096] of the prompts in seqs[] order
 * (seqs, lens: host arrays).  The linear layers run over all prompt rows together (better MFMA tile occupancy),
 * attention stays per sequence; every sequence gets exactly the result of its own cr_llm_prefill.
 * last_logits [n,vocab] fp32 (may be NULL). */
int cr_llm_prefill_batch(cr_ctx* ctx, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens,
                         float penalty, float* last_logits, void* stream);
/* Teacher-forced scores: what the model thinks of a text the CALLER brings (a ground truth, a candidate, a correction).  A continued prefill exactly as
 * cr_llm_prefill_batch defines it -- the rows are appended at each sequence's current length, RoPE and the causal mask count from that length, cr_kv_length
 * grows by lens[i], every row's K / V reach the cache -- that makes NO pick: no id is appended, and no stop, sampling, constraint or score state of the
 * sequences is read or changed.  Instead every row r with targets_host[r] = y >= 0 (host array over the concatenated rows, < 0: the row is not scored) is
 * scored by cr_kv_set_logprobs' definition, on the distribution over the id that FOLLOWS row r: with h = the targets of the scored rows of the same sequence
 * that precede r in this call,
 *     z        = the raw fp32 LM-head row of r after the repetition penalty over h (v < 0 ? v * penalty : v / penalty; an id repeated in h is penalised
 *                once: every duplicate sees the original score)
 *     logprob  = z[y] - lse(z);   top_ids / top_lp = the top_n largest entries of z (descending, an exact tie towards the lower id) as id and z - lse
 * -- what a greedy generation that happened to produce the text would have recorded for it.  The usual call holds the rows prompt ++ embed(y[0 .. T-1)) with
 * targets [-1] * (P - 1) ++ y[0 .. T); put the EOS id into y to score the stop as well.  To score over a cache that already holds the WHOLE prompt (L rows),
 * roll it back by one row and feed that row again: cr_kv_truncate(seq, L - 1), then the rows prompt[L - 1] ++ embed(y[0 .. T-1)) with targets y[0 .. T).
 * Outputs (device), one slot per SCORED row in row order: lp [R] fp32, top_ids [R][8] int32 and top_lp [R][8] fp32 (entries top_n..8 hold -1 and -inf; both
 * may be NULL when top_n == 0), logits [R][vocab] fp32 = the raw rows (may be NULL).  The final decoder layer runs on every row; the LM head runs on the scored
 * rows in tiles of 256 with the tiled kernels, so a row's logits do not depend on what it is batched with (they need not equal cr_llm_prefill's last_logits bit
 * for bit: that head may take the weight-streaming kernel); the score kernels (csrc/score.hip) keep csrc/logprobs.hip's summation order, so a row's scores are
 * bit-equal to cr_op_logprobs on the penalised row, within 5e-6 absolute of the float64 log-softmax for |z| <= 32.
 * Checked before anything is enqueued, nothing changes on refusal: CR_ERR_ARG for a sequence out of range or listed twice, lens[i] <= 0, rows that exceed the
 * cache, a call without any scored row, a target >= vocab, top_n outside 0..8, a penalty that is not finite and > 0, an e4m3 cache, or a member of a beam
 * group; CR_ERR_STATE for a sequence that holds generated ids (the penalty history is the call's own: cr_kv_truncate / cr_kv_fork / cr_kv_reset give a
 * sequence without ids).  Enqueued on `stream`.  Added within ABI v13. */
int cr_llm_score_batch(cr_ctx* ctx, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens, const int64_t* targets_host,
                       float penalty, int top_n, float* lp, int32_t* top_ids, float* top_lp, float* logits, void* stream);
/* Grounding: cr_llm_score_batch's pass, which also reports WHERE every scored row looked.  Arguments up to top_lp are cr_llm_score_batch's (there is no
 * logits output); lp may be NULL: a grounding-only call that runs every layer (the cache is what scoring leaves) but no final norm, LM head or score kernel,
 * and top_n must then be 0.  The grounded rows are the scored rows, slot r as above.  spans_host holds (start, end) pairs of absolute cache positions, the
 * call's sequences one after another, span_counts_host [n] how many each sequence has (0..1024).  A span is the half-open key range [start, end); per sequence
 * the spans are sorted by start and do not overlap, a span may be empty, and it may lie anywhere in [0, cr_kv_length + lens[i]) -- so also behind a row, where
 * the causal mask gives it 0.  For a grounded row r at position p, with H = 32 heads:
 *     s_k      = bf16(bf16(q . k) * (1.0f / sqrtf(128)))      the prefill attention's own score arithmetic, the dot product in fp32
 *     P_k      = exp(s_k - m) / sum over k' <= p of exp(s_k' - m)      in fp32, never rounded to bf16
 *     mass[r][b] = 1 / (H * (layer1 - layer0)) * sum over layers layer0 <= l < layer1, heads h and keys k in span b with k <= p of P_k
 * mass is a DEVICE array [R][mass_ld] fp32, mass_ld >= the largest span count; columns from a row's own sequence's count upward are written 0.  What the
 * spans do not get, 1 - sum_b mass[r][b], is the caller's to compute.  A row's mass depends on its own sequence only: the same row alone and in a larger call
 * gives the same bits (no float atomics; every sum has a fixed order).  lp / top_ids / top_lp and the cache are bit for bit cr_llm_score_batch's.
 * Checked before anything is enqueued, nothing changes on refusal: everything cr_llm_score_batch refuses; CR_ERR_ARG for a null mass, spans_host or
 * span_counts_host, a count outside 0..1024, spans that are unsorted, overlapping, reversed or outside [0, cr_kv_length + lens[i]), mass_ld below a count,
 * layer0 < 0, layer1 > llm_layers, layer0 >= layer1, or top_n > 0 with a null lp.  Enqueued on `stream`.  Added within ABI v13. */
int cr_llm_ground_batch(cr_ctx* ctx, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens, const int64_t* targets_host,
                        float penalty, int top_n, float* lp, int32_t* top_ids, float* top_lp, const int32_t* spans_host, const int32_t* span_counts_host,
                        int layer0, int layer1, float* mass, int mass_ld, void* stream);
/* Parity tooling: while `dst` is not NULL, every cr_llm_prefill / cr_llm_prefill_batch also copies rows [row0, row0 + rows) of the
 * residual stream (row index into the concatenated prompt rows) into dst [llm_layers + 1][rows][4096] bf16 (device): slot 0 = the
 * decoder stack's input, slot l + 1 = the output of InternLM2DecoderLayer l (InternVL/modeling_internlm2.py:621-681; what
 * output_hidden_states=True collects at :916-918,965-967, before the final norm).  dst = NULL switches it off. */
int cr_llm_hidden_probe(cr_ctx* ctx, void* dst, int row0, int rows);
/* One greedy step for sequences seqs[0..n) (host array): embed each sequence's last generated id (or
 * force_tokens[i], device int64, when not NULL), run the decoder against the cache, append K/V, apply the
 * penalty, argmax, append the new id.  logits [n,vocab] fp32 raw (may be NULL).  Replaces one iteration of
 * GenerationMixin._sample as driven from InternVL/modeling_internvl_chat.py:1111-1120 with
 * prepare_inputs_for_generation (InternVL/modeling_internlm2.py:1112-1149). */
int cr_llm_decode(cr_ctx* ctx, cr_kv* kv, const int32_t* seqs, int n, const int64_t* force_tokens, float penalty,
                  float* logits, void* stream);
/* One DRAFT-VERIFIED greedy step for sequences seqs[0..n) (host array): sequence i brings k = draft_lens_host[i] (0..7) drafted ids
 * d[0..k) = draft_host[i * draft_stride ..] (host arrays; draft_host may be NULL when every k is 0), a guess at the ids it is about to generate, and takes
 * k + 1 rows of the ONE decode launch: row r is fed the sequence's last generated id (r = 0) or d[r - 1], sits at position cr_kv_length + r (RoPE, cache
 * row) and attends over the cr_kv_length + r + 1 keys up to itself.  Row r's pick p_r is cr_llm_decode's -- the repetition penalty over the generated ids
 * followed by d[0..r), argmax with first-max-wins -- so with a the longest prefix for which p_j == d[j], the ids p_0 .. p_a are exactly what a + 1 calls
 * of cr_llm_decode would have appended, and they are appended, in order, each with the stop check of cr_kv_set_stop at its own count: the first id that
 * stops the sequence is appended and nothing behind it.  The sequence then holds cr_kv_length + (ids appended) tokens; cache rows past that are dead, as
 * after cr_kv_truncate.  EXACT, not approximate: whatever the draft holds, the ids, the stops and the live cache rows are those of plain steps (the decode
 * GEMMs give a row the same bits at 1..64 rows, the attention of a row depends on its own key count only); a wrong draft costs rows, never an id.  With
 * every draft_lens_host[i] == 0 the call computes what cr_llm_decode(seqs, n, NULL, penalty, NULL) computes, bit for bit.
 * The call SYNCHRONISES `stream`, as cr_kv_generated does, and writes the count of ids appended per sequence (1..k + 1) to appended_host[n]; cr_kv_length
 * and the host-side id counts follow it.  That is the price of a variable step: the caller's next window depends on the counts anyway.
 * Checked before anything is enqueued, nothing changes on refusal: CR_ERR_ARG for a sequence out of range or listed twice, k outside 0..7, more than 64
 * rows in all (the step stays inside the decode forms whose bits do not depend on the batch), cr_kv_length + k + 1 > max_tokens, a drafted id outside the
 * vocabulary, or an e4m3 cache (left out: a window's rows are written by the bf16 RoPE + split forms only); CR_ERR_STATE for a sequence without a generated
 * id, one that samples (a sampled pick is a draw, not a comparison), records token scores or has logits constraints (both are per appended id), or belongs
 * to a beam group (its step re-orders the cache).  A history of more than 4096 ids under a penalty is handled as cr_llm_decode handles it (the pick reads
 * an untouched copy of the rows).  Added within ABI v13. */
int cr_llm_decode_draft(cr_ctx* ctx, cr_kv* kv, const int32_t* seqs, int n, const int64_t* draft_host, const int32_t* draft_lens_host,
                        int draft_stride, float penalty, int32_t* appended_host, void* stream);

/* fp8 weight path (BASELINE.json configs[4]; the reference itself has no fp8 -- an option, OFF by default, the headline stays
 * bf16).  enable != 0: every linear weight of the language model the batched decode streams (wqkv, wo, w1|w3, w2 of each
 * layer, the LM head) gets an e4m3 (OCP e4m3fn) copy with one fp32 scale per output row, scale = max|w| / 448, built on the
 * device on first use; cr_llm_decode with <= 64 sequences then reads those (half the HBM bytes), dequantising in registers
 * (exact: e4m3 is a subset of bf16), multiplying in the same bf16 MFMA with fp32 accumulation and applying the row scale to
 * the fp32 sum.  Activations, KV cache, prefill and everything visual stay bf16.  enable == 0 switches back (copies kept).
 * Call after cr_finalize; re-run it after reloading weights. */
int cr_enable_fp8_decode(cr_ctx* ctx, int enable, void* stream);
/* fp8 on the matrix cores (same standing: an option, OFF by default; a THROUGHPUT option -- e4m3 keeps 3 mantissa bits, every such
 * linear adds ~5 % of relative noise to its output, and whether the transcription survives that is what evaluate.py --compare_fp8 measures
 * on a real checkpoint; nothing here is claimed to preserve the reference's tokens).
 * enable = 1: the linears whose input is a norm's output -- QKV and fc1 of every ViT layer, mlp1's first linear, wqkv and w1|w3 of every
 *   LLM layer in PREFILL -- get the e4m3 copy + row scale above, the norm kernel in front of each writes the normalised row as e4m3 with
 *   one fp32 scale per row (max|y| / 448 over the bf16-rounded row) instead of bf16, and the 256x256 tiled kernel multiplies e4m3 x e4m3
 *   with v_mfma_f32_16x16x128_f8f6f4 (fp32 accumulation, twice the bf16 rate), applying ascale[m] * wscale[n] to the finished sum before
 *   the bias and the rest of the epilogue.  proj / fc2 / wo / w2, attention, the residual stream, the KV cache and decode stay bf16.
 * enable = 2: additionally the linears whose input no norm produces: ViT fc2 (fc1's epilogue writes its GELU output as e4m3 rows under a
 *   LayerNorm-derived bound) and the LLM's wo / w2 in prefill (one quantiser pass over their input each).
 * enable = 0 switches back (copies kept).  Call after cr_finalize; re-run it after reloading weights. */
int cr_enable_fp8_mfma(cr_ctx* ctx, int enable, void* stream);

/* ---- measurement ------------------------------------------------------------------------------- */
/* While enabled, every launch of the dense-GEMM kernel made by the stage entry points is bracketed by a pair of
 * HIP events on the launch stream.  cr_profile_read synchronises and returns, for the compute-bound class
 * (M >= 1024 rows) in out[0..3] = {launches, summed kernel ms, summed algorithmic FLOPs (2*M*N*K), algorithmic bytes} and for the
 * weight-streaming class (M < 1024) in out[4..7] = {launches, ms, FLOPs, algorithmic bytes (W + A + C)}; then clears. */
/* enable: 0 off, 1 every GEMM launch, 2 only the compute-bound class (the decode steps' many short launches then
 * carry no events). */
int cr_profile(cr_ctx* ctx, int enable);
int cr_profile_read(cr_ctx* ctx, double* out8);
/* Bookkeeping of the above since cr_create: out[0] = launches bracketed, out[1] = launches accounted for (retired into
 * the sums or still pending), out[2] = launches whose events could not be created or read (0 in a healthy run),
 * out[3] = most records ever pending at once.  Records are retired as their events complete; there is no cap. */
int cr_profile_stats(cr_ctx* ctx, int64_t* out4);

/* ---- ordering front end ------------------------------------------------------------- */
/* OrderFormer.model forward -- models/model.py:206-233, called from predict :458-461.
 * boxes [B][L][4] bf16 (L <= 64; the reference pads every page to max_nums = 50 rows) -> scores [B][L] fp32
 * (= the bf16 decoder output).  Weights: the reference's `Transformer` state_dict keys under "orderformer."
 * (embedding.*, transformer_encoder.layers.N.*, decoder.*), loaded with cr_load_weight. */
int cr_orderformer(cr_ctx* ctx, const void* boxes, int B, int L, float* scores, void* stream);

/* ---- single operators (unit-parity tests and profiling) --------------------------------------- */
/* C = epi(A[M,K] . W[N,K]^T); epi: 0 store, 1 gelu, 2 layerscale+residual, 3 residual, 4 swiglu, 5 patch, 6 f32,
 * 7 decode partial sums (M <= 64, no bias: C = fp32 [S][M][N], S <= 8 K-slices summed by the consumer),
 * 8 row arg-max partials (cosine VQ: C = uint64 [M][ldc], one per row and 64-column block: bits of the bf16-rounded maximum in the
 *   high word, its first column in the low word; M > 64 tile kernels only).
 * Bits 8..15 of epi pin a kernel for the unit tests: 0 dispatcher's choice, 1 128x128 tiles, 2 256x256 persistent,
 * 3 weight-streaming (M <= 64), 5 / 6 the 256x256 kernel with its 16- / 32-MFMA-slot schedule (the same sums: the same bits);
 * a pinned kernel that cannot take the shape returns CR_ERR_ARG.
 * Bits 18-19 (M <= 64, bf16 weights, the weight-streaming kernels): W is cr_op_decode_swizzle's copy of the weight (ldw ignored) -- 1: plain 16-row
 * tiles (its which = 1..4), 2: wqkv's RoPE tile order (which = 0; epi 7 only: the K-slices still land in their nn.Linear columns).  The same bits as
 * from the nn.Linear layout. */
int cr_op_gemm(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
               const void* bias, const void* scale, const void* res, int64_t ldr, int M, int N, int K, int group,
               void* stream);
/* With bit 16 of epi set, W is e4m3 bytes [N][ldw] and `scale` is float[N] (one per row): C = epi((A . W^T) * scale); M <= 64. */
/* With bits 16 AND 17 set, A is e4m3 bytes [M][lda] too and `res` is float[M] (one scale per row of A):
 * C = epi((A . W^T) * res[m] * scale[n] + bias); the 256x256 kernel's e4m3 instance: K % 256 == 0, N % 64 == 0, epi 0 | 1 | 4 | 6. */
/* rows of a bf16 matrix -> e4m3 bytes q [N][K] + scale [N] (max|w| / 448 per row), as cr_enable_fp8_decode builds them */
int cr_op_quantize_fp8(const void* w, int64_t ldw, int N, int K, void* q, float* scale, void* stream);
int cr_op_layernorm(const void* in, void* out, const void* gamma, const void* beta, int64_t rows, int n, float eps,
                    int pixel_shuffle, void* stream);
/* cr_op_layernorm's plain rows (n = 1024 | 4096) with the output-row regrouping the resampler uses to write cat(norm_media(x), norm_learns(learns)) in place
 * (test entry; cr_resample fills its launches through the same function, regroup_norm_params, and drives the same kernel): input row r lands in output row
 * (r / in_group) * out_group + out_off + r % in_group; out_group = 0: output row = input row, as cr_op_layernorm.  CR_ERR_ARG for out_group > 0 with
 * in_group <= 0 or out_off + in_group > out_group (rows of two groups would overlap).  out holds ceil(rows / in_group) * out_group rows at the most; rows of
 * out that no input row maps to are not written.  Added within ABI v13. */
int cr_op_layernorm_regroup(const void* in, void* out, const void* gamma, const void* beta, int64_t rows, int n, float eps, int in_group, int out_group,
                            int out_off, void* stream);
int cr_op_rmsnorm(const void* in, void* out, const void* gamma, int64_t rows, int n, float eps, void* stream);
/* the same norms with the fp8 output cr_enable_fp8_mfma uses: beta == NULL selects RMSNorm (n = 4096), otherwise LayerNorm
 * (n = 1024 | 4096); out8 = e4m3 [rows][n], out_scale = float[rows] */
int cr_op_norm_fp8(const void* in, const void* gamma, const void* beta, int64_t rows, int n, float eps, void* out8, float* out_scale,
                   float* next_scale, const float* next_bound, void* stream);
/* next_scale / next_bound (both or neither): next_scale[row] = (1.13 * ||y_row||_2 * next_bound[0] + next_bound[1]) / 448 -- an upper bound
 * of what the next linear (largest weight-row norm next_bound[0], largest |bias| next_bound[1], device floats) can make of this row,
 * used as the e4m3 scale of THAT linear's output row by cr_op_gemm_q8 / the ViT's fc1 under cr_enable_fp8_mfma. */
/* C8 = e4m3(bf16(gelu(bf16((A8 . W8^T) * ascale[m] * wscale[n] + bias))) / c8scale[m]), bytes [M][N]: fc1's output as fc2's operand */
int cr_op_gemm_q8(const void* a8, const float* ascale, const void* w8, const float* wscale, const void* bias, const float* c8scale,
                  void* c8, int M, int N, int K, void* stream);
/* One small-batch decode GEMM with its neighbours folded in (gemm_decode.hip; M <= 8 rows, InternLM2.5-7B shapes): which = 0 wqkv
 * [RMSNorm(xres) -> GEMM -> RoPE + split: q_out rows, K / V rows into kc / vc at (seqs[m], lens[seqs[m]])], 1 wo [X -> GEMM -> xio += ],
 * 2 w1|w3 [RMSNorm(xres) -> GEMM -> SwiGLU -> C], 3 w2 [as 1], 4 LM head [RMSNorm(xres) -> GEMM -> fp32 C].  Replaces, per decode step of
 * InternLM2DecoderLayer.forward (modeling_internlm2.py:621-681): the norm / linear / rotary / residual statements around each linear.
 * Test and tuning entry point (cr_llm_decode drives the same launcher).  flags: bit 8 (256) = W is in the decode layout cr_op_decode_swizzle
 * writes (ldw ignored); other bits 0. */
int cr_op_decode_gemm(int which, int flags, const void* W, int64_t ldw, int M, int N, int K, const void* X, int64_t ldx, const void* xres,
                      const void* gamma, float eps, void* xio, void* C, int64_t ldc, const void* cosT, const void* sinT, void* q_out, void* kc,
                      void* vc, const int32_t* seqs, const int32_t* lens, int max_tokens, void* stream);
/* The decode layout of a weight for cr_op_decode_gemm's `which`: one 1 KiB block per (16-row tile, 32-deep k-step), lane l's eight elements at l * 16
 * bytes, in the kernel's own tile order (which = 0: RoPE tiles of 8 + 8 rows) -- a wave's load is one contiguous KiB instead of 16 rows x 64 bytes.
 * dst: ceil(N / 16) * 16 * K bf16.  cr_finalize keeps such a copy of every LLM linear (+15 GB on InternLM2.5-7B) for decode batches of <= 8 rows. */
int cr_op_decode_swizzle(int which, const void* W, int64_t ldw, int N, int K, void* dst, void* stream);
/* The sampling pick of cr_kv_set_sampling alone (test / tuning entry; the prefill and decode launch the same kernel): logits [n][vocab] fp32 (not
 * modified), history [n][hist_cap] int64 with hist_len[n] ids per row (hist_cap <= 4096; history may be NULL when hist_cap == 0) for the penalty,
 * per row temperature / top_k / top_p / seed / step as above (temperature <= 0: the greedy pick).  out_ids[n] = the id, out_kept[n] = the size of
 * the kept set (0 for a greedy row).  All pointers are DEVICE arrays.  ABI v12. */
int cr_op_sample(cr_ctx* ctx, const float* logits, int n, int vocab, const int64_t* history, int hist_cap, const int32_t* hist_len, float penalty,
                 const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seed, const int32_t* step, int64_t* out_ids,
                 int32_t* out_kept, void* stream);
/* The constraint kernel of cr_kv_set_constraints alone (test / tuning entry; the prefill and decode launch the same kernel): logits [n][vocab] fp32, MODIFIED
 * in place (banned ids become -inf, every other value is untouched); row r reads the history of s = seqs[r] (seqs: DEVICE int32 [n], NULL: s = r): history
 * [.][hist_cap] int64 with hist_len[s] ids (DEVICE arrays; counts above hist_cap are read as hist_cap; history may be NULL when hist_cap == 0).  `c` (host, not
 * NULL) constrains every row and is checked as cr_kv_set_constraints checks it.  Synchronises `stream`.  Added within ABI v13. */
int cr_op_constrain(const cr_constraints* c, float* logits, int n, int vocab, const int32_t* seqs, const int64_t* history, int hist_cap, const int32_t* hist_len,
                    void* stream);
/* The score kernels of cr_kv_set_logprobs alone (test entry; the prefill and decode launch the same kernels): logits [n][vocab] fp32 = the rows z
 * (not modified), ids [n] int64 = the id scored in each row; lp [n], top_ids [n][8], top_lp [n][8] as above with top_n alternatives (1..8, CR_ERR_ARG
 * otherwise; vocab >= 8, n <= 65535).  All pointers are DEVICE arrays.  Synchronises `stream`.  Added within ABI v13. */
int cr_op_logprobs(const float* logits, int n, int vocab, const int64_t* ids, int top_n, float* lp, int32_t* top_ids, float* top_lp, void* stream);
/* The score kernels of cr_llm_score_batch alone (test entry; the stage launches the same three kernels): logits [n][vocab] fp32 = raw rows (DEVICE, not
 * modified); targets_host [n] int64 = the id scored in each row, row_seq_host [n] int32 = which history the row belongs to (0 .. n - 1), hist_index_host [n]
 * int32 = its ordinal j in that history (HOST arrays): row r is penalised at the targets of the rows of the same history with a smaller ordinal.  lp [n],
 * top_ids [n][8], top_lp [n][8] (DEVICE) as above with top_n alternatives (0..8; top_* may be NULL when top_n == 0).  vocab >= 8, n <= 65535, every target
 * inside the vocabulary, penalty finite and > 0 (CR_ERR_ARG otherwise).  Synchronises `stream`.  Added within ABI v13. */
int cr_op_score_rows(const float* logits, int n, int vocab, const int64_t* targets_host, const int32_t* row_seq_host, const int32_t* hist_index_host,
                     float penalty, int top_n, float* lp, int32_t* top_ids, float* top_lp, void* stream);
/* One beam-search step of cr_kv_set_beam alone (test entry; the prefill and decode launch the same three kernels): logits [n][vocab] fp32 (OVERWRITTEN with the
 * penalised log-probabilities), history [n][hist_cap] int64 with hist_len[n] ids per row (both updated: re-ordered, the new id appended), group[n] = the first row
 * of the row's beam group (every row belongs to one; a group's rows are consecutive, in beam order), fin_ids [n][hist_cap] int64 = ids of the finished slots
 * (row = first row + fin_phys), state [n][64] four-byte words = a group's state at its first row:
 *   0 num_beams, 1 eos_id, 2 max_new, 3 early_stopping, 4 g, 5 done, 6 skip, 7 heuristic still unsatisfied (start: 1), 8 finished slots in use, 9 prompt length,
 *   10 length_penalty (float), 16..23 running scores (float; start 0, -1e9, ...), 24..31 finished scores (float; start -1e9), 32..39 their lengths,
 *   40..47 their rows of fin_ids, 48..55 source beam of each next beam, 56..63 its new id.
 * All pointers are DEVICE arrays.  vocab >= 16, n <= 65535.  Synchronises `stream`. */
int cr_op_beam_step(float* logits, int n, int vocab, int64_t* history, int hist_cap, int32_t* hist_len, float penalty, const int32_t* group, void* state,
                    int64_t* fin_ids, void* stream);
/* q/k/v/o addressed as base + b*bs + row*rs + head*hs (elements) */
int cr_op_attention(const void* q, const void* k, const void* v, void* o, const int64_t* strides12, int B, int H,
                    int Sq, int Sk, int head_dim, int kv_group, int causal, int q_pos0, float q_prescale, float s_div,
                    void* stream);
/* The prefill attention's segment launch alone (test entry; cr_llm_prefill_batch fills its launch through the same function and drives the same kernel,
 * flash_attn_kernel<128, causal, divisor>): q / o [rows][H][128] bf16, kc / vc [n_slots][H / kv_group][max_tokens][128] bf16 caches that already hold every
 * segment's keys / values, seg = n x {first row, rows S, position of the first row pos0, cache slot} int32 (DEVICE array), Sq = the longest segment's rows
 * (the grid).  Row r of a segment attends causally over cache positions 0 .. pos0 + r of its slot: scores bf16 -> / s_div -> bf16, fp32 softmax, bf16
 * probabilities (modeling_internlm2.py:393-410).  Only rows first row .. first row + S - 1 of o are written and only positions < pos0 + S of the slot are
 * read; the caller guarantees first row + S <= rows, pos0 + S <= max_tokens and slot < n_slots (the entry cannot see the device array).  Added within ABI v13. */
int cr_op_attention_segments(const void* q, const void* kc, const void* vc, void* o, const int32_t* seg, int n, int Sq, int H, int kv_group, int max_tokens,
                             float s_div, void* stream);
/* The span-mass kernels of cr_llm_ground_batch alone, on ONE layer (test entry; the stage launches the same two kernels): q [q_rows][H][128] bf16 roped
 * queries, kc [n_slots][H / kv_group][max_tokens][128] bf16 K cache that already holds every segment's keys (both DEVICE); seg_host = n x {first row, rows S,
 * position of the first row pos0, cache slot} (HOST), grounded_host [q_rows] bytes (HOST): a segment's rows with a non-zero byte are its grounded rows;
 * spans_host / span_counts_host as cr_llm_ground_batch (limit pos0 + S); mass [R][mass_ld] fp32 (DEVICE), R = the grounded rows in segment then row order,
 * receives the mean over the H heads.  kv_group must be 4 and H a multiple of it.  CR_ERR_ARG for a null pointer, a segment outside q / the cache, segments
 * that share rows of q or a slot, no grounded row, bad spans or mass_ld below a count.  Synchronises `stream`.  Added within ABI v13. */
int cr_op_span_mass(const void* q, int q_rows, const void* kc, int n_slots, int max_tokens, int H, int kv_group, const int32_t* seg_host, int n,
                    const unsigned char* grounded_host, const int32_t* spans_host, const int32_t* span_counts_host, float s_div, float* mass, int mass_ld,
                    void* stream);
/* PerceiverAttention's softmax(q k^T) v alone (test entry; cr_resample makes its launch through the same function, launch_perceiver_attn, and drives the same
 * kernels): T tiles x 8 heads x 3 queries x 259 keys x 64 dims.  q [T * 3][512] bf16 (head h in columns 64 h .. 64 h + 63), kv [T * 259][1024] bf16 (a tile's
 * 256 media rows then its 3 latent rows; K in columns 0..511, V in 512..1023), out [T * 3][512] bf16.  Rounding points of perceiver_resampler.py:43-51:
 * q * 0.125 (exact), scores -> bf16, scores - row maximum -> bf16, fp32 softmax -> bf16, probabilities . v accumulated in fp32 -> bf16.  which = 0: the
 * production kernel, 1: round 1's kernel (CR_PERCEIVER_ATTN_V1=1), bit-identical by construction.  Reads nothing outside q and kv.  CR_ERR_ARG for a null
 * pointer, T <= 0 or another `which`.  Added within ABI v13. */
int cr_op_perceiver_attention(int which, const void* q, const void* kv, void* out, int T, void* stream);

/* Batched decode attention alone (test / tuning entry; cr_llm_decode drives the same launcher): row b = one new token of cache slot seqs[b], its H_kv x 4 query heads x 128 at
 * q + b * 4096 (InternLM2's GQA layout: the 4 query heads of KV head h at (4 h .. 4 h + 3) * 128), keys / values [n_slots][8][max_tokens][128] bf16, lens[slot] + 1 keys per row
 * (the new token's K / V row is already in the cache), scores bf16 -> / s_div -> bf16, fp32 softmax, bf16 probabilities (modeling_internlm2.py:393-410); splits of 256 keys, partials in
 * `scratch` (cr_op_decode_attention_scratch_floats(B, max_keys) floats), merged in index order.  which = 0: the dispatcher's choice (attention_decode.hip), 1: the matrix-core split
 * kernel of attention.hip.  seqs / lens are DEVICE arrays.  ABI v10. */
int64_t cr_op_decode_attention_scratch_floats(int B, int max_keys);
int cr_op_decode_attention(int which, const void* q, const void* kc, const void* vc, int max_tokens, const int32_t* seqs, const int32_t* lens, int B, int max_keys,
                           float s_div, float* scratch, void* out, void* stream);
/* The same with shared prompts (test entry; cr_llm_decode drives the same launcher): row b reads positions [0, pfx_len[b]) from slot pfx_src[b] and the rest from
 * its own slot seqs[b]; pfx_src[b] < 0: all its own.  pfx_src / pfx_len are HOST arrays of B ints (a row's share, not a slot's), pfx_len a multiple of 256 and
 * <= lens[seqs[b]]; seqs / lens are DEVICE arrays as above.  Rows with the same (pfx_src, pfx_len) -- and the row whose slot IS that source -- are grouped, in chunks
 * of 8; the rows of a sharer's slot below pfx_len are never read.  Bit-equal to cr_op_decode_attention on a cache that holds copies.  Synchronises `stream`.
 * CR_ERR_ARG for a pfx_len that is no multiple of 256 or reaches max_keys.  Added within ABI v13. */
int cr_op_decode_attention_shared(const void* q, const void* kc, const void* vc, int max_tokens, const int32_t* seqs, const int32_t* lens, const int32_t* pfx_src,
                                  const int32_t* pfx_len, int B, int max_keys, float s_div, float* scratch, void* out, void* stream);
/* The same over an e4m3 cache (the reader cr_llm_decode uses on a CR_KV_E4M3 cache): kc / vc [n_slots][8][max_tokens][128] e4m3 bytes, ks / vs
 * [n_slots][8][max_tokens] fp32 row scales, arithmetic as under cr_kv_alloc_ex.  which = 0 only (1, the matrix-core kernel, reads bf16: CR_ERR_ARG).  ABI v13. */
int cr_op_decode_attention_e4m3(int which, const void* q, const void* kc, const void* vc, const float* ks, const float* vs, int max_tokens, const int32_t* seqs,
                                const int32_t* lens, int B, int max_keys, float s_div, float* scratch, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CALLIREADER_HIP_H */

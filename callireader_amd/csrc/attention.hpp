#pragma once
#include <vector>

#include "common.hpp"

// Strides are in elements.  Q/K/V/O are addressed as base + b*bs + row*rs + head*hs + d.
struct AttnParams {
    const bf16* Q; const bf16* K; const bf16* V; bf16* O;
    int64_t q_bs, q_rs, q_hs;
    int64_t k_bs, k_rs, k_hs;
    int64_t v_bs, v_rs, v_hs;
    int64_t o_bs, o_rs, o_hs;
    int B, H, Sq, Sk;
    int kv_group;        // query heads per kv head (GQA): kv head = head / kv_group
    int q_pos0;          // causal: absolute position of query row 0 (keys start at position 0)
    float q_prescale;    // multiply q in bf16 before Q.K^T (ViT: 64^-0.5, exact); 1 = off
    float s_div;         // divide bf16-rounded scores (LLM: sqrt(128)); 1 = off
    // batched decode over a KV cache: batch b reads cache slot seq_map[b] (or b) holding sk_arr[slot] + sk_add keys
    const int32_t* seq_map;
    const int32_t* sk_arr;
    int sk_add;
    // split-KV (decode): workgroup x = split of SPLIT_TILES key tiles; partial (m, l) and un-normalised O go to
    // part_ml [B][H][nsplit][Sq][2] / part_o [B][H][nsplit][Sq][D] (fp32), merged by launch_attn_combine
    int nsplit;
    float* part_ml;
    float* part_o;
    // causal prefill of several pages in ONE launch: batch b is segment seg[4b..4b+3] = {first row, rows, position of the first
    // row, cache slot}: Q / O rows start at `first row` (q_bs / o_bs unused), keys = position + rows, Sq = the longest segment
    const int32_t* seg;
    bool force_matrix_core;   // decode: keep the matrix-core split kernel even where attention_decode.hip's streaming kernel qualifies (cr_op_decode_attention which = 1: A/B)
    // decode with RoPE + split FOLDED IN (attention_decode.hip, 9..64-row batches): instead of reading Q and finding the new token's K / V row in the cache, the
    // kernel sums wqkv's K-slice partial sums [qkv_splits][B][qkv_ld] fp32 itself (slice order, rounded once), rotates q and k (rope_split_kernel's arithmetic) and
    // the workgroup whose split holds the new position writes the K / V row to the cache.  Row layout of qkv: [H groups][4 q | k | v][128].
    const float* qkv_part;
    int qkv_splits;
    int64_t qkv_ld;
    const bf16* rope_cos;     // [max_pos][128]
    const bf16* rope_sin;
    // decode over an e4m3 cache (cr_kv_alloc_ex CR_KV_E4M3; K / V unused): K8 / V8 bytes addressed with the k_* / v_* strides above (one byte per element),
    // one fp32 scale per cached row at k_scale / v_scale + slot * s_bs + head * s_hs + key.  Only attention_decode.hip's decode_attn8_kernel reads it.
    const unsigned char* K8;
    const unsigned char* V8;
    const float* k_scale;
    const float* v_scale;
    int64_t s_bs, s_hs;
    // decode with several consecutive positions of one sequence as rows (cr_llm_decode_draft), may be NULL: batch b holds sk_arr[slot] + sk_add + sk_off[b] keys.
    // The streaming bf16 kernel and the matrix-core split kernel take it (instances of their own: a launch without it runs the code it always ran); the folded
    // form and the e4m3 kernel do not (decode_attn_fold_supported / decode_attn8_supported are false)
    const int32_t* sk_off;
    // decode with a shared prompt (cr_kv_fork_shared; attention_decode.hip), share_n = 0: none, and the launch is the one it always was.  share_chunks (device) =
    // share_n chunks of ATTN_SHARE_CHUNK_INTS ints {source slot, shared splits, rows, 0, the rows' batch indices[8]}: one workgroup of the group form loads a split
    // of the source slot once and runs every row of the chunk over it.  share_skip (device) [B]: the splits of batch b that the group form writes (0: none); the
    // per-row form returns from them without writing.  share_splits = the most shared splits of any chunk.  attn_share_table builds all of it.
    const int32_t* share_skip;
    const int32_t* share_chunks;
    int share_n, share_splits;
};

constexpr int ATTN_SHARE_ROWS = 8;                              // rows per chunk of the group form
constexpr int ATTN_SHARE_CHUNK_INTS = 4 + ATTN_SHARE_ROWS;
// The share table of one decode launch, built on the host: row b reads cache slot seqs[b], whose positions [0, pfx_len[b]) are those of slot pfx_src[b]
// (pfx_src[b] < 0: its own; pfx_len a multiple of 256).  Rows with equal (pfx_src, pfx_len) form a group, the source's own row joins when it is in the launch,
// and a group is cut into chunks of ATTN_SHARE_ROWS.  table = [B] skips, then the chunks.  Returns the number of chunks (0: no row shares, table left empty),
// *max_splits = the most shared splits of any chunk.  Grouping is a matter of speed only: a row's partials are the same whatever it is grouped with.
int attn_share_table(const int32_t* seqs, const int32_t* pfx_src, const int32_t* pfx_len, int B, std::vector<int32_t>& table, int* max_splits);

bool decode_attn_fold_supported(const AttnParams& p, int head_dim);
// e4m3 caches: false when the process runs with CR_DECODE_ATTN=0 (the matrix-core split kernel reads bf16 only); launch_flash_attn_split then refuses them
bool decode_attn8_available();
bool decode_attn8_supported(const AttnParams& p, int head_dim);

// The segment launch of the causal d = 128 kernel (AttnParams::seg above), filled in ONE place for the LLM stage's prefill (llm.hip, prefill_attn_params) and for
// the test entry cr_op_attention_segments (api.hip): q / o rows [row][H][128], K / V [slot][H / kv_group][T][128], bf16-rounded scores divided by s_div.
inline AttnParams segment_attn_params(const bf16* k, const bf16* v, int T, const bf16* q, bf16* o, int H, int kv_group, int n_segs, const int32_t* seg, int Sq,
                                      float s_div) {
    constexpr int HD = 128;
    AttnParams ap{};
    ap.K = k; ap.V = v; ap.Q = q; ap.O = o;
    ap.k_bs = ap.v_bs = (int64_t)(H / kv_group) * T * HD; ap.k_rs = ap.v_rs = HD; ap.k_hs = ap.v_hs = (int64_t)T * HD;
    ap.q_prescale = 1.0f; ap.s_div = s_div;
    ap.q_bs = 0; ap.q_rs = (int64_t)H * HD; ap.q_hs = HD; ap.o_bs = 0; ap.o_rs = (int64_t)H * HD; ap.o_hs = HD;
    ap.H = H; ap.kv_group = kv_group; ap.B = n_segs; ap.seg = seg; ap.Sq = Sq;
    return ap;
}

constexpr int ATTN_SPLIT_TILES = 4;     // 256 keys per split: depends only on the row's own key count

int launch_flash_attn(const AttnParams& p, int head_dim, bool causal, hipStream_t stream);
// decode: Sq <= 32 query rows per (batch, head), non-causal over each sequence's own keys, split over the keys
int launch_flash_attn_split(const AttnParams& p, int head_dim, hipStream_t stream);
size_t attn_split_ws_floats(int B, int H, int Sq, int nsplit, int head_dim);
// attention_decode.hip: the split half of launch_flash_attn_split as a streaming vector-pipe kernel (d = 128, 4 query rows per (batch, head): InternLM2's GQA
// group); launch_flash_attn_split takes it by itself when the shape qualifies (CR_DECODE_ATTN=0: the matrix-core split kernel)
bool decode_attn_supported(const AttnParams& p, int head_dim);
int launch_decode_attn(const AttnParams& p, hipStream_t stream);
// attention_decode_group.hip: the shared splits of a launch with p.share_n > 0 chunks (launch_decode_attn calls it, then the per-row form for everything else)
int launch_decode_attn_group(const AttnParams& p, hipStream_t stream);

// ViT layout (S = 1 + 128 n tokens, d = 64, no mask): attention_vit.hip.  launch_flash_attn takes this path by itself when
// p.part_ml points at vit_attn_ws_floats(B, H, S) floats of scratch (the CLS query's partials) and the shape qualifies.
bool vit_attn_supported(const AttnParams& p, int head_dim, bool causal);
size_t vit_attn_ws_floats(int B, int H, int S);
int launch_vit_attn(const AttnParams& p, hipStream_t stream);

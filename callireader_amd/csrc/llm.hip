// Language-model stage: InternLM2.5-7B prefill + batched greedy decode over a pre-allocated KV cache.
//   reference: InternVL/modeling_internlm2.py:129-143 (RMSNorm), :233-247 (RoPE), :250-264 (SwiGLU),
//              :341-426 (attention), :621-681 (layer), :854-984 (model), :1022-1110 (LM head),
//              :1112-1149 (prepare_inputs_for_generation); greedy loop = transformers 4.45.2 _sample.
//
// Per layer: RMSNorm -> GEMM wqkv -> RoPE + split (q to a dense buffer, k/v straight into the cache)
//            -> flash attention (causal GQA in prefill; 4 heads of a KV group as the "rows" in decode)
//            -> GEMM wo (+x in place) -> RMSNorm -> GEMM w1|w3 with SwiGLU epilogue -> GEMM w2 (+x in place).
// Decode (<= 64 rows): wqkv / wo / w2 leave fp32 K-slices that RoPE-split and a fused residual-add + RMSNorm sum up.
//
// This file holds the model: the kernels, the two layer loops and the entry points cr_llm_prefill_batch / cr_llm_score_batch / cr_llm_decode / cr_llm_decode_draft.  The weights come
// resolved (weights.hpp: LlmWeights; weight preparation and every tensor name are in weights.hip).  The cache object (struct cr_kv, every cr_kv_* entry point) is
// kv.hpp / kv.hip; what follows the LM head (the picks, scores, constraints, the beam step) is pick.hip.
#include <float.h>

#include <algorithm>
#include <vector>

#include "attention.hpp"
#include "decode.hpp"
#include "draft.hpp"
#include "ground.hpp"
#include "kv.hpp"
#include "logprobs.hpp"
#include "norm.hpp"
#include "score.hpp"
#include "weights.hpp"

namespace {

// x[i] = tok_embeddings[id_i]; id_i = force[i] or the last generated id of seq_i
// OFF (a draft window's rows, cr_llm_decode_draft): row i is fed the id row_off[i] slots behind that one -- the drafted ids that draft.hip staged there
template <bool OFF = false>
__global__ __launch_bounds__(256) void embed_rows_kernel(const bf16* __restrict__ table, const int64_t* __restrict__ force,
                                                         const int32_t* __restrict__ seqs, const int64_t* __restrict__ gen,
                                                         const int32_t* __restrict__ ngen, int gen_cap, bf16* __restrict__ x,
                                                         const int32_t* __restrict__ row_off = nullptr) {
    const int i = blockIdx.x;
    int64_t id;
    if (force) id = force[i];
    else { const int s = seqs[i]; id = gen[(int64_t)s * gen_cap + ngen[s] - 1 + (OFF ? row_off[i] : 0)]; }
    const bf16x8* src = (const bf16x8*)(table + id * D);
    bf16x8* dst = (bf16x8*)(x + (int64_t)i * D);
    dst[threadIdx.x] = src[threadIdx.x];
    dst[threadIdx.x + 256] = src[threadIdx.x + 256];
}

// splice: src_row[s] >= 0 -> table row; -1-r -> vit row r; -(1<<30)-r -> ref row r
__global__ __launch_bounds__(1024) void splice_index_kernel(const int64_t* __restrict__ ids, int S, int64_t img_id, int64_t ref_id,
                                                            int has_vit, int has_ref, int32_t* __restrict__ src_row,
                                                            int32_t* __restrict__ counts) {
    // one workgroup; running counts carried across chunks of 1024 ids
    __shared__ int s_img[1024], s_ref[1024];
    __shared__ int base_img, base_ref;
    const int tid = threadIdx.x;
    if (tid == 0) { base_img = 0; base_ref = 0; }
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += 1024) {
        const int s = s0 + tid;
        const int64_t id = s < S ? ids[s] : -1;
        const int is_img = (has_vit && id == img_id) ? 1 : 0;
        const int is_ref = (has_vit && has_ref && id == ref_id) ? 1 : 0;
        s_img[tid] = is_img; s_ref[tid] = is_ref;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int a = tid >= o ? s_img[tid - o] : 0, b = tid >= o ? s_ref[tid - o] : 0;
            __syncthreads();
            s_img[tid] += a; s_ref[tid] += b;
            __syncthreads();
        }
        if (s < S) {
            int v = (int)id;
            if (is_img) v = -1 - (base_img + s_img[tid] - 1);
            else if (is_ref) v = -(1 << 30) - (base_ref + s_ref[tid] - 1);
            src_row[s] = v;
        }
        __syncthreads();
        if (tid == 1023) { base_img += s_img[1023]; base_ref += s_ref[1023]; }
        __syncthreads();
    }
    if (tid == 0) { counts[0] = base_img; counts[1] = base_ref; }
}

__global__ __launch_bounds__(256) void splice_rows_kernel(const bf16* __restrict__ table, const bf16* __restrict__ vit,
                                                          const bf16* __restrict__ ref, const int32_t* __restrict__ src_row,
                                                          int n_vit, int n_ref, bf16* __restrict__ out) {
    const int s = blockIdx.x;
    const int v = src_row[s];
    const bf16* src;
    if (v >= 0) src = table + (int64_t)v * D;
    else if (v > -(1 << 30)) { const int r = -1 - v; if (r >= n_vit) return; src = vit + (int64_t)r * D; }
    else { const int r = -(1 << 30) - v; if (r >= n_ref) return; src = ref + (int64_t)r * D; }
    const bf16x8* sp = (const bf16x8*)src;
    bf16x8* dp = (bf16x8*)(out + (int64_t)s * D);
    dp[threadIdx.x] = sp[threadIdx.x];
    dp[threadIdx.x + 256] = sp[threadIdx.x + 256];
}

// dst[i] = src[idx[i]] (GATHER) or dst[idx[i]] = src[i]: rows of 4096 bf16 (the last prompt row of every page around the final layer's row-wise tail)
template <bool GATHER>
__global__ __launch_bounds__(256) void move_rows_kernel(const bf16* __restrict__ src, const int32_t* __restrict__ idx, bf16* __restrict__ dst) {
    const int i = blockIdx.x;
    const int64_t r = idx[i];
    const bf16x8* sp = (const bf16x8*)(src + (GATHER ? r : (int64_t)i) * D);
    bf16x8* dp = (bf16x8*)(dst + (GATHER ? (int64_t)i : r) * D);
    dp[threadIdx.x] = sp[threadIdx.x];
    dp[threadIdx.x + 256] = sp[threadIdx.x + 256];
}

// maximum over the 16 lanes of a DPP row, left in every lane
__device__ __forceinline__ float row_max16(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, true)));      // row_ror:8
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, true)));      // row_ror:4
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, true)));      // row_ror:2
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, true)));      // row_ror:1
    return v;
}

// RoPE + split of the fused wqkv output (modeling_internlm2.py:359-388, 233-247).
// qkv row = [8 groups][4 q | k | v][128].  q_embed = bf16(bf16(q*cos) + bf16(rotate_half(q)*sin)), same for k.
// grid (rows, 8 groups), 128 threads: thread = (slot 0..7 [6 used], 16-B chunk 0..15).
// Q8 (e4m3 cache): the K / V rows go to the cache as e4m3 bytes + one fp32 scale each (common.hpp's e4m3 row rule, as quant_fp8_rows_kernel; a slot's 16 chunks
// are one DPP row, so the row maximum is four rotate-max steps), and -- when kc / vc are given (prefill) -- as bf16 into the prefill's staging
// [pages][8][stage_T][128] at (row_page[row], pos), which the prefill attention reads instead of the cache.
// OFF (a draft window's rows, cr_llm_decode_draft): the row sits row_off[row] positions past lens[seq]; an instance of its own.
template <bool Q8 = false, bool OFF = false>
__global__ __launch_bounds__(128) void rope_split_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ cosT,
                                                         const bf16* __restrict__ sinT, bf16* __restrict__ q_out,
                                                         bf16* __restrict__ kc, bf16* __restrict__ vc, int pos0, int seq0,
                                                         const int32_t* __restrict__ seqs, const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ row_pos, int max_tokens,
                                                         const float* __restrict__ part, int splits,
                                                         unsigned char* __restrict__ k8 = nullptr, unsigned char* __restrict__ v8 = nullptr,
                                                         float* __restrict__ ks = nullptr, float* __restrict__ vs = nullptr,
                                                         const int32_t* __restrict__ row_page = nullptr, int stage_T = 0,
                                                         const int32_t* __restrict__ row_off = nullptr) {
    // part != nullptr (decode): the wqkv output arrives as `splits` fp32 K-slices [s][rows][QKV]; their sum in slice
    // order, rounded once, is the bf16 linear output the reference rotates
    const int row = blockIdx.x, grp = blockIdx.y;
    const int slot = threadIdx.x >> 4, c = threadIdx.x & 15;
    if (slot >= 6) return;
    const int seq = seqs ? seqs[row] : seq0;
    const int pos = (row_pos ? row_pos[row] : (lens ? lens[seq] : pos0 + row)) + (OFF ? row_off[row] : 0);
    const int64_t col0 = (int64_t)(grp * 6 + slot) * HD;
    auto chunk = [&](int cc) -> bf16x8 {
        if (!part) return *(const bf16x8*)(qkv + (int64_t)row * QKV + col0 + cc * 8);
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < splits; s++) {
            const f32x4* pp = (const f32x4*)(part + ((int64_t)s * gridDim.x + row) * QKV + col0 + cc * 8);
            const f32x4 v0 = pp[0], v1 = pp[1];
#pragma unroll
            for (int e = 0; e < 4; e++) { a[e] += v0[e]; a[4 + e] += v1[e]; }
        }
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; e++) r[e] = f2bf(a[e]);
        return r;
    };
    const bf16x8 x = chunk(c);
    bf16x8 y;
    if (slot < 5) {
        const bf16x8 xp = chunk((c + 8) & 15);
        const bf16x8 cs = *(const bf16x8*)(cosT + (int64_t)pos * HD + c * 8);
        const bf16x8 sn = *(const bf16x8*)(sinT + (int64_t)pos * HD + c * 8);
        const float sign = c < 8 ? -1.0f : 1.0f;           // rotate_half: (-x2, x1)
#pragma unroll
        for (int e = 0; e < 8; e++)
            y[e] = f2bf(rbf(bf2f(x[e]) * bf2f(cs[e])) + rbf(sign * bf2f(xp[e]) * bf2f(sn[e])));
    } else {
        y = x;
    }
    if (Q8 && slot >= 4) {
        float mx = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) mx = fmaxf(mx, fabsf(bf2f(y[e])));
        mx = row_max16(mx);
        const float sc = e4m3_row_scale(mx);
        const uint2 y8 = pack8_e4m3(y, 1.0f / sc);
        const int64_t r8 = ((int64_t)seq * NKV + grp) * max_tokens + pos;
        *(uint2*)((slot == 4 ? k8 : v8) + r8 * HD + c * 8) = y8;
        if (c == 0) (slot == 4 ? ks : vs)[r8] = sc;
        if (kc) {
            bf16* base = slot == 4 ? kc : vc;
            *(bf16x8*)(base + (((int64_t)row_page[row] * NKV + grp) * stage_T + pos) * HD + c * 8) = y;
        }
        return;
    }
    bf16* dst;
    if (slot < 4) dst = q_out + (int64_t)row * D + (grp * 4 + slot) * HD;
    else {
        bf16* base = slot == 4 ? kc : vc;
        dst = base + (((int64_t)seq * NKV + grp) * max_tokens + pos) * HD;
    }
    *(bf16x8*)(dst + c * 8) = y;
}

// prefill: the cached length of every page's sequence = its first position + its rows (d_seg: 4 per page, see cr_llm_prefill_batch).
// Only the prefilled sequences are written: another context may be decoding other sequences of the same cache meanwhile.
__global__ __launch_bounds__(256) void set_len_kernel(const int32_t* __restrict__ seg, int n, int32_t* __restrict__ lens) {
    for (int i = threadIdx.x; i < n; i += 256) lens[seg[4 * i + 3]] = seg[4 * i + 2] + seg[4 * i + 1];
}

int rms(const bf16* in, bf16* out, const bf16* w, int64_t rows, float eps, hipStream_t st, float* row_scale = nullptr) {
    NormParams np{};
    np.in = in; np.ld_in = D; np.out = out; np.ld_out = D; np.gamma = w; np.rows = rows; np.eps = eps;
    if (row_scale) { np.out8 = (unsigned char*)out; np.out8_scale = row_scale; }     // e4m3 rows in the first half of `out`
    return launch_rmsnorm(np, D, st);
}

enum LinForm {
    LIN_PREFILL,    // bf16 as loaded; a prompt row's result must not depend on what it is prefilled with: prompts of <= 64 rows in all stay on the tiled kernel,
                    // whose K order is that of every longer prefill (the weight-streaming kernel the dispatcher would pick splits K over its waves)
    LIN_LOADED,     // bf16 as loaded, the dispatcher's choice of kernel
    LIN_DECODE,     // <= 64 rows: the weight-streaming kernels take the decode-layout copy where llm_finalize made one (a contiguous KiB per load instruction)
    LIN_E4M3        // the e4m3 copy (decode only: C = (A . W8^T) * wscale), <= 64 rows in its decode layout where cr_enable_fp8_decode made one
};

// C = epi(A . W^T) on dense rows: lda = ldw = K, ldc = the width the epilogue writes; EPI_RES adds into C in place
int linear(cr_ctx* c, int epi, const bf16* A, const LinW& w, LinForm form, void* C, int M, hipStream_t st) {
    GemmParams p{};
    p.A = A; p.lda = w.K; p.W = w.w; p.ldw = w.K; p.C = C; p.ldc = epi == EPI_SWIGLU ? w.N / 2 : w.N; p.M = M; p.N = w.N; p.K = w.K;
    if (epi == EPI_RES) { p.res = (const bf16*)C; p.ldr = p.ldc; }
    if (form == LIN_E4M3) {
        if (!w.e4m3()) return cr_fail(CR_ERR_STATE, "linear: no e4m3 copy of this weight (cr_enable_fp8_decode)");
        p.W = (const bf16*)w.q8; p.w8 = 1; p.wscale = w.s8;
        if (w.dl8 && M <= 64) { p.W = (const bf16*)w.dl8; p.wsw = 1; }
    } else if (form == LIN_DECODE && w.dl && M <= 64) { p.W = w.dl; p.wsw = w.dl_kind; }
    else if (form == LIN_PREFILL && M <= 64) p.kernel = 128;
    return ctx_gemm(c, epi, p, st);
}

// the same on the fp8 matrix cores (prefill): A as e4m3 rows with one scale each, the weight's e4m3 copy
int linear_f8(cr_ctx* c, int epi, const void* a8, const float* ascale, const LinW& w, void* C, int M, hipStream_t st) {
    const bool res = epi == EPI_RES;
    return ctx_gemm_f8(c, epi, a8, ascale, w.q8, w.s8, C, epi == EPI_SWIGLU ? w.N / 2 : w.N, nullptr, M, w.N, w.K, st, res ? (const bf16*)C : nullptr, res ? w.N : 0);
}

// One layer of the cache: bf16 rows [n_seqs][8][max_tokens][128], or e4m3 rows of that shape + one scale per row (the other pointers null)
struct LayerKV { bf16 *k, *v; unsigned char *k8, *v8; float *ks, *vs; };
LayerKV layer_kv(const cr_kv* kv, int l) {
    const int64_t per_layer = (int64_t)kv->n_seqs * NKV * kv->max_tokens * HD;
    if (kv->fmt == CR_KV_E4M3) return {nullptr, nullptr, kv->k8 + l * per_layer, kv->v8 + l * per_layer, kv->ks + l * (per_layer / HD), kv->vs + l * (per_layer / HD)};
    return {kv->k + l * per_layer, kv->v + l * per_layer, nullptr, nullptr, nullptr, nullptr};
}

constexpr float LLM_S_DIV = 11.313708498984761f;      // math.sqrt(128)
// what every attention launch of the stage shares: K / V rows [slot][8][T][128], bf16-rounded scores divided by sqrt(128)
AttnParams attn_params(const LayerKV& lk, int T, bf16* q, bf16* ao) {
    AttnParams ap{};
    ap.K = lk.k; ap.V = lk.v; ap.Q = q; ap.O = ao;
    ap.k_bs = ap.v_bs = (int64_t)NKV * T * HD; ap.k_rs = ap.v_rs = HD; ap.k_hs = ap.v_hs = (int64_t)T * HD;
    ap.q_prescale = 1.0f; ap.s_div = LLM_S_DIV;
    return ap;
}

// Causal prefill attention, the pages' query blocks as ONE launch of `n_segs` segments {first row, rows, first position, slot} whose longest has Sq rows:
// causal attention is per page, the linear layers see all pages at once (a launch per page left its 800 workgroups of 2..50 key tiles each a ragged
// tail on 512 slots).  q / ao rows are [row][32 heads][128].
AttnParams prefill_attn_params(const LayerKV& lk, int T, bf16* q, bf16* ao, int n_segs, const int32_t* seg, int Sq) {
    static_assert(HD == 128 && D == NH * HD, "segment_attn_params lays rows out as [row][NH][128]");
    return segment_attn_params(lk.k, lk.v, T, q, ao, NH, NH / NKV, n_segs, seg, Sq, attn_params(lk, T, q, ao).s_div);      // (attention.hpp; cr_op_attention_segments fills its launch there too)
}

struct Segment { int seq, row0, S, pos0; };     // a page's rows inside a batched prefill

// The index arrays of a batched prefill (M rows, n pages): one block of ints, laid out the same on the host and on the device
struct PrefillRows {
    int32_t *row_seq, *row_pos;      // per row: cache slot, position
    int32_t* seg;                    // per page, 4 ints: first row, rows, first position, cache slot (the attention launch's segments)
    int32_t* seg_last;               // per page, 4 ints: the final layer's segment, the rows that share a 32-row wave with the page's last row
    int32_t* last;                   // per page: that last row
    int32_t *seg8, *seg_last8;       // e4m3 cache only: seg and seg_last with the page index as the slot (they address the staging)
    int32_t* row_page;               // e4m3 cache only: page index of every row
};
size_t prefill_rows_ints(int M, int n, bool kv8) { return 2 * (size_t)M + 9 * (size_t)n + (kv8 ? 8 * (size_t)n + (size_t)M : 0); }
PrefillRows prefill_rows(int32_t* p, int M, int n) {
    int32_t* g = p + 2 * (size_t)M;
    return {p, p + M, g, g + 4 * n, g + 8 * n, g + 9 * n, g + 13 * n, g + 17 * n};
}

// The grounding hook of a batched prefill (cr_llm_ground_batch): span_mass of ground.hip on layers [layer0, layer1), launched right after RoPE + split, when the
// roped q of every row sits in b.q and the roped k in the cache.  p.k, p.first and p.last are filled in per layer.
struct GroundHook { SpanMassParams p; int layer0, layer1; };

// What a batched prefill (M prompt rows of n_pages pages, the longest max_S rows) takes from the workspace
struct PrefillBufs {
    int M, n_pages, max_S, ff;
    bool kv8;           // prefill into an e4m3 cache: the prompts' bf16 K / V of the current layer go to a staging [pages][8][max_S][128] that the prefill attention
                        // reads; the cache gets the e4m3 rows
    bool any8;          // fp8 matrix-core path (cr_enable_fp8_mfma): both norms emit e4m3 rows + scales, wqkv and w1|w3 take them (gemm256 F8)
    bool last_rows;     // the final layer on the pages' last rows only, see prefill_layers
    bf16 *x, *stage_k, *stage_v, *h, *qkv, *q, *ao, *act, *xl, *aol, *hl2, *actl;
    float* hs;          // any8: one scale per normalised row
    unsigned char* a8;  // any8: e4m3 rows of the attention output / the SwiGLU output
    PrefillRows rows;
    HeadBufs head;
    const GroundHook* ground = nullptr;      // null: the call does not ground (nothing is launched for it)

    PrefillBufs(cr_ctx* c, int ff, const cr_kv* kv, int M, int n_pages, int max_S, const RowFeatures& f)
        : M(M), n_pages(n_pages), max_S(max_S), ff(ff), kv8(kv->fmt == CR_KV_E4M3), any8(c->fp8_mfma && M >= 256),
          last_rows(c->prefill_last_rows && !any8 && !c->probe_dst), head{n_pages, c->d.vocab, f} {}

    void carve(Arena& ar) {
        x = ar.take<bf16>((size_t)M * D);
        stage_k = kv8 ? ar.take<bf16>((size_t)n_pages * NKV * max_S * HD) : nullptr;
        stage_v = kv8 ? ar.take<bf16>((size_t)n_pages * NKV * max_S * HD) : nullptr;
        h = ar.take<bf16>((size_t)M * D); qkv = ar.take<bf16>((size_t)M * QKV); q = ar.take<bf16>((size_t)M * D); ao = ar.take<bf16>((size_t)M * D);
        act = ar.take<bf16>((size_t)M * ff);
        hs = any8 ? ar.take<float>((size_t)M) : nullptr;
        a8 = any8 ? ar.take<unsigned char>((size_t)M * ff) : nullptr;
        xl = aol = hl2 = actl = nullptr;
        if (last_rows) {
            xl = ar.take<bf16>((size_t)n_pages * D); aol = ar.take<bf16>((size_t)n_pages * D); hl2 = ar.take<bf16>((size_t)n_pages * D);
            actl = ar.take<bf16>((size_t)n_pages * ff);
        }
        rows = prefill_rows(ar.take<int32_t>(prefill_rows_ints(M, n_pages, kv8)), M, n_pages);
        head.carve(ar);
    }
};

// The decoder stack over the prompt rows b.x of a batched prefill.
int prefill_layers(cr_ctx* c, const LlmWeights& lw, cr_kv* kv, const PrefillBufs& b, hipStream_t st) {
    const PrefillRows& r = b.rows;
    const int M = b.M, n_pages = b.n_pages, layers = c->d.llm_layers;
    const float eps = c->d.rms_eps;
    const bf16 *cosT = lw.cosT, *sinT = lw.sinT;
    // cr_llm_hidden_probe (parity tooling): rows [row0, row0 + rows) of the residual stream before layer 0 and after every layer
    auto probe = [&](int slot) -> int {
        if (!c->probe_dst || c->probe_row0 + c->probe_rows > M) return CR_OK;
        CR_HIP(hipMemcpyAsync(c->probe_dst + (size_t)slot * c->probe_rows * D, b.x + (size_t)c->probe_row0 * D, (size_t)c->probe_rows * D * 2,
                              hipMemcpyDeviceToDevice, st));
        return CR_OK;
    };
    CR_TRY(probe(0));
    for (int l = 0; l < layers; l++) {
        const LayerW& w = lw.layer[l];
        LayerKV lk = layer_kv(kv, l);
        if (b.kv8) { lk.k = b.stage_k; lk.v = b.stage_v; }
        const int T = b.kv8 ? b.max_S : kv->max_tokens;      // rows per (slot, head) of what the attention reads
        const bool m8 = b.any8 && w.qkv.e4m3() && w.w13.e4m3();
        const bool m8all = m8 && c->fp8_mfma >= 2 && w.o.e4m3() && w.w2.e4m3();      // level 2: wo and w2 as well (their inputs take a quantiser pass)
        // x += in . W^T for wo and w2.  Level 2: their inputs are activations no norm produced, so one quantiser pass each (row maximum, then the e4m3 row)
        auto add_linear = [&](const bf16* in, const LinW& lin) -> int {
            if (!m8all) return linear(c, EPI_RES, in, lin, LIN_PREFILL, b.x, M, st);
            launch_quant_fp8_rows(in, lin.K, M, lin.K, b.a8, b.hs, st);
            return linear_f8(c, EPI_RES, b.a8, b.hs, lin, b.x, M, st);
        };
        CR_TRY(rms(b.x, b.h, w.an, M, eps, st, m8 ? b.hs : nullptr));
        CR_TRY(m8 ? linear_f8(c, EPI_STORE, b.h, b.hs, w.qkv, b.qkv, M, st) : linear(c, EPI_STORE, b.h, w.qkv, LIN_PREFILL, b.qkv, M, st));
        // (bf16 cache: lk's e4m3 pointers are null, and the kernel takes no staging)
        hipLaunchKernelGGL(b.kv8 ? rope_split_kernel<true> : rope_split_kernel<false>, dim3(M, NKV), dim3(128), 0, st, b.qkv, cosT, sinT, b.q, lk.k, lk.v, 0, 0,
                           r.row_seq, nullptr, r.row_pos, kv->max_tokens, nullptr, 0, lk.k8, lk.v8, lk.ks, lk.vs, b.kv8 ? r.row_page : nullptr, b.kv8 ? b.max_S : 0, nullptr);
        if (b.ground && l >= b.ground->layer0 && l < b.ground->layer1) {
            SpanMassParams gp = b.ground->p;
            gp.k = lk.k; gp.first = l == b.ground->layer0; gp.last = l + 1 == b.ground->layer1;
            if (launch_span_mass(gp, st) != CR_OK) return cr_fail(CR_ERR_HIP, "span mass launch failed");
        }
        // FINAL layer: only each page's last row is ever read again (the LM head, :1081-1082 + _sample; the reference computes every row).  K / V of
        // every row still go to the cache, so the norm, wqkv and RoPE + split run on all rows; attention, wo, the second norm, w1|w3 and w2 run on the n last rows
        // only -- 88 % of that layer's linear work.  Bit-exact: the tiled kernels give a row the same sum whatever it is batched with (LIN_PREFILL pins rows <= 64;
        // more pages than that take the tiled kernel by the dispatcher's own rule), and the attention launch keeps a last row in the company of the rows that share
        // its WAVE in the full launch (the kernel's deferred-rescale vote is wave-wide): segment = {first row of that 32-row group, rows up to the last, their first
        // position}.  CR_PREFILL_LAST_ROWS=0: every row (A/B aid).
        if (b.last_rows && l + 1 == layers) {
            if (launch_flash_attn(prefill_attn_params(lk, T, b.q, b.ao, n_pages, b.kv8 ? r.seg_last8 : r.seg_last, 32), HD, true, st) != CR_OK)
                return cr_fail(CR_ERR_HIP, "prefill attention launch failed");
            hipLaunchKernelGGL(move_rows_kernel<true>, dim3(n_pages), dim3(256), 0, st, b.ao, r.last, b.aol);
            hipLaunchKernelGGL(move_rows_kernel<true>, dim3(n_pages), dim3(256), 0, st, b.x, r.last, b.xl);
            CR_TRY(linear(c, EPI_RES, b.aol, w.o, LIN_PREFILL, b.xl, n_pages, st));
            CR_TRY(rms(b.xl, b.hl2, w.fn, n_pages, eps, st));
            CR_TRY(linear(c, EPI_SWIGLU, b.hl2, w.w13, LIN_PREFILL, b.actl, n_pages, st));
            CR_TRY(linear(c, EPI_RES, b.actl, w.w2, LIN_PREFILL, b.xl, n_pages, st));
            hipLaunchKernelGGL(move_rows_kernel<false>, dim3(n_pages), dim3(256), 0, st, b.xl, r.last, b.x);
            continue;
        }
        if (launch_flash_attn(prefill_attn_params(lk, T, b.q, b.ao, n_pages, b.kv8 ? r.seg8 : r.seg, b.max_S), HD, true, st) != CR_OK)
            return cr_fail(CR_ERR_HIP, "prefill attention launch failed");
        CR_TRY(add_linear(b.ao, w.o));
        CR_TRY(rms(b.x, b.h, w.fn, M, eps, st, m8 ? b.hs : nullptr));
        CR_TRY(m8 ? linear_f8(c, EPI_SWIGLU, b.h, b.hs, w.w13, b.act, M, st) : linear(c, EPI_SWIGLU, b.h, w.w13, LIN_PREFILL, b.act, M, st));
        CR_TRY(add_linear(b.act, w.w2));
        CR_TRY(probe(l + 1));
    }
    CR_HIP(hipGetLastError());
    return CR_OK;
}

// The index arrays of a batched prefill, built on the host and copied into b.rows
int stage_prefill_rows(const PrefillBufs& b, const std::vector<Segment>& segs, hipStream_t st) {
    const int M = b.M, n = b.n_pages;
    const bool kv8 = b.kv8;
    std::vector<int32_t> h(prefill_rows_ints(M, n, kv8));
    const PrefillRows hr = prefill_rows(h.data(), M, n);
    for (int i = 0; i < n; i++) {
        const Segment& sg = segs[i];
        int32_t *e = hr.seg + 4 * i, *f = hr.seg_last + 4 * i;
        e[0] = sg.row0; e[1] = sg.S; e[2] = sg.pos0; e[3] = sg.seq;
        // the attention kernel's query blocks are 128 rows of a segment, its waves 32: rows [32 k, 32 k + 32) of a page meet in one wave
        const int w0 = (sg.S - 1) / 32 * 32;
        f[0] = sg.row0 + w0; f[1] = sg.S - w0; f[2] = sg.pos0 + w0; f[3] = sg.seq;
        hr.last[i] = sg.row0 + sg.S - 1;
        for (int r = 0; r < sg.S; r++) { hr.row_seq[sg.row0 + r] = sg.seq; hr.row_pos[sg.row0 + r] = sg.pos0 + r; }
        if (kv8) {
            for (int k = 0; k < 3; k++) { hr.seg8[4 * i + k] = e[k]; hr.seg_last8[4 * i + k] = f[k]; }
            hr.seg8[4 * i + 3] = hr.seg_last8[4 * i + 3] = i;
            for (int r = 0; r < sg.S; r++) hr.row_page[sg.row0 + r] = i;
        }
    }
    CR_HIP(hipMemcpyAsync(b.rows.row_seq, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));   // pageable source: staged before return
    return CR_OK;
}

// What cr_llm_score_batch takes from the workspace: a batched prefill whose final layer runs on every row, then the R scored rows' head in tiles
struct ScoreBufs {
    PrefillBufs pre;
    int R, tile, V;
    bool pen;           // penalty != 1: one first-occurrence table per sequence of the call (score.hpp)
    bf16 *xs, *hl;      // the scored rows of the residual stream, gathered; one tile of them normalised
    float* lg;          // one tile of logits [tile][V]
    void* scratch;      // the score kernels' partials for one tile
    int32_t* gather;    // per scored row: its row in the prefill
    int64_t* index;     // score.hpp's index block
    int32_t* first;
    // cr_llm_ground_batch: the hook, its index arrays and one layer's partials (g_ints = 0: the call does not ground).  head = false: grounding only, no LM head
    bool head = true;
    size_t g_ints = 0, g_part = 0;
    int32_t* g_index = nullptr;
    GroundHook hook{};

    ScoreBufs(cr_ctx* c, int ff, const cr_kv* kv, int M, int n_pages, int max_S, int R, bool pen)
        : pre(c, ff, kv, M, n_pages, max_S, RowFeatures{}), R(R), tile(std::min(R, SCORE_HEAD_ROWS)), V(c->d.vocab), pen(pen) {
        pre.last_rows = false;      // any row may be scored
        pre.head.n = 0;             // no pick: the head below is the call's own
    }

    void carve(Arena& ar) {
        pre.carve(ar);
        xs = hl = nullptr; lg = nullptr; scratch = nullptr; gather = nullptr; index = nullptr; first = nullptr;
        if (head) {
            xs = ar.take<bf16>((size_t)R * D); hl = ar.take<bf16>((size_t)tile * D);
            lg = ar.take<float>((size_t)tile * V);
            scratch = ar.take<char>(logprobs_scratch_bytes(tile, V));
            gather = ar.take<int32_t>((size_t)R);
            index = ar.take<int64_t>(score_index_words(R));
            first = pen ? ar.take<int32_t>((size_t)pre.n_pages * V) : nullptr;
        }
        if (g_ints) {
            g_index = ar.take<int32_t>(g_ints);
            hook.p.partial = ar.take<float>(g_part);
        }
    }
};

// What a decode step (M rows, one per sequence; the longest sequence's keys in nsplit attention splits) takes from the workspace
struct DecodeBufs {
    int M, nsplit, ff;
    bool kv8;
    // <= 64 rows: wqkv, wo and w2 run as K-sliced partial-sum GEMMs (gemm_skinny.hip: tall workgroups re-read X once per 64 weight rows); the slices are
    // summed by the kernel that consumes the result anyway -- RoPE/split for wqkv, the residual add fused with the NEXT RMSNorm for wo and w2 -- in slice
    // order, so a row's result is the same whatever it is batched with.  CR_NO_SLICED_DECODE=1, or > 64 rows: the one-tile GEMMs.
    int s_qkv, s_o, s_2;
    bool sliced;
    // <= DECODE_FUSED_MAX_ROWS = 8 rows: gemm_decode.hip folds the norms, RoPE + split and the residual adds into the five GEMMs -- six launches per layer instead
    // of nine, every sum in the order of the separate kernels (a row's bits do not depend on its batch): its virtual slices are compiled in, so the path is only
    // taken while the K-sliced kernels' geometry (cost model or CR_PARTIAL_GEOM) is the one they reproduce (an e4m3 cache takes the separate kernels: the fused
    // wqkv epilogue writes bf16 cache rows)
    bool fused;
    bf16 *x, *h, *qkv, *q, *ao, *act;
    float *part, *pbuf;      // the attention splits' partials; the K-slices of one GEMM ([slices][M][N] fp32, the largest of the three)
    HeadBufs head;
    // cr_llm_decode_draft: rows of one sequence's draft window.  off (NULL in a plain step, and in a draft step without a window): row i sits off[i] positions past
    // its sequence's cached length -- RoPE, the cache row and the key count follow it, and the RoPE-folded attention form is not taken.  Set by DraftBufs' carve.
    const int32_t* off = nullptr;
    // rows that read a shared prompt (cr_kv_fork_shared): the launch's share table on the device (ctx_stage_share; attention.hpp: attn_share_table), share_n = 0:
    // none, and the step launches what it always launched.  With shares the RoPE-folded attention form is not taken (the separate launch gives the same bits)
    const int32_t* share = nullptr;
    int share_n = 0, share_splits = 0;

    DecodeBufs(cr_ctx* c, int ff, const cr_kv* kv, int M, int nsplit, const RowFeatures& f)
        : M(M), nsplit(nsplit), ff(ff), kv8(kv->fmt == CR_KV_E4M3), s_qkv(gemm_partial_splits(QKV, D)),
          s_o(gemm_partial_splits(D, D)), s_2(gemm_partial_splits(D, ff)), sliced(M <= 64 && s_qkv > 0 && s_o > 0 && s_2 > 0 && !c->no_sliced_decode),
          fused(sliced && c->fused_decode && !c->fp8_decode && !kv8 && decode_fused_supported(M, ff) && s_qkv == DEC_SLICES_WQKV && s_o == DEC_SLICES_WO &&
                s_2 == DEC_SLICES_W2), head{M, c->d.vocab, f} {}

    void carve(Arena& ar) {
        x = ar.take<bf16>((size_t)M * D);
        part = ar.take<float>(attn_split_ws_floats(M, NKV, NH / NKV, nsplit, HD));
        h = ar.take<bf16>((size_t)M * D); q = ar.take<bf16>((size_t)M * D); ao = ar.take<bf16>((size_t)M * D); act = ar.take<bf16>((size_t)M * ff);
        qkv = sliced ? nullptr : ar.take<bf16>((size_t)M * QKV);
        pbuf = sliced ? ar.take<float>((size_t)std::max(s_qkv * QKV, std::max(s_o, s_2) * D) * M) : nullptr;
        head.carve(ar);
    }
};

// The decode attention launch: rows = the 4 query heads of one KV group, all at the same position (no mask needed), the keys of cache slot seqs[row]
// in nsplit splits.  The one description of it: the fused path, decode_attn_fold_supported and the launch itself all start from this.
AttnParams decode_attn_params(const cr_kv* kv, const LayerKV& lk, const DecodeBufs& b, const int32_t* d_seqs) {
    AttnParams ap = attn_params(lk, kv->max_tokens, b.q, b.ao);
    if (b.kv8) {      // attention_decode.hip, decode_attn8_kernel
        ap.K8 = lk.k8; ap.V8 = lk.v8; ap.k_scale = lk.ks; ap.v_scale = lk.vs;
        ap.s_bs = (int64_t)NKV * kv->max_tokens; ap.s_hs = kv->max_tokens;
    }
    ap.q_bs = D; ap.q_rs = HD; ap.q_hs = 4 * HD; ap.o_bs = D; ap.o_rs = HD; ap.o_hs = 4 * HD;
    ap.B = b.M; ap.H = NKV; ap.Sq = NH / NKV; ap.Sk = 0; ap.kv_group = 1; ap.q_pos0 = 0;
    ap.seq_map = d_seqs; ap.sk_arr = kv->d_len; ap.sk_add = 1; ap.sk_off = b.off;
    ap.nsplit = b.nsplit; ap.part_ml = b.part; ap.part_o = b.part + (size_t)b.M * NKV * b.nsplit * (NH / NKV) * 2;
    if (b.share_n > 0) { ap.share_skip = b.share; ap.share_chunks = b.share + b.M; ap.share_n = b.share_n; ap.share_splits = b.share_splits; }
    return ap;
}

// gemm_decode.hip's parameters for one weight: the decode-layout copy where there is one
DecodeGemmParams fused_gemm_params(cr_ctx* c, const LinW& w, int M) {
    DecodeGemmParams dp{};
    dp.M = M; dp.eps = c->d.rms_eps; dp.W = w.w; dp.ldw = w.K; dp.N = w.N; dp.K = w.K;
    if (w.dl) { dp.W = w.dl; dp.swizzled = 1; }
    return dp;
}

// The decoder stack over the rows b.x of a decode step (row i = the next token of sequence d_seqs[i]).
int decode_layers(cr_ctx* c, const LlmWeights& lw, cr_kv* kv, const DecodeBufs& b, const int32_t* d_seqs, hipStream_t st) {
    const int M = b.M, layers = c->d.llm_layers;
    const float eps = c->d.rms_eps;
    const bf16 *cosT = lw.cosT, *sinT = lw.sinT;
    auto fused_layer = [&](const LayerW& w, const LayerKV& lk) -> int {
        DecodeGemmParams dp = fused_gemm_params(c, w.qkv, M);
        dp.xres = b.x; dp.gamma = w.an;
        dp.cosT = cosT; dp.sinT = sinT; dp.q_out = b.q; dp.kc = lk.k; dp.vc = lk.v; dp.seqs = d_seqs; dp.lens = kv->d_len; dp.max_tokens = kv->max_tokens;
        dp.pos_off = b.off;
        CR_TRY(launch_decode_gemm(DEC_WQKV, dp, st));
        if (launch_flash_attn_split(decode_attn_params(kv, lk, b, d_seqs), HD, st) != CR_OK) return cr_fail(CR_ERR_HIP, "decode attention launch failed");
        dp = fused_gemm_params(c, w.o, M);
        dp.X = b.ao; dp.ldx = D; dp.xio = b.x;
        CR_TRY(launch_decode_gemm(DEC_WO, dp, st));
        dp = fused_gemm_params(c, w.w13, M);
        dp.xres = b.x; dp.gamma = w.fn; dp.C = b.act; dp.ldc = b.ff;
        CR_TRY(launch_decode_gemm(DEC_W13, dp, st));
        dp = fused_gemm_params(c, w.w2, M);
        dp.X = b.act; dp.ldx = b.ff; dp.xio = b.x;
        return launch_decode_gemm(DEC_W2, dp, st);
    };
    for (int l = 0; l < layers; l++) {
        const LayerW& w = lw.layer[l];
        const LayerKV lk = layer_kv(kv, l);
        if (b.fused) {
            CR_TRY(fused_layer(w, lk));
            continue;
        }
        const bool f8 = M <= 64 && c->fp8_decode && w.qkv.e4m3() && w.o.e4m3() && w.w13.e4m3() && w.w2.e4m3();
        const LinForm dec = f8 ? LIN_E4M3 : LIN_DECODE;
        // the one-tile fallback takes bf16 wqkv, wo and w2 as loaded (wqkv's decode-layout copy is in RoPE tile order, which only the K-sliced kernel reads)
        const LinForm plain = f8 ? LIN_E4M3 : LIN_LOADED;
        if (b.sliced) {
            if (l == 0) CR_TRY(rms(b.x, b.h, w.an, M, eps, st));      // later layers: the add + norm after the previous layer's w2 left h
            CR_TRY(linear(c, EPI_PARTIAL, b.h, w.qkv, dec, b.pbuf, M, st));
        } else {
            CR_TRY(rms(b.x, b.h, w.an, M, eps, st));
            CR_TRY(linear(c, EPI_STORE, b.h, w.qkv, plain, b.qkv, M, st));
        }
        AttnParams ap = decode_attn_params(kv, lk, b, d_seqs);
        // 9..64 rows: RoPE + split + the new token's cache row are folded into the attention kernel (attention_decode.hip, FOLD) where it qualifies
        // (not on an e4m3 cache: rope_split_kernel<true> quantises the new rows, decode_attn8_kernel reads them back from the cache)
        AttnParams fp = ap;
        fp.qkv_part = b.pbuf; fp.qkv_splits = b.s_qkv; fp.qkv_ld = QKV; fp.rope_cos = cosT; fp.rope_sin = sinT;
        // (never with a draft window's rows: a row would read cache rows that other workgroups of the same launch are still writing; decode_attn_fold_supported
        // refuses AttnParams::sk_off, and the separate launch below gives the same bits)
        // (nor with rows that share a prompt: the group form reads q from b.q)
        const bool rope_folded = b.sliced && c->fold_rope && !b.kv8 && b.share_n == 0 && decode_attn_fold_supported(fp, HD);
        if (rope_folded) ap = fp;
        // (b.pbuf: wqkv's K-slices when sliced, else null and the kernel reads b.qkv; of lk either the bf16 or the e4m3 pointers are null)
        else if (b.off)      // (bf16 caches only: cr_llm_decode_draft refuses an e4m3 one)
            hipLaunchKernelGGL((rope_split_kernel<false, true>), dim3(M, NKV), dim3(128), 0, st, b.qkv, cosT, sinT, b.q, lk.k, lk.v, 0, 0, d_seqs, kv->d_len, nullptr,
                               kv->max_tokens, (const float*)b.pbuf, b.s_qkv, nullptr, nullptr, nullptr, nullptr, nullptr, 0, b.off);
        else
            hipLaunchKernelGGL(b.kv8 ? rope_split_kernel<true> : rope_split_kernel<false>, dim3(M, NKV), dim3(128), 0, st, b.qkv, cosT, sinT, b.q, lk.k, lk.v, 0, 0,
                               d_seqs, kv->d_len, nullptr, kv->max_tokens, (const float*)b.pbuf, b.s_qkv, lk.k8, lk.v8, lk.ks, lk.vs, nullptr, 0, nullptr);
        if (launch_flash_attn_split(ap, HD, st) != CR_OK) return cr_fail(CR_ERR_HIP, "decode attention launch failed");
        if (b.sliced) {
            CR_TRY(linear(c, EPI_PARTIAL, b.ao, w.o, dec, b.pbuf, M, st));
            CR_TRY(launch_add_rmsnorm(b.x, b.pbuf, b.s_o, M, w.fn, b.h, eps, st));
        } else {
            CR_TRY(linear(c, EPI_RES, b.ao, w.o, plain, b.x, M, st));
            CR_TRY(rms(b.x, b.h, w.fn, M, eps, st));
        }
        CR_TRY(linear(c, EPI_SWIGLU, b.h, w.w13, dec, b.act, M, st));
        if (b.sliced) {
            CR_TRY(linear(c, EPI_PARTIAL, b.act, w.w2, dec, b.pbuf, M, st));
            // the last layer's sum only lands in x: the caller norms what it needs
            CR_TRY(launch_add_rmsnorm(b.x, b.pbuf, b.s_2, M, l + 1 < layers ? lw.layer[l + 1].an : nullptr, b.h, eps, st));
        } else {
            CR_TRY(linear(c, EPI_RES, b.act, w.w2, plain, b.x, M, st));
        }
    }
    CR_HIP(hipGetLastError());
    return CR_OK;
}

// The final RMSNorm and the LM head over the rows of a decode step: b.head.lg
int decode_head(cr_ctx* c, const LlmWeights& lw, const DecodeBufs& b, hipStream_t st) {
    const int n = b.M, V = c->d.vocab;
    const LinW& head = lw.head;
    if (c->fused_decode && !c->fp8_decode && !c->no_sliced_decode && decode_fused_supported(n, b.ff)) {
        DecodeGemmParams dh = fused_gemm_params(c, head, n);      // final RMSNorm folded into the LM head (gemm_decode.hip)
        dh.xres = b.x; dh.gamma = lw.norm; dh.C = b.head.lg; dh.ldc = V;
        return launch_decode_gemm(DEC_HEAD, dh, st);
    }
    CR_TRY(rms(b.x, b.head.hl, lw.norm, n, c->d.rms_eps, st));
    return linear(c, EPI_F32, b.head.hl, head, c->fp8_decode && n <= 64 && head.e4m3() ? LIN_E4M3 : LIN_DECODE, b.head.lg, n, st);
}

// A draft-verified step: the decode step's buffers for its M rows and draft.hpp's index block for its n sequences
struct DraftBufs {
    DecodeBufs dec;
    int n;
    bool windows;
    int64_t* index;
    DraftBufs(cr_ctx* c, int ff, const cr_kv* kv, int M, int n, int nsplit, const RowFeatures& f) : dec(c, ff, kv, M, nsplit, f), n(n), windows(M > n), index(nullptr) {}
    void carve(Arena& ar) {
        dec.carve(ar);
        index = ar.take<int64_t>(draft_index_words(n, dec.M));
        dec.off = windows && index ? draft_index(index, n, dec.M).off : nullptr;
    }
};

}  // namespace

extern "C" {

int cr_embed_splice(cr_ctx* c, const int64_t* ids, int S, const void* vit, int n_vit, int64_t img_id, const void* ref,
                    int n_ref, int64_t ref_id, void* out, void* stream) {
    if (!c || !ids || !out || S <= 0) return cr_fail(CR_ERR_ARG, "cr_embed_splice: bad argument");
    if ((size_t)S * 4 + 64 > c->scratch_bytes) return cr_fail(CR_ERR_ARG, "cr_embed_splice: S too large");
    CR_HIP(hipSetDevice(c->device));
    const bf16* table = llm_embed_table(c);
    if (!table) return CR_ERR_STATE;
    hipStream_t st = (hipStream_t)stream;
    int32_t* counts = (int32_t*)c->scratch;
    int32_t* src_row = counts + 16;
    hipLaunchKernelGGL(splice_index_kernel, dim3(1), dim3(1024), 0, st, ids, S, img_id, ref_id, vit ? 1 : 0, ref ? 1 : 0, src_row, counts);
    hipLaunchKernelGGL(splice_rows_kernel, dim3(S), dim3(256), 0, st, table, (const bf16*)vit, (const bf16*)ref, src_row, n_vit, n_ref, (bf16*)out);
    CR_HIP(hipGetLastError());
    // `input_embeds[selected] = vit_embeds` raises on a count mismatch in the reference; check it the same way
    int32_t hc[2];
    CR_HIP(hipMemcpyAsync(hc, counts, 8, hipMemcpyDeviceToHost, st));
    CR_HIP(hipStreamSynchronize(st));
    if (vit && hc[0] != n_vit) return cr_fail(CR_ERR_ARG, "cr_embed_splice: %d <IMG_CONTEXT> ids but %d visual rows", hc[0], n_vit);
    if (vit && hc[0] == 0) return cr_fail(CR_ERR_ARG, "cr_embed_splice: no <IMG_CONTEXT> id in the prompt");
    if (vit && ref && hc[1] != n_ref) return cr_fail(CR_ERR_ARG, "cr_embed_splice: %d pseudo-token ids but %d rows", hc[1], n_ref);
    if (vit && ref && hc[1] == 0) return cr_fail(CR_ERR_ARG, "cr_embed_splice: no pseudo-token id in the prompt");
    return CR_OK;
}

int cr_llm_prefill_batch(cr_ctx* c, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens, float penalty,
                         float* last_logits, void* stream) {
    if (!c || !kv || !seqs || !lens || !embeds || n <= 0 || n > kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_llm_prefill_batch: bad argument");
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "cr_llm_prefill_batch: call cr_finalize first");
    CR_TRY(ctx_share_ok(c, "cr_llm_prefill_batch"));
    const LlmWeights* lw;
    CR_TRY(llm_weights(c, &lw));
    std::vector<Segment> segs;
    int M = 0;
    for (int i = 0; i < n; i++) {
        const int s = seqs[i];
        if (s < 0 || s >= kv->n_seqs || lens[i] <= 0) return cr_fail(CR_ERR_ARG, "cr_llm_prefill_batch: bad sequence %d / length %d", s, lens[i]);
        for (int j = 0; j < i; j++) if (seqs[j] == s) return cr_fail(CR_ERR_ARG, "cr_llm_prefill_batch: sequence %d listed twice", s);
        if (kv->seq[s].len + lens[i] > kv->max_tokens)
            return cr_fail(CR_ERR_ARG, "cr_llm_prefill: %d + %d tokens exceed the cache (%d)", kv->seq[s].len, lens[i], kv->max_tokens);
        if (kv->fmt == CR_KV_E4M3 && kv->seq[s].len != 0)
            return cr_fail(CR_ERR_ARG, "cr_llm_prefill: sequence %d of an e4m3 cache already holds %d tokens (the prefill attends in bf16 and an e4m3 cache "
                           "keeps no bf16 copy of a prefix: cr_kv_reset it first)", s, kv->seq[s].len);
        CR_TRY(kv_refuse_sharer(kv, s, "cr_llm_prefill", "the prefill attention reads a sequence's own rows; continue an unshared copy (cr_kv_fork)"));
        if (kv->seq[s].len < kv_share_floor(kv, s))
            return cr_fail(CR_ERR_STATE, "cr_llm_prefill: %d other sequences read the first %d cached positions of sequence %d (cr_kv_fork_shared), and the prefill "
                           "would write from position %d", kv->seq[s].sharers, kv_share_floor(kv, s), s, kv->seq[s].len);
        if (kv->seq[s].bgrp >= 0 && (kv->seq[s].bgrp != s || kv->seq[s].len != 0 || kv->seq[s].ngen != 0))
            return cr_fail(CR_ERR_ARG, "cr_llm_prefill: sequence %d belongs to the beam group of sequence %d: prefill the group's FIRST sequence, once, after "
                           "cr_kv_reset and cr_kv_set_beam", s, kv->seq[s].bgrp);
        segs.push_back({s, M, lens[i], kv->seq[s].len});
        M += lens[i];
    }
    const RowFeatures feat = kv_scan_rows(kv, seqs, n, penalty);
    const bool beams = feat.beam_rows > 0;
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    int max_S = 0;
    for (const Segment& sg : segs) max_S = sg.S > max_S ? sg.S : max_S;
    PrefillBufs b(c, lw->ff, kv, M, n, max_S, feat);
    CR_TRY(ws_carve(c, "cr_llm_prefill_batch", b));
    CR_TRY(stage_prefill_rows(b, segs, st));
    CR_TRY(ctx_stage_seqs(c, seqs, n, st, true));
    CR_HIP(hipMemcpyAsync(b.x, embeds, (size_t)M * D * 2, hipMemcpyDeviceToDevice, st));
    CR_TRY(prefill_layers(c, *lw, kv, b, st));
    // only each page's last row feeds the LM head (the reference computes all S rows and reads the last, :1081 + _sample)
    for (int i = 0; i < n; i++)
        CR_TRY(rms(b.x + (size_t)(segs[i].row0 + segs[i].S - 1) * D, b.head.hl + (size_t)i * D, lw->norm, 1, c->d.rms_eps, st));
    CR_TRY(linear(c, EPI_F32, b.head.hl, lw->head, LIN_LOADED, b.head.lg, n, st));
    CR_TRY(pick_rows(kv, b.head, c->d_seqs, penalty, 0, last_logits, st, true));
    hipLaunchKernelGGL(set_len_kernel, dim3(1), dim3(256), 0, st, b.rows.seg, n, kv->d_len);
    if (beams) {    // the fan-out: the prompt's cache rows, the first id and the length go from a group's first sequence to its others
        std::vector<int> firsts;
        for (int i = 0; i < n; i++) if (kv->seq[seqs[i]].bgrp == seqs[i]) firsts.push_back(i);
        BeamLaunch bl = beam_launch(kv, b.head, 0, 1);
        if (kv->share_mode) { CR_TRY(kv_share_alloc(kv, st)); bl.share = 1; }      // the shared fork: the last < 256 positions only, the rest is read from the first
        CR_TRY(launch_beam_reorder(b.head.rows(c->d_seqs, penalty), kv_seq_state(kv), bl, beam_cache(kv), firsts.data(), (int)firsts.size(), max_S, 1, st));
    }
    CR_HIP(hipGetLastError());
    for (const Segment& sg : segs) {
        Seq& q = kv->seq[sg.seq];
        q.len += sg.S;
        if (q.ngen < kv->gen_cap) q.ngen += 1;
        if (q.bgrp == sg.seq)
            for (int j = 1; j < q.bnum; j++) {
                Seq& m = kv->seq[sg.seq + j];
                m.len = q.len; m.ngen = q.ngen;
                if (kv->share_mode && q.len >= 256) { m.pfx_src = sg.seq; m.pfx_len = q.len & ~255; q.sharers++; }      // (beam_reorder_kernel wrote the device side)
            }
    }
    return CR_OK;
}

int cr_llm_hidden_probe(cr_ctx* c, void* dst, int row0, int rows) {
    if (!c || (dst && (row0 < 0 || rows <= 0))) return cr_fail(CR_ERR_ARG, "cr_llm_hidden_probe: bad argument");
    c->probe_dst = (bf16*)dst; c->probe_row0 = row0; c->probe_rows = dst ? rows : 0;
    return CR_OK;
}

int cr_llm_prefill(cr_ctx* c, cr_kv* kv, int seq, const void* embeds, int S, float penalty, float* last_logits, void* stream) {
    if (!kv || S <= 0) return cr_fail(CR_ERR_ARG, "cr_llm_prefill: bad argument");
    const int32_t s = seq, l = S;
    return cr_llm_prefill_batch(c, kv, &s, 1, embeds, &l, penalty, last_logits, stream);
}

// What cr_llm_ground_batch adds to a scoring call (host arrays as the header describes them)
struct GroundArgs { const int32_t* spans; const int32_t* counts; int layer0, layer1; float* mass; int mass_ld; };

// cr_llm_score_batch and cr_llm_ground_batch: ONE function.  g = null: a scoring call, which launches what it always launched.  lp = null (grounding
// calls only): no gather, no final norm, no LM head, no score kernels.
static int score_rows_batch(const char* who, cr_ctx* c, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens, const int64_t* targets_host,
                            float penalty, int top_n, float* lp, int32_t* top_ids, float* top_lp, float* logits, const GroundArgs* g, void* stream) {
    if (top_n < 0 || top_n > LOGPROBS_MAX_TOP) return cr_fail(CR_ERR_ARG, "%s: top_n %d (want 0..%d)", who, top_n, LOGPROBS_MAX_TOP);
    if (!c || !kv || !seqs || !lens || !embeds || !targets_host || (!lp && !g) || (top_n > 0 && (!lp || !top_ids || !top_lp)) || n <= 0 || n > kv->n_seqs)
        return cr_fail(CR_ERR_ARG, "%s: bad argument", who);
    if (g && (!g->mass || !g->spans || !g->counts)) return cr_fail(CR_ERR_ARG, "%s: null mass, spans or span counts", who);
    if (!(penalty > 0.f) || penalty > FLT_MAX) return cr_fail(CR_ERR_ARG, "%s: penalty %g (want a finite value > 0)", who, penalty);
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "%s: call cr_finalize first", who);
    CR_TRY(ctx_share_ok(c, who));
    const LlmWeights* lw;
    CR_TRY(llm_weights(c, &lw));
    if (kv->fmt != CR_KV_BF16) return cr_fail(CR_ERR_ARG, "%s: an e4m3 cache (left out: a continued prefill needs the bf16 prefix)", who);
    if (g && (g->layer0 < 0 || g->layer1 > c->d.llm_layers || g->layer0 >= g->layer1))
        return cr_fail(CR_ERR_ARG, "%s: layers [%d, %d) (want a non-empty range inside [0, %d))", who, g->layer0, g->layer1, c->d.llm_layers);
    const int V = c->d.vocab;
    std::vector<Segment> segs;
    int M = 0, max_S = 0;
    for (int i = 0; i < n; i++) {
        const int s = seqs[i];
        if (s < 0 || s >= kv->n_seqs || lens[i] <= 0) return cr_fail(CR_ERR_ARG, "%s: bad sequence %d / length %d", who, s, lens[i]);
        for (int j = 0; j < i; j++) if (seqs[j] == s) return cr_fail(CR_ERR_ARG, "%s: sequence %d listed twice", who, s);
        if (kv->seq[s].len + lens[i] > kv->max_tokens)
            return cr_fail(CR_ERR_ARG, "%s: %d + %d tokens exceed the cache (%d)", who, kv->seq[s].len, lens[i], kv->max_tokens);
        if (kv->seq[s].bgrp >= 0) return cr_fail(CR_ERR_ARG, "%s: sequence %d belongs to the beam group of sequence %d", who, s, kv->seq[s].bgrp);
        CR_TRY(kv_refuse_sharer(kv, s, who, "the prefill attention reads a sequence's own rows; score an unshared copy (cr_kv_fork)"));
        if (kv->seq[s].len < kv_share_floor(kv, s))
            return cr_fail(CR_ERR_STATE, "%s: other sequences read the first %d cached positions of sequence %d (cr_kv_fork_shared), and the call would write from "
                           "position %d", who, kv_share_floor(kv, s), s, kv->seq[s].len);
        segs.push_back({s, M, lens[i], kv->seq[s].len});
        M += lens[i];
        max_S = std::max(max_S, lens[i]);
    }
    // the scored rows, in row order: slot r of lp / top_* / logits / mass; history = the call's sequence ordinal, ordinal = the row's place among that sequence's scored rows
    std::vector<int32_t> gather;
    std::vector<int64_t> tgt;
    std::vector<int32_t> hist, ord;
    for (int i = 0; i < n; i++) {
        int j = 0;
        for (int r = 0; r < segs[i].S; r++) {
            const int64_t y = targets_host[segs[i].row0 + r];
            if (y < 0) continue;
            if (y >= V) return cr_fail(CR_ERR_ARG, "%s: target %lld of sequence %d outside the vocabulary (%d)", who, (long long)y, segs[i].seq, V);
            gather.push_back(segs[i].row0 + r); tgt.push_back(y); hist.push_back(i); ord.push_back(j++);
        }
    }
    const int R = (int)gather.size();
    if (R == 0) return cr_fail(CR_ERR_ARG, "%s: no scored row (every target < 0)", who);
    // the grounded rows are the scored rows; a sequence's spans lie inside what it holds after the call
    std::vector<GroundSeq> gseqs;
    int g_total = 0, g_W = 0;
    if (g) {
        gseqs.resize(n);
        for (int i = 0; i < n; i++) {
            const int cnt = g->counts[i];
            if (cnt < 0 || cnt > GROUND_MAX_SPANS) return cr_fail(CR_ERR_ARG, "%s: %d spans for sequence %d (want 0..%d)", who, cnt, segs[i].seq, GROUND_MAX_SPANS);
            if (cnt > g->mass_ld) return cr_fail(CR_ERR_ARG, "%s: mass_ld %d below the %d spans of sequence %d", who, g->mass_ld, cnt, segs[i].seq);
            const int bad = ground_check_spans(g->spans + 2 * (size_t)g_total, cnt, segs[i].pos0 + segs[i].S);
            if (bad) return cr_fail(CR_ERR_ARG, "%s: span %d of sequence %d is reversed, overlaps its predecessor, is out of order or leaves [0, %d)", who, bad - 1,
                                    segs[i].seq, segs[i].pos0 + segs[i].S);
            gseqs[i].slot = segs[i].seq; gseqs[i].spans = g->spans + 2 * (size_t)g_total; gseqs[i].n_spans = cnt;
            g_total += cnt; g_W = std::max(g_W, cnt);
        }
        for (int r = 0; r < R; r++) {
            const Segment& sg = segs[hist[r]];
            gseqs[hist[r]].row_q.push_back(gather[r]); gseqs[hist[r]].row_pos.push_back(sg.pos0 + gather[r] - sg.row0);
        }
    }
    for (int i = 0; i < n; i++)
        if (kv->seq[seqs[i]].ngen != 0)
            return cr_fail(CR_ERR_STATE, "%s: sequence %d holds %d generated ids (the penalty history is the call's own: cr_kv_truncate / cr_kv_fork / "
                           "cr_kv_reset give a sequence without ids)", who, seqs[i], kv->seq[seqs[i]].ngen);
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const bool pen = penalty != 1.0f;
    ScoreBufs b(c, lw->ff, kv, M, n, max_S, R, pen);
    b.head = lp != nullptr;
    const int G = g ? ground_groups(gseqs) : 0;
    if (g) { b.g_ints = ground_index_ints(R, G, n, g_total); b.g_part = std::max<size_t>(span_mass_partial_floats(NH, R, g_W), 1); }
    CR_TRY(ws_carve(c, who, b));
    CR_TRY(stage_prefill_rows(b.pre, segs, st));
    if (g) {
        std::vector<int32_t> h(b.g_ints);
        ground_fill_index(gseqs, h.data());
        CR_HIP(hipMemcpyAsync(b.g_index, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));      // pageable source: staged before return
        SpanMassParams& gp = b.hook.p;
        gp.q = b.pre.q; gp.H = NH; gp.max_tokens = kv->max_tokens; gp.s_div = LLM_S_DIV;
        gp.R = R; gp.G = G; gp.W = g_W; gp.ix = ground_index(b.g_index, R, G, n, g_total);
        gp.mass = g->mass; gp.mass_ld = g->mass_ld; gp.scale = 1.0f / (float)(NH * (g->layer1 - g->layer0));
        b.hook.layer0 = g->layer0; b.hook.layer1 = g->layer1;
        b.pre.ground = &b.hook;
    }
    if (b.head) {
        std::vector<int64_t> h(score_index_words(R));
        const ScoreIndex hx = score_index(h.data(), R);
        for (int r = 0; r < R; r++) { hx.tgt[r] = tgt[r]; hx.hist[r] = hist[r]; hx.ord[r] = ord[r]; }
        CR_HIP(hipMemcpyAsync(b.index, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));      // pageable sources: staged before return
        CR_HIP(hipMemcpyAsync(b.gather, gather.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    }
    CR_HIP(hipMemcpyAsync(b.pre.x, embeds, (size_t)M * D * 2, hipMemcpyDeviceToDevice, st));
    CR_TRY(prefill_layers(c, *lw, kv, b.pre, st));
    if (b.head) {
        const ScoreIndex ix = score_index(b.index, R);
        hipLaunchKernelGGL(move_rows_kernel<true>, dim3(R), dim3(256), 0, st, b.pre.x, b.gather, b.xs);
        if (pen) CR_TRY(launch_score_table(ix, R, n, V, b.first, st));
        // the head in tiles: LIN_PREFILL keeps a row's logits independent of the tile's size and of the row's place in it
        for (int r0 = 0; r0 < R; r0 += b.tile) {
            const int rows = std::min(b.tile, R - r0);
            CR_TRY(rms(b.xs + (size_t)r0 * D, b.hl, lw->norm, rows, c->d.rms_eps, st));
            CR_TRY(linear(c, EPI_F32, b.hl, lw->head, LIN_PREFILL, b.lg, rows, st));
            if (logits) CR_HIP(hipMemcpyAsync(logits + (size_t)r0 * V, b.lg, (size_t)rows * V * 4, hipMemcpyDeviceToDevice, st));
            CR_TRY(launch_score_rows(ScoreLaunch{b.lg, V, V, rows, r0, ix, b.first, penalty, top_n, b.scratch, lp, top_ids, top_lp}, st));
        }
    }
    hipLaunchKernelGGL(set_len_kernel, dim3(1), dim3(256), 0, st, b.pre.rows.seg, n, kv->d_len);
    CR_HIP(hipGetLastError());
    for (const Segment& sg : segs) kv->seq[sg.seq].len += sg.S;      // no pick: no id is appended
    return CR_OK;
}

int cr_llm_score_batch(cr_ctx* c, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens, const int64_t* targets_host, float penalty,
                       int top_n, float* lp, int32_t* top_ids, float* top_lp, float* logits, void* stream) {
    return score_rows_batch("cr_llm_score_batch", c, kv, seqs, n, embeds, lens, targets_host, penalty, top_n, lp, top_ids, top_lp, logits, nullptr, stream);
}

int cr_llm_ground_batch(cr_ctx* c, cr_kv* kv, const int32_t* seqs, int n, const void* embeds, const int32_t* lens, const int64_t* targets_host, float penalty,
                        int top_n, float* lp, int32_t* top_ids, float* top_lp, const int32_t* spans_host, const int32_t* span_counts_host, int layer0, int layer1,
                        float* mass, int mass_ld, void* stream) {
    const GroundArgs g{spans_host, span_counts_host, layer0, layer1, mass, mass_ld};
    return score_rows_batch("cr_llm_ground_batch", c, kv, seqs, n, embeds, lens, targets_host, penalty, top_n, lp, top_ids, top_lp, nullptr, &g, stream);
}

int cr_llm_decode(cr_ctx* c, cr_kv* kv, const int32_t* seqs, int n, const int64_t* force_tokens, float penalty, float* logits,
                  void* stream) {
    if (!c || !kv || !seqs || n <= 0 || n > kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_llm_decode: bad argument");
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "cr_llm_decode: call cr_finalize first");
    CR_TRY(ctx_share_ok(c, "cr_llm_decode"));
    const LlmWeights* lw;
    CR_TRY(llm_weights(c, &lw));
    for (int i = 0; i < n; i++) {
        const int s = seqs[i];
        if (s < 0 || s >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_llm_decode: sequence %d out of range", s);
        if (kv->seq[s].len + 1 > kv->max_tokens) return cr_fail(CR_ERR_ARG, "cr_llm_decode: sequence %d cache full", s);
        if (!force_tokens && kv->seq[s].ngen == 0) return cr_fail(CR_ERR_STATE, "cr_llm_decode: sequence %d has no generated id to feed", s);
        for (int j = 0; j < i; j++) if (seqs[j] == s) return cr_fail(CR_ERR_ARG, "cr_llm_decode: sequence %d listed twice", s);
    }
    int beam_span = 0;                                        // > 0: the launch holds beam groups; the most cache positions their re-order moves
    std::vector<int> beam_firsts;                             // the rows of the groups' first sequences
    for (int i = 0; i < n && kv->d_beam; i++) {
        const int f = kv->seq[seqs[i]].bgrp;
        if (f < 0) continue;
        const int B = kv->seq[f].bnum;
        if (seqs[i] != f || i + B > n) return cr_fail(CR_ERR_ARG, "cr_llm_decode: a beam group decodes whole: its %d sequences from %d on, consecutive in seqs[]", B, f);
        for (int j = 1; j < B; j++)
            if (seqs[i + j] != f + j) return cr_fail(CR_ERR_ARG, "cr_llm_decode: a beam group decodes whole: its %d sequences from %d on, consecutive in seqs[]", B, f);
        if (force_tokens) return cr_fail(CR_ERR_ARG, "cr_llm_decode: force_tokens with a beam group (sequence %d)", f);
        beam_span = std::max(beam_span, kv->seq[f].ngen + 1);
        // the step's re-order moves rows [prompt length, length) only: past every shared prompt of the group (what the fan-out shared lies below the prompt's length)
        for (int j = 0; j < B; j++)
            if (kv->seq[f + j].pfx_len > kv->seq[f].len - kv->seq[f].ngen + 1)
                return cr_fail(CR_ERR_STATE, "cr_llm_decode: sequence %d shares %d positions, more than its group's prompt holds", f + j, kv->seq[f + j].pfx_len);
        beam_firsts.push_back(i);
        i += B - 1;
    }
    if (kv->fmt == CR_KV_E4M3 && !decode_attn8_available())
        return cr_fail(CR_ERR_ARG, "cr_llm_decode: an e4m3 cache is read by attention_decode.hip's e4m3 kernel only, and CR_DECODE_ATTN=0 selects the matrix-core "
                       "split kernel, which reads bf16 caches");
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    int max_len = 0;
    for (int i = 0; i < n; i++) max_len = kv->seq[seqs[i]].len > max_len ? kv->seq[seqs[i]].len : max_len;
    const int nsplit = ((max_len + 1 + 63) / 64 + ATTN_SPLIT_TILES - 1) / ATTN_SPLIT_TILES;
    DecodeBufs b(c, lw->ff, kv, n, nsplit, kv_scan_rows(kv, seqs, n, penalty));
    CR_TRY(ws_carve(c, "cr_llm_decode", b));
    CR_TRY(ctx_stage_seqs(c, seqs, n, st, false));
    if (b.head.f.shares) {      // the groups of this launch, from the host's mirrors; sent again only when the rows or a share have changed
        std::vector<int32_t> psrc(n), plen(n), table;
        for (int i = 0; i < n; i++) { psrc[i] = kv->seq[seqs[i]].pfx_src; plen[i] = kv->seq[seqs[i]].pfx_len; }
        b.share_n = attn_share_table(seqs, psrc.data(), plen.data(), n, table, &b.share_splits);
        CR_TRY(ctx_stage_share(c, table, st));
        b.share = c->d_share;
    }
    const int32_t* d_seqs = c->d_seqs;
    hipLaunchKernelGGL(embed_rows_kernel<false>, dim3(n), dim3(256), 0, st, lw->embed, force_tokens, d_seqs, kv->d_gen, kv->d_ngen, kv->gen_cap, b.x, nullptr);
    CR_TRY(decode_layers(c, *lw, kv, b, d_seqs, st));
    CR_TRY(decode_head(c, *lw, b, st));
    CR_TRY(pick_rows(kv, b.head, d_seqs, penalty, 1, logits, st, false));
    if (beam_span > 0)
        CR_TRY(launch_beam_reorder(b.head.rows(d_seqs, penalty), kv_seq_state(kv), beam_launch(kv, b.head, 1, 0), beam_cache(kv), beam_firsts.data(),
                                   (int)beam_firsts.size(), beam_span, 1, st));
    CR_HIP(hipGetLastError());
    for (int i = 0; i < n; i++) {
        Seq& q = kv->seq[seqs[i]];
        q.len += 1;
        if (q.ngen < kv->gen_cap) q.ngen += 1;
    }
    return CR_OK;
}

int cr_llm_decode_draft(cr_ctx* c, cr_kv* kv, const int32_t* seqs, int n, const int64_t* draft_host, const int32_t* draft_lens_host, int draft_stride,
                        float penalty, int32_t* appended_host, void* stream) {
    if (!c || !kv || !seqs || !draft_lens_host || !appended_host || n <= 0 || n > kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: bad argument");
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "cr_llm_decode_draft: call cr_finalize first");
    CR_TRY(ctx_share_ok(c, "cr_llm_decode_draft"));
    const LlmWeights* lw;
    CR_TRY(llm_weights(c, &lw));
    const int V = c->d.vocab;
    int M = 0, max_keys = 0;
    bool deep = false;
    for (int i = 0; i < n; i++) {
        const int s = seqs[i], k = draft_lens_host[i];
        if (s < 0 || s >= kv->n_seqs) return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: sequence %d out of range", s);
        for (int j = 0; j < i; j++) if (seqs[j] == s) return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: sequence %d listed twice", s);
        if (k < 0 || k > DRAFT_MAX) return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: %d drafted ids for sequence %d (want 0..%d)", k, s, DRAFT_MAX);
        if (k > 0 && (!draft_host || draft_stride < k)) return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: %d drafted ids for sequence %d, but no draft array of that stride", k, s);
        const Seq& q = kv->seq[s];
        if (q.len + k + 1 > kv->max_tokens || q.ngen + k + 1 > kv->gen_cap)
            return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: sequence %d holds %d tokens, %d more exceed the cache (%d)", s, q.len, k + 1, kv->max_tokens);
        for (int j = 0; j < k; j++) {
            const int64_t id = draft_host[(size_t)i * draft_stride + j];
            if (id < 0 || id >= V) return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: drafted id %lld of sequence %d outside the vocabulary (%d)", (long long)id, s, V);
        }
        M += k + 1;
        max_keys = std::max(max_keys, q.len + k + 1);
        deep |= penalty != 1.0f && q.ngen + k > 4096;
    }
    if (M > DRAFT_MAX_ROWS)
        return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: %d rows in all (sequences + drafted ids; at most %d: the decode forms whose bits do not depend on the batch)", M,
                       DRAFT_MAX_ROWS);
    if (kv->fmt != CR_KV_BF16)
        return cr_fail(CR_ERR_ARG, "cr_llm_decode_draft: an e4m3 cache (left out: the window's rows are written by the bf16 RoPE + split forms only)");
    for (int i = 0; i < n; i++) {
        const Seq& q = kv->seq[seqs[i]];
        if (q.ngen == 0) return cr_fail(CR_ERR_STATE, "cr_llm_decode_draft: sequence %d has no generated id to feed", seqs[i]);
        // left out, each for its own reason: a sampled pick is a draw, not a comparison; scores and constraints are per appended id and would have to be redone for
        // the accepted prefix; a beam group's step re-orders the cache
        if (q.sampled) return cr_fail(CR_ERR_STATE, "cr_llm_decode_draft: sequence %d samples (greedy rows only)", seqs[i]);
        if (q.scored) return cr_fail(CR_ERR_STATE, "cr_llm_decode_draft: sequence %d records token scores (not with drafts)", seqs[i]);
        if (q.constrained) return cr_fail(CR_ERR_STATE, "cr_llm_decode_draft: sequence %d has logits constraints (not with drafts)", seqs[i]);
        if (q.bgrp >= 0) return cr_fail(CR_ERR_STATE, "cr_llm_decode_draft: sequence %d belongs to the beam group of sequence %d (not with drafts)", seqs[i], q.bgrp);
        CR_TRY(kv_refuse_sharer(kv, seqs[i], "cr_llm_decode_draft", "a draft window's rows take the per-row attention forms only; draft on an unshared copy (cr_kv_fork)"));
    }
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const int nsplit = ((max_keys + 63) / 64 + ATTN_SPLIT_TILES - 1) / ATTN_SPLIT_TILES;
    RowFeatures feat{};
    feat.deep = deep;                       // histories of more than 4096 ids under a penalty: the pick reads an untouched copy of the rows, as pick_rows does
    DraftBufs b(c, lw->ff, kv, M, n, nsplit, feat);
    CR_TRY(ws_carve(c, "cr_llm_decode_draft", b));
    // the rows: sequence i's window is rows row0[i] .. row0[i] + k_i, all naming its cache slot
    std::vector<int32_t> row_seq(M);
    std::vector<int64_t> hix(draft_index_host_words(n, M), 0);
    const DraftIndex hx = draft_index(hix.data(), n, M);
    for (int i = 0, r = 0; i < n; i++) {
        const int k = draft_lens_host[i];
        hx.row0[i] = r; hx.klen[i] = k;
        for (int j = 0; j < k; j++) hx.ids[i * DRAFT_MAX + j] = draft_host[(size_t)i * draft_stride + j];
        for (int j = 0; j <= k; j++, r++) { row_seq[r] = seqs[i]; hx.off[r] = j; }
    }
    CR_HIP(hipMemcpyAsync(b.index, hix.data(), hix.size() * 8, hipMemcpyHostToDevice, st));      // pageable source: staged before return
    CR_TRY(ctx_stage_seqs(c, row_seq.data(), M, st, false));
    const int32_t* d_seqs = c->d_seqs;
    const Rows rows = b.dec.head.rows(d_seqs, penalty);
    const SeqState ss = kv_seq_state(kv);
    const DraftLaunch dl{n, draft_index(b.index, n, M), b.windows};
    CR_TRY(launch_draft_stage(rows, ss, dl, st));
    if (b.dec.off)
        hipLaunchKernelGGL(embed_rows_kernel<true>, dim3(M), dim3(256), 0, st, lw->embed, (const int64_t*)nullptr, d_seqs, kv->d_gen, kv->d_ngen, kv->gen_cap, b.dec.x, b.dec.off);
    else
        hipLaunchKernelGGL(embed_rows_kernel<false>, dim3(M), dim3(256), 0, st, lw->embed, (const int64_t*)nullptr, d_seqs, kv->d_gen, kv->d_ngen, kv->gen_cap, b.dec.x, nullptr);
    CR_TRY(decode_layers(c, *lw, kv, b.dec, d_seqs, st));
    CR_TRY(decode_head(c, *lw, b.dec, st));
    if (rows.orig) CR_HIP(hipMemcpyAsync(b.dec.head.lg0, b.dec.head.lg, (size_t)M * V * 4, hipMemcpyDeviceToDevice, st));
    CR_TRY(launch_draft_pick_accept(rows, ss, dl, st));
    CR_HIP(hipGetLastError());
    // the price of a variable step: the host's mirror of the lengths needs the counts, and the next window depends on them anyway
    CR_HIP(hipMemcpyAsync(appended_host, dl.ix.app, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CR_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        Seq& q = kv->seq[seqs[i]];
        q.len += appended_host[i];
        q.ngen += appended_host[i];
    }
    return CR_OK;
}

}  // extern "C"

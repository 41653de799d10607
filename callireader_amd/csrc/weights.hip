// The weight map and what is derived from it (weights.hpp): the only code that writes cr_ctx::w.  The map's access functions and the kinds of copy, the
// resolved table of the language model's weights, and weight preparation: w1|w3 interleaved, the decode layouts, the e4m3 copies.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "decode.hpp"
#include "kv.hpp"
#include "weights.hpp"

namespace {

// w13 rows: [16q + e] = w1[8q + e], [16q + 8 + e] = w3[8q + e]   (pairs gate/up for the SwiGLU epilogue)
__global__ __launch_bounds__(256) void interleave8_kernel(const bf16* __restrict__ w1, const bf16* __restrict__ w3,
                                                          bf16* __restrict__ out, int ff) {
    const int r = blockIdx.x;                 // output row, 0 .. 2*ff
    const int q = r >> 4, e = r & 15;
    const bf16* src = (e < 8 ? w1 : w3) + (int64_t)(q * 8 + (e & 7)) * D;
    const bf16x8* sp = (const bf16x8*)src;
    bf16x8* dp = (bf16x8*)(out + (int64_t)r * D);
    dp[threadIdx.x] = sp[threadIdx.x];
    dp[threadIdx.x + 256] = sp[threadIdx.x + 256];
}

// One weight row -> e4m3 bytes + its scale (common.hpp's e4m3 row rule): q = round-to-nearest-even (w / scale).  One workgroup per row, K % 8 == 0.
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const bf16* __restrict__ w, int64_t ldw, int K, unsigned char* __restrict__ q,
                                                              float* __restrict__ scale) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const bf16* wr = w + r * ldw;
    float mx = 0.f;
    for (int k = tid * 8; k < K; k += 256 * 8) {
        const bf16x8 v = *(const bf16x8*)(wr + k);
#pragma unroll
        for (int e = 0; e < 8; e++) mx = fmaxf(mx, fabsf(bf2f(v[e])));
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = e4m3_row_scale(mx);
    const float inv = 1.0f / sc;
    if (tid == 0) scale[r] = sc;
    for (int k = tid * 8; k < K; k += 256 * 8) *(uint2*)(q + r * (int64_t)K + k) = pack8_e4m3(*(const bf16x8*)(wr + k), inv);
}

// out[0] = max over rows of ||w_row||_2, out[1] = max |b| (positive floats order like their bit patterns: atomicMax on the bits)
__global__ __launch_bounds__(256) void row_norm_max_kernel(const bf16* __restrict__ w, int K, const bf16* __restrict__ b, float* __restrict__ out) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const bf16* wr = w + (int64_t)blockIdx.x * K;
    float ss = 0.f;
    for (int k = tid; k < K; k += 256) { const float v = bf2f(wr[k]); ss += v * v; }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) {
        atomicMax((unsigned*)out, __float_as_uint(sqrtf(red[0] + red[1] + red[2] + red[3])));
        if (b) atomicMax((unsigned*)out + 1, __float_as_uint(fabsf(bf2f(b[blockIdx.x]))));
    }
}

// The kinds of copy: the prefix each is filed under, and whether it is part of an fp8 option (losing one switches the options off)
constexpr struct { const char* prefix; bool e4m3; } KIND[COPY_KINDS] = {
    {"declayout.", false}, {"fp8.", true}, {"fp8s.", true}, {"fp8b.", true}, {"fp8dl.", true}};
// A copy that depends on a second tensor besides the one it is named after: the tensor ending in `on` also invalidates the copy of kind k of its sibling `of`
constexpr struct { CopyKind k; const char *on, *of; } ALSO_ON[] = {
    {COPY_FP8_BOUND, "mlp.fc1.bias", "mlp.fc1.weight"}};      // fc1's bound = {max row norm of W1, max |b1|}

std::string copy_name(CopyKind k, const std::string& name) { return KIND[k].prefix + name; }

// The names of the language model's tensors: all the string work of the LLM stage is in this file
const char *const EMBED = "language_model.model.tok_embeddings.weight", *const HEAD = "language_model.output.weight";
std::string layer_prefix(int l) { return "language_model.model.layers." + std::to_string(l) + "."; }
std::string w13_name(int l) { return "derived.w13." + std::to_string(l); }
// the LLM's linears in DecodeGemm's order per layer (wqkv, wo, w1|w3, w2), then the LM head
struct LlmLinear { int which; std::string name; int64_t N, K; };
std::vector<LlmLinear> llm_linears(const cr_ctx* c, int64_t ff) {
    std::vector<LlmLinear> v;
    for (int l = 0; l < c->d.llm_layers; l++) {
        const std::string p = layer_prefix(l);
        v.push_back({DEC_WQKV, p + "attention.wqkv.weight", QKV, D}); v.push_back({DEC_WO, p + "attention.wo.weight", D, D});
        v.push_back({DEC_W13, w13_name(l), 2 * ff, D}); v.push_back({DEC_W2, p + "feed_forward.w2.weight", D, ff});
    }
    v.push_back({DEC_HEAD, HEAD, c->d.vocab, D});
    return v;
}

bool decode_layout_wanted() { const char* e = getenv("CR_DECODE_LAYOUT"); return !(e && atoi(e) == 0); }      // CR_DECODE_LAYOUT=0: none (A/B aid)

// All or nothing: the decode layout of each of `lin` as its copy of kind k -- of the bf16 tensor, for gemm_decode.hip's `which` (COPY_DECLAYOUT: the shapes the kernels
// are built for), or of its e4m3 bytes (COPY_FP8_DECLAYOUT: one that is there stays).  When one fails every copy of the kind goes (a partial set would leave the
// device nearly full and the decode path on two layouts): false, and `freed` gets their bytes.
bool build_decode_layouts(cr_ctx* c, CopyKind k, const std::vector<LlmLinear>& lin, hipStream_t st, size_t* freed = nullptr) {
    const bool e8 = k == COPY_FP8_DECLAYOUT;
    for (const LlmLinear& x : lin) {
        const DevTensor* src = e8 ? w_copy(c, COPY_FP8, x.name) : w_find(c, x.name);
        const bool mat = src && src->shape.size() == 2;
        if (e8 ? w_copy(c, k, x.name) != nullptr : (x.which == DEC_HEAD && !(mat && src->shape[1] == D))) continue;      // built already / no LM head of this width
        bool ok = mat && (e8 || x.which == DEC_HEAD || (src->shape[0] == x.N && src->shape[1] == x.K));
        if (ok) {
            const int N = (int)src->shape[0], K = (int)src->shape[1];
            DevTensor* t = w_put(c, copy_name(k, x.name), e8 ? CR_U8 : CR_BF16, {(N + 15) / 16 * 16, K}, e8 ? decode_swizzled8_bytes(N, K) : decode_swizzled_bytes(N, K));
            ok = t && (e8 ? decode_swizzle_weight8((const unsigned char*)src->ptr, K, N, K, (unsigned char*)t->ptr, st)
                          : decode_swizzle_weight(x.which, (const bf16*)src->ptr, K, N, K, (bf16*)t->ptr, st)) == CR_OK;
        }
        if (ok) continue;
        const size_t b = w_drop_kind(c, k);
        if (freed) *freed = b;
        return false;
    }
    return true;
}

}  // namespace

const DevTensor* w_find(const cr_ctx* c, const std::string& name) {
    auto it = c->w.find(name);
    return it == c->w.end() ? nullptr : &it->second;
}
const DevTensor* w_copy(const cr_ctx* c, CopyKind k, const std::string& name) { return w_find(c, copy_name(k, name)); }

DevTensor* w_put(cr_ctx* c, const std::string& name, int dtype, std::vector<int64_t> shape, size_t bytes) {
    c->llm.reset();
    DevTensor& t = c->w[name];
    if (t.bytes != bytes) {
        if (t.ptr) hipFree(t.ptr);
        t.ptr = nullptr; t.bytes = 0;
        if (hipMalloc(&t.ptr, (bytes + 255) & ~(size_t)255) != hipSuccess) { (void)hipGetLastError(); c->w.erase(name); return nullptr; }
        t.bytes = bytes;
    }
    t.dtype = dtype; t.shape = std::move(shape);
    return &t;
}

bool w_drop(cr_ctx* c, const std::string& name) {
    auto it = c->w.find(name);
    if (it == c->w.end()) return false;
    c->llm.reset();
    hipFree(it->second.ptr);
    c->w.erase(it);
    return true;
}

bool w_drop_copies(cr_ctx* c, const std::string& name) {
    bool had8 = false;
    for (int k = 0; k < COPY_KINDS; k++) had8 |= w_drop(c, copy_name((CopyKind)k, name)) && KIND[k].e4m3;
    for (const auto& a : ALSO_ON) {
        const size_t n = strlen(a.on);
        if (name.size() >= n && name.compare(name.size() - n, n, a.on) == 0) had8 |= w_drop(c, copy_name(a.k, name.substr(0, name.size() - n) + a.of)) && KIND[a.k].e4m3;
    }
    if (had8) { c->fp8_decode = false; c->fp8_mfma = 0; }
    return had8;
}

size_t w_drop_kind(cr_ctx* c, CopyKind k) {
    c->llm.reset();
    size_t freed = 0;
    for (auto it = c->w.begin(); it != c->w.end();) {
        if (it->first.rfind(KIND[k].prefix, 0) != 0) { ++it; continue; }
        freed += it->second.bytes; hipFree(it->second.ptr);
        it = c->w.erase(it);
    }
    return freed;
}

const bf16* llm_embed_table(cr_ctx* c) { return W(c, EMBED); }

int llm_weights(cr_ctx* c, const LlmWeights** out) {
    if (!c->llm) {
        bool ok = true;      // W / WT name the tensor they miss in the error message: nothing is looked up after the first miss
        auto ptr = [&](const std::string& nm) { const bf16* p = ok ? W(c, nm) : nullptr; ok = ok && p; return p; };
        auto lin = [&](const std::string& nm, int N, int K, int dl_kind = 1) -> LinW {
            auto cp = [&](CopyKind k) -> const void* { const DevTensor* t = w_copy(c, k, nm); return t ? t->ptr : nullptr; };
            return {ptr(nm), N, K, (const bf16*)cp(COPY_DECLAYOUT), dl_kind, (const unsigned char*)cp(COPY_FP8), (const float*)cp(COPY_FP8_SCALE), (const unsigned char*)cp(COPY_FP8_DECLAYOUT)};
        };
        auto t = std::make_shared<LlmWeights>();
        t->embed = ptr(EMBED); t->cosT = ptr("rope.cos"); t->sinT = ptr("rope.sin"); t->norm = ptr("language_model.model.norm.weight");
        t->head = lin(HEAD, c->d.vocab, D);
        const DevTensor* w13_0 = ok ? WT(c, w13_name(0)) : nullptr;      // (cr_finalize interleaves w1 and w3 into it)
        if (!w13_0) return CR_ERR_STATE;
        t->ff = (int)w13_0->shape[0] / 2;
        for (int l = 0; l < c->d.llm_layers; l++) {
            const std::string p = layer_prefix(l);
            t->layer.push_back({ptr(p + "attention_norm.weight"), ptr(p + "ffn_norm.weight"), lin(p + "attention.wqkv.weight", QKV, D, 2),
                                lin(p + "attention.wo.weight", D, D), lin(w13_name(l), 2 * t->ff, D), lin(p + "feed_forward.w2.weight", D, t->ff)});
        }
        if (!ok) return CR_ERR_STATE;
        c->llm = t;
    }
    *out = c->llm.get();
    return CR_OK;
}

void launch_quant_fp8_rows(const bf16* w, int64_t ldw, int rows, int K, unsigned char* q, float* scale, hipStream_t st) {
    hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, w, ldw, K, q, scale);
}

int build_fp8_copy(cr_ctx* c, const std::string& nm, int k_multiple, hipStream_t st) {
    const DevTensor* src = WT(c, nm);
    if (!src) return CR_ERR_STATE;
    const int64_t N = src->shape[0], K = src->shape[1];
    if ((K % k_multiple) != 0) return cr_fail(CR_ERR_ARG, "fp8 copy: %s has K = %lld, not a multiple of %d", nm.c_str(), (long long)K, k_multiple);
    const DevTensor* have = w_copy(c, COPY_FP8, nm);
    if (have && have->shape == src->shape && w_copy(c, COPY_FP8_SCALE, nm)) return CR_OK;     // built already for these weights
    DevTensor* q = w_put(c, copy_name(COPY_FP8, nm), CR_U8, src->shape, (size_t)N * K);
    DevTensor* s = q ? w_put(c, copy_name(COPY_FP8_SCALE, nm), CR_F32, {N}, (size_t)N * 4) : nullptr;
    if (!s) { w_drop(c, copy_name(COPY_FP8, nm)); return cr_fail(CR_ERR_NOMEM, "fp8 copy: %s", nm.c_str()); }
    launch_quant_fp8_rows((const bf16*)src->ptr, K, (int)N, (int)K, (unsigned char*)q->ptr, (float*)s->ptr, st);
    return CR_OK;
}

int llm_finalize(cr_ctx* c, hipStream_t st) {
    for (int l = 0; l < c->d.llm_layers; l++) {
        const std::string p = layer_prefix(l) + "feed_forward.", dn = w13_name(l);
        const DevTensor *w1 = w_find(c, p + "w1.weight"), *w3 = w_find(c, p + "w3.weight");
        if (!w1 || !w3) {
            // one of the pair reloaded without the other: the interleaved tensor cannot be rebuilt (the other original was released)
            if (w1 || w3) return cr_fail(CR_ERR_STATE, "layer %d: reload feed_forward.w1 and w3 together", l);
            if (w_find(c, dn)) continue;          // already derived, originals released
            return cr_fail(CR_ERR_STATE, "layer %d: w1/w3 missing", l);
        }
        const int ff = (int)w1->shape[0];
        if (w1->shape[1] != D || w3->shape != w1->shape || (ff % 8)) return cr_fail(CR_ERR_ARG, "layer %d: w1/w3 must be [ff,4096] with ff %% 8 == 0", l);
        // the copies made from the interleaved tensor carry ITS name, not w1's / w3's: the reload of w1 / w3 could not take them along, so they go now
        w_drop_copies(c, dn);
        DevTensor* t = w_put(c, dn, CR_BF16, {2 * ff, D}, (size_t)2 * ff * D * 2);
        if (!t) return cr_fail(CR_ERR_NOMEM, "layer %d: the interleaved w1|w3", l);
        hipLaunchKernelGGL(interleave8_kernel, dim3(2 * ff), dim3(256), 0, st, (const bf16*)w1->ptr, (const bf16*)w3->ptr, (bf16*)t->ptr, ff);
        CR_HIP(hipStreamSynchronize(st));
        w_drop(c, p + "w1.weight"); w_drop(c, p + "w3.weight");      // the interleaved copy replaces them
    }
    // Decode-layout copies of the five weight streams of a small-batch decode step (gemm_decode.hip: one contiguous KiB per load instruction instead of
    // 16 rows x 64 bytes; wqkv 16.7 -> 11.1 us, w1|w3 43.1 -> 37.5, w2 26.0 -> 20.5, LM head 130 -> 116 at one row, the same bits): +15.9 GB on
    // InternLM2.5-7B, only if the shapes are the ones the kernels are built for.  A failed allocation leaves the decode path on the nn.Linear layout.
    w_drop_kind(c, COPY_DECLAYOUT);               // copies of an earlier cr_finalize: the weights may have been reloaded
    const DevTensor* w13_0 = WT(c, w13_name(0));
    if (decode_layout_wanted() && w13_0 && decode_fused_supported(1, (int)w13_0->shape[0] / 2)) {
        size_t freed = 0;
        if (!build_decode_layouts(c, COPY_DECLAYOUT, llm_linears(c, w13_0->shape[0] / 2), st, &freed))
            fprintf(stderr, "[callireader_hip] no room (or not the shapes) for the decode-layout copies of the LLM weights: %zu MB released, decode streams the nn.Linear layout\n", freed >> 20);
    }
    CR_HIP(hipStreamSynchronize(st));
    return CR_OK;
}

extern "C" {

int cr_op_quantize_fp8(const void* w, int64_t ldw, int N, int K, void* q, float* scale, void* stream) {
    if (!w || !q || !scale || N <= 0 || K <= 0 || (K & 7) || (ldw & 7)) return cr_fail(CR_ERR_ARG, "cr_op_quantize_fp8: bad argument");
    launch_quant_fp8_rows((const bf16*)w, ldw, N, K, (unsigned char*)q, scale, (hipStream_t)stream);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int cr_enable_fp8_mfma(cr_ctx* c, int enable, void* stream) {
    if (!c) return cr_fail(CR_ERR_ARG, "cr_enable_fp8_mfma: null context");
    if (!enable) { if (c->fp8_mfma) cr_bump_gen(c); c->fp8_mfma = 0; return CR_OK; }      // borrowers of these weights watch weight_gen (ctx_share_ok)
    if (c->borrowed) return cr_fail(CR_ERR_STATE, "cr_enable_fp8_mfma: enable it on the context that owns the weights, then share again");
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "cr_enable_fp8_mfma: call cr_finalize first");
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<std::string> names;
    // the linears whose input is a norm's output: that kernel emits the e4m3 row and its scale for free
    for (int l = 0; l < c->d.vit_layers; l++) {
        const std::string p = "vision_model.encoder.layers." + std::to_string(l) + ".", fc1 = p + "mlp.fc1.weight";
        if (!w_find(c, p + "attn.qkv.weight")) continue;
        names.push_back(p + "attn.qkv.weight"); names.push_back(fc1); names.push_back(p + "mlp.fc2.weight");
        // fc1's output goes to fc2 as e4m3 straight from fc1's epilogue (EPI_GELU_Q8); its row scale is a bound LayerNorm 2 derives from the COPY_FP8_BOUND of fc1
        const DevTensor *w1 = WT(c, fc1), *b1 = WT(c, p + "mlp.fc1.bias");
        if (!w1 || !b1) return CR_ERR_STATE;
        if (w_copy(c, COPY_FP8_BOUND, fc1)) continue;
        DevTensor* t = w_put(c, copy_name(COPY_FP8_BOUND, fc1), CR_F32, {2}, 8);
        if (!t) return cr_fail(CR_ERR_NOMEM, "cr_enable_fp8_mfma: bound of layer %d", l);
        CR_HIP(hipMemsetAsync(t->ptr, 0, 8, st));
        hipLaunchKernelGGL(row_norm_max_kernel, dim3((unsigned)w1->shape[0]), dim3(256), 0, st, (const bf16*)w1->ptr, (int)w1->shape[1], (const bf16*)b1->ptr, (float*)t->ptr);
    }
    if (w_find(c, "mlp1.1.weight")) names.push_back("mlp1.1.weight");
    bool layer_loaded = false;      // the LLM's layers that are loaded (wo and w2: their inputs take a quantiser pass); not the LM head
    for (const LlmLinear& x : llm_linears(c, 0)) {
        if (x.which == DEC_WQKV) layer_loaded = w_find(c, x.name) != nullptr;
        if (layer_loaded && x.which != DEC_HEAD) names.push_back(x.name);
    }
    for (const std::string& nm : names) CR_TRY(build_fp8_copy(c, nm, 256, st));
    CR_HIP(hipGetLastError());
    CR_HIP(hipStreamSynchronize(st));
    c->fp8_mfma = enable >= 2 ? 2 : 1;
    cr_bump_gen(c);
    return CR_OK;
}

int cr_enable_fp8_decode(cr_ctx* c, int enable, void* stream) {
    if (!c) return cr_fail(CR_ERR_ARG, "cr_enable_fp8_decode: null context");
    if (!enable) { if (c->fp8_decode) cr_bump_gen(c); c->fp8_decode = false; return CR_OK; }
    if (c->borrowed) return cr_fail(CR_ERR_STATE, "cr_enable_fp8_decode: enable it on the context that owns the weights, then share again");
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "cr_enable_fp8_decode: call cr_finalize first");
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const std::vector<LlmLinear> lin = llm_linears(c, 0);
    for (const LlmLinear& x : lin) CR_TRY(build_fp8_copy(c, x.name, 512, st));
    // ... and each of them once more in the decode layout (gemm_decode.hip: decode_swizzle8_kernel; + 7.7 GB on InternLM2.5-7B): without it the e4m3-weight
    // decode LOST to the bf16 decode on ITS decode layout (round 4: 9.76 against 9.23 ms per 64-row step).  All or nothing.
    if (!decode_layout_wanted()) w_drop_kind(c, COPY_FP8_DECLAYOUT);
    else build_decode_layouts(c, COPY_FP8_DECLAYOUT, lin, st);
    CR_HIP(hipGetLastError());
    CR_HIP(hipStreamSynchronize(st));
    c->fp8_decode = true;
    cr_bump_gen(c);
    return CR_OK;
}

}  // extern "C"

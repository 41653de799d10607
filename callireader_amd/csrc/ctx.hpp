// Context of libcallireader_hip.so: weights (library-owned device copies), derived
// tensors, a grow-only device workspace.  Host-side C++ only; no torch types.
// The weight map is read everywhere and written in weights.hip only (weights.hpp: w_put, w_drop_*).
#pragma once
#include <atomic>
#include <deque>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/callireader_hip.h"
#include "common.hpp"

struct DevTensor {
    void* ptr = nullptr;
    size_t bytes = 0;
    int dtype = CR_BF16;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct LlmWeights;                      // weights.hpp

struct cr_ctx {
    int device = 0;
    cr_model_desc d{};
    bool finalized = false;
    int prof_mode = 0;                  // cr_profile: 1 = every GEMM launch, 2 = only the tiled class (M >= 1024): no events around the decode steps' launches
    uint64_t weight_gen = 0;            // bumped by cr_load_weight / cr_finalize / the fp8 switches: contexts that borrow these weights watch it (ctx_share_ok)
    bool fp8_decode = false;            // cr_enable_fp8_decode: batched decode streams e4m3 copies of the LLM's linear weights (half the bytes)
    int fp8_mfma = 0;                   // cr_enable_fp8_mfma level: 1 = the norm-fed linears of the ViT, the projector and the LLM prefill run e4m3 x e4m3 on the
                                        // matrix cores; 2 = also the linears whose input no norm produces (ViT fc2 via fc1's e4m3 epilogue, LLM wo / w2 via a quantiser pass)
    bf16* probe_dst = nullptr;          // cr_llm_hidden_probe: [layers + 1][probe_rows][4096] rows of the residual stream of the next prefills
    int probe_row0 = 0, probe_rows = 0;
    bool fused_decode = true;           // decode batches of <= DECODE_FUSED_MAX_ROWS (8) rows take gemm_decode.hip (six launches per layer, the same bits); CR_DECODE_FUSED=0: the separate kernels
    bool prefill_last_rows = true;      // prefill: the final decoder layer's attention / wo / w1|w3 / w2 on each page's last row only (bit-identical; CR_PREFILL_LAST_ROWS=0: all rows)
    bool no_sliced_decode = false;      // CR_NO_SLICED_DECODE=1: decode through the one-tile weight-streaming GEMMs (A/B aid)
    bool perceiver_v1 = false;          // CR_PERCEIVER_ATTN_V1=1 at cr_create: round 1's perceiver attention kernel (the bit-for-bit yardstick of the current one)
    bool fold_rope = true;              // 9..64-row decode: RoPE + split + the new token's cache row inside the attention kernel (attention_decode.hip FOLD; bit-identical); CR_DECODE_FOLD_ROPE=0 at cr_create: rope_split_kernel as its own launch
    std::unordered_map<std::string, DevTensor> w;      // loaded tensors, "derived.*" tensors and the prefixed copies of weights.hpp's CopyKind
    std::shared_ptr<LlmWeights> llm;    // the language model's weights resolved from `w` (weights.hpp llm_weights); reset by whatever writes `w`
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    bool borrowed = false;              // cr_share_weights: the tensors in `w` belong to another context (not freed here)
    // weight_gen mirrored into a cell that OUTLIVES the context (cr_destroy stores ~0 into it): a borrower keeps the cell of the context that
    // really owns the tensors (the root of a chain of cr_share_weights calls), never a pointer to the context itself
    std::shared_ptr<std::atomic<uint64_t>> gen_cell = std::make_shared<std::atomic<uint64_t>>(0);
    std::shared_ptr<std::atomic<uint64_t>> owner_cell;      // borrowed: the owning context's cell, and its value when the map was copied: a reload /
    uint64_t owner_gen = 0;             //     re-finalize / fp8 toggle / destroy of the owner frees or replaces tensors this copy still points at -> the
                                        //     stage entry points refuse to run (ctx_share_ok)
    // the seqs[] of the last prefill / decode call (ctx_stage_seqs); per context, so that two contexts sharing weights can work on one KV cache
    int32_t* d_seqs = nullptr;
    int d_seqs_cap = 0;
    std::vector<int32_t> seqs_on_device;   // what d_seqs holds
    struct SeqStage { int32_t* host = nullptr; int cap = 0; hipEvent_t copied = nullptr; };   // pinned source of one staging copy, and its completion
    static constexpr int SEQ_STAGES = 8;
    SeqStage seq_stage[SEQ_STAGES];
    int seq_stage_next = 0;
    // the share table of the last decode call with shared prompts (ctx_stage_share; attention.hpp: attn_share_table), staged as the seqs[] are
    int32_t* d_share = nullptr;
    int d_share_cap = 0;
    std::vector<int32_t> share_on_device;  // what d_share holds
    SeqStage share_stage[SEQ_STAGES];
    int share_stage_next = 0;
    // small persistent device scratch (counters, argmax partials)
    char* scratch = nullptr;
    size_t scratch_bytes = 0;
    // measurement (cr_profile): event pairs around GEMM launches
    bool prof = false;
    struct ProfRec { hipEvent_t a, b; double flops, bytes; int big; };
    std::deque<ProfRec> prof_recs;      // launches whose events have not been read back yet (bounded: see ctx_gemm)
    std::vector<hipEvent_t> prof_pool;
    double prof_acc[2][4] = {};         // [tiled M >= 1024 | the rest][launches, ms, flops, bytes] of the retired records
    int64_t prof_issued = 0, prof_retired = 0, prof_lost = 0, prof_peak_pending = 0;
};

inline void cr_bump_gen(cr_ctx* c) { c->weight_gen++; c->gen_cell->store(c->weight_gen, std::memory_order_release); }


// CR_OK, or CR_ERR_STATE when this context borrows weights whose owner has changed them since cr_share_weights
int ctx_share_ok(const cr_ctx* c, const char* who);

// GEMM launch used by every stage: validates, launches, and (when profiling) brackets the launch with events.
int ctx_gemm(cr_ctx* c, int epi, const GemmParams& p, hipStream_t st);
// C = epi((A8 . W8^T) * ascale[m] * wscale[n] + bias): both operands e4m3 (gemm256's F8 instance), the weight's e4m3 copy and its row scales
int ctx_gemm_f8(cr_ctx* c, int epi, const void* a8, const float* ascale, const void* w8, const float* wscale, void* C, int64_t ldc,
                const bf16* bias, int M, int N, int K, hipStream_t st, const bf16* res = nullptr, int64_t ldr = 0);

void cr_set_error(const char* fmt, ...);
int cr_fail(int code, const char* fmt, ...);
#define CR_HIP(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return cr_fail(CR_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define CR_TRY(call)                       \
    do {                                   \
        int r_ = (call);                   \
        if (r_ != CR_OK) return r_;        \
    } while (0)

// weight lookup helpers (api.hip)
const bf16* W(cr_ctx* c, const std::string& name);
const DevTensor* WT(cr_ctx* c, const std::string& name);
int ws_ensure(cr_ctx* c, size_t bytes);
// the seqs[] of a prefill / decode call into c->d_seqs (api.hip)
int ctx_stage_seqs(cr_ctx* c, const int32_t* seqs, int n, hipStream_t st, bool always);
// the share table of a decode call into c->d_share (api.hip): copied only when it differs from what the device holds; no allocation once the capacity is there
int ctx_stage_share(cr_ctx* c, const std::vector<int32_t>& table, hipStream_t st);

// simple bump allocator over the workspace.  Without a base it only measures: the takes return null and bytes() is what they need.  With a capacity,
// a take that would pass it returns null and clears ok(); the caller checks ok() before it launches anything (ws_carve below).  A caller that
// passes no capacity (the other stages, which size the workspace by their own formulas) gets no check.
struct Arena {
    char* base; size_t cap; size_t off = 0; bool fits = true;
    explicit Arena(char* b = nullptr, size_t capacity = ~(size_t)0) : base(b), cap(capacity) {}
    template <typename T> T* take(size_t n) {
        const size_t at = (off + 255) & ~(size_t)255;
        off = at + n * sizeof(T);
        if (off > cap) fits = false;
        return base && fits ? (T*)(base + at) : nullptr;
    }
    size_t bytes() const { return off; }
    bool ok() const { return fits; }
};

// Runs the call's carve twice: on an Arena without a base to measure what the call needs, then -- the workspace grown to that -- on the workspace itself.
// The bytes reserved and the pointers handed out come from the same takes.
template <class Bufs> int ws_carve(cr_ctx* c, const char* who, Bufs& b) {
    Arena measure;
    b.carve(measure);
    CR_TRY(ws_ensure(c, measure.bytes()));
    Arena ar(c->ws, c->ws_bytes);
    b.carve(ar);
    return ar.ok() ? CR_OK : cr_fail(CR_ERR_STATE, "%s: the carve passed the %zu bytes of workspace (%zu measured)", who, c->ws_bytes, measure.bytes());
}

// CalliAlign stage: PerceiverResampler, cosine VQ, de-normalisation.
//   reference: models/perceiver_resampler.py:8-100,130-141; models/similarity.py:9-27;
//              InternVL/modeling_internvl_chat.py:602-640
#include "weights.hpp"
#include "calli.hpp"
#include "misc.hpp"
#include "norm.hpp"

namespace {

constexpr int D = 4096, NQ = 3, NKV = 259, INNER = 512, HEADS = 8, DH = 64;

// learns[t*3 + i][:] = resampler.learns[i][:]      (perceiver_resampler.py:92)
__global__ __launch_bounds__(256) void bcast_rows_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, int rows_src, int64_t rows_dst) {
    const int64_t r = blockIdx.x;
    if (r >= rows_dst) return;
    const bf16x8* s = (const bf16x8*)(src + (int64_t)(r % rows_src) * D);
    bf16x8* d = (bf16x8*)(dst + r * D);
    d[threadIdx.x] = s[threadIdx.x];
    d[threadIdx.x + 256] = s[threadIdx.x + 256];
}

// Round 1's form, kept as the bit-for-bit yardstick of the kernel below (CR_PERCEIVER_ATTN_V1=1 at cr_create; tests/test_gpu_calli.py): fully unrolled, hipcc hoists
// the 192 LDS reads of q and all 40 key loads together -- 512 registers and 448 scratch instructions, 235 us per 252-tile launch.
// One wave per (tile, head): 3 queries x 259 keys x 64 dims, with the reference's exact rounding sequence
// (perceiver_resampler.py:43-51): q*scale (bf16, exact), sim -> bf16, sim - amax -> bf16, softmax -> bf16, attn@v -> bf16.
__global__ __launch_bounds__(64) void perceiver_attn_v1_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kv,
                                                            bf16* __restrict__ out, float scale) {
    __shared__ float qs[NQ][DH];
    __shared__ float ps[NQ][320];
    const int t = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NQ; i++) qs[i][lane] = rbf(bf2f(q[((int64_t)t * NQ + i) * INNER + h * DH + lane]) * scale);
    __syncthreads();
    const bf16* kb = kv + (int64_t)t * NKV * (2 * INNER) + h * DH;
    const bf16* vb = kb + INNER;
    float s[NQ][5];
    float mx[NQ] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kk = 0; kk < 5; kk++) {
        const int key = lane + 64 * kk;
        const bool ok = key < NKV;
        const bf16* kr = kb + (int64_t)(ok ? key : 0) * (2 * INNER);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const bf16x8 kc = *(const bf16x8*)(kr + c * 8);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float kf = bf2f(kc[e]);
                a0 += qs[0][c * 8 + e] * kf; a1 += qs[1][c * 8 + e] * kf; a2 += qs[2][c * 8 + e] * kf;
            }
        }
        s[0][kk] = ok ? rbf(a0) : -INFINITY; s[1][kk] = ok ? rbf(a1) : -INFINITY; s[2][kk] = ok ? rbf(a2) : -INFINITY;
#pragma unroll
        for (int i = 0; i < NQ; i++) mx[i] = fmaxf(mx[i], s[i][kk]);
    }
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const float m = wave_max(mx[i]);
        float e[5], sum = 0.f;
#pragma unroll
        for (int kk = 0; kk < 5; kk++) {
            const float d = rbf(s[i][kk] - m);            // sim - amax in bf16; its own max is exactly 0
            e[kk] = (lane + 64 * kk < NKV) ? __expf(d) : 0.f;
            sum += e[kk];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int kk = 0; kk < 5; kk++) ps[i][lane + 64 * kk] = rbf(e[kk] / sum);
    }
    __syncthreads();
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    for (int key = 0; key < NKV; key++) {
        const float vf = bf2f(vb[(int64_t)key * (2 * INNER) + lane]);
        o0 += ps[0][key] * vf; o1 += ps[1][key] * vf; o2 += ps[2][key] * vf;
    }
    bf16* ob = out + (int64_t)t * NQ * INNER + h * DH + lane;
    ob[0] = f2bf(o0); ob[INNER] = f2bf(o1); ob[2 * INNER] = f2bf(o2);
}

// PerceiverAttention's softmax(q k^T) v for one (tile, head) per wave: 3 queries x 259 keys x 64 dims, with the reference's exact rounding sequence
// (perceiver_resampler.py:43-51): q*scale (bf16, exact), sim -> bf16, sim - amax -> bf16, softmax -> bf16, attn@v -> bf16.
// Every fp32 sum is formed in the order of perceiver_attn_v1_kernel (a score = the fused multiply-adds over dims 0..63 in ascending order, the row sum = a lane's
// keys lane + 64 kk in ascending kk then the wave butterfly, an output = the fused multiply-adds over keys 0..258 in ascending order): the same bits.  What changed
// is what is in flight (round-5 verdict, item 6: the one kernel of the path that spilled inside its body):
//   * the dims loop is the OUTER loop and a real one: per 8-dim chunk three q values at a time from LDS (broadcast) feed the fifteen (query, key) chains of a lane's
//     five keys, the next chunk's five 16-byte loads in flight underneath: no scratch;
//   * the (tile, head)'s V block (259 x 128 B) comes in ONE burst of 33 coalesced 16-byte loads per lane (requested before the softmax, which hides them) and is
//     laid into 33 KiB of LDS; the P.V loop reads its dim's value per key from there instead of issuing 259 dependent 2-byte global loads.
__global__ __launch_bounds__(64) void perceiver_attn_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kv,
                                                            bf16* __restrict__ out, float scale) {
    constexpr int KP = 264;                                   // keys padded to whole 8-key load rounds
    __shared__ float qs[NQ][DH];
    __shared__ __attribute__((aligned(16))) float ps[NQ][320];
    __shared__ __attribute__((aligned(16))) bf16 vs[KP][DH];
    const int t = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const bf16* kb = kv + (int64_t)t * NKV * (2 * INNER) + h * DH;
    const bf16* vb = kb + INNER;
    // a lane's five key rows (keys lane + 64 kk), one 8-dim chunk at a time with the next chunk's five loads in flight: a REAL loop over the chunks (fully unrolled,
    // hipcc kept all 320 converted key values and the 192 q values live: 512 registers + scratch)
    const bf16* krow[5];
#pragma unroll
    for (int kk = 0; kk < 5; kk++) krow[kk] = kb + (int64_t)(lane + 64 * kk < NKV ? lane + 64 * kk : 0) * (2 * INNER);
    bf16x8 kcur[5], knext[5];
#pragma unroll
    for (int kk = 0; kk < 5; kk++) kcur[kk] = *(const bf16x8*)krow[kk];
#pragma unroll
    for (int i = 0; i < NQ; i++) qs[i][lane] = rbf(bf2f(q[((int64_t)t * NQ + i) * INNER + h * DH + lane]) * scale);
    __syncthreads();
    float a[NQ][5];
#pragma unroll
    for (int i = 0; i < NQ; i++)
#pragma unroll
        for (int kk = 0; kk < 5; kk++) a[i][kk] = 0.f;
#pragma unroll 1
    for (int c = 0; c < 8; c++) {
        const int cn = c < 7 ? c + 1 : 7;
#pragma unroll
        for (int kk = 0; kk < 5; kk++) knext[kk] = *(const bf16x8*)(krow[kk] + cn * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float q0 = qs[0][c * 8 + e], q1 = qs[1][c * 8 + e], q2 = qs[2][c * 8 + e];
#pragma unroll
            for (int kk = 0; kk < 5; kk++) {
                const float kf = bf2f(kcur[kk][e]);
                a[0][kk] += q0 * kf; a[1][kk] += q1 * kf; a[2][kk] += q2 * kf;
            }
        }
#pragma unroll
        for (int kk = 0; kk < 5; kk++) kcur[kk] = knext[kk];
    }
    // the V block: 33 rounds of (8 keys x 8 chunks of 16 bytes), requested now, stored to LDS after the softmax
    const int vkey = lane >> 3, vch = lane & 7;
    bf16x8 vr[KP / 8];
#pragma unroll
    for (int r = 0; r < KP / 8; r++) {
        const int key = r * 8 + vkey;
        vr[r] = *(const bf16x8*)(vb + (int64_t)(key < NKV ? key : NKV - 1) * (2 * INNER) + vch * 8);
    }
    float s[NQ][5];
    float mx[NQ] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kk = 0; kk < 5; kk++) {
        const bool ok = lane + 64 * kk < NKV;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            s[i][kk] = ok ? rbf(a[i][kk]) : -INFINITY;
            mx[i] = fmaxf(mx[i], s[i][kk]);
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const float m = wave_max(mx[i]);
        float e[5], sum = 0.f;
#pragma unroll
        for (int kk = 0; kk < 5; kk++) {
            const float d = rbf(s[i][kk] - m);            // sim - amax in bf16; its own max is exactly 0
            e[kk] = (lane + 64 * kk < NKV) ? __expf(d) : 0.f;
            sum += e[kk];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int kk = 0; kk < 5; kk++) ps[i][lane + 64 * kk] = rbf(e[kk] / sum);
    }
#pragma unroll
    for (int r = 0; r < KP / 8; r++) *(bf16x8*)&vs[r * 8 + vkey][vch * 8] = vr[r];
    __syncthreads();
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    for (int key = 0; key < 256; key += 4) {
        const f32x4 p0 = *(const f32x4*)&ps[0][key], p1 = *(const f32x4*)&ps[1][key], p2 = *(const f32x4*)&ps[2][key];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float vf = bf2f(vs[key + j][lane]);
            o0 += p0[j] * vf; o1 += p1[j] * vf; o2 += p2[j] * vf;
        }
    }
#pragma unroll
    for (int key = 256; key < NKV; key++) {
        const float vf = bf2f(vs[key][lane]);
        o0 += ps[0][key] * vf; o1 += ps[1][key] * vf; o2 += ps[2][key] * vf;
    }
    bf16* ob = out + (int64_t)t * NQ * INNER + h * DH + lane;
    ob[0] = f2bf(o0); ob[INNER] = f2bf(o1); ob[2 * INNER] = f2bf(o2);
}

// F.normalize(x, p=2, dim=-1) on bf16 rows of 4096 (similarity.py:17-18):
//   n = bf16(sqrt(sum x^2)); y = bf16(x / max(n, 1e-12))
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const bf16* __restrict__ in, bf16* __restrict__ out, int64_t rows) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const bf16x8 a = *(const bf16x8*)(in + r * D + tid * 16), b = *(const bf16x8*)(in + r * D + tid * 16 + 8);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) { s += bf2f(a[e]) * bf2f(a[e]); s += bf2f(b[e]) * bf2f(b[e]); }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float n = fmaxf(rbf(sqrtf(red[0] + red[1] + red[2] + red[3])), 1e-12f);
    bf16x8 oa, ob;
#pragma unroll
    for (int e = 0; e < 8; e++) { oa[e] = f2bf(bf2f(a[e]) / n); ob[e] = f2bf(bf2f(b[e]) / n); }
    *(bf16x8*)(out + r * D + tid * 16) = oa;
    *(bf16x8*)(out + r * D + tid * 16 + 8) = ob;
}

// similarity.max(dim=-1) from the GEMM's per-block partials (EPI_ARGMAX: {bits(max bf16 value), column} per row and
// 64-column block): larger value first, then the smaller column -- torch's first maximal index
__global__ __launch_bounds__(256) void vq_pick_kernel(const unsigned long long* __restrict__ part, int64_t ld, int n_blk,
                                                      int64_t* __restrict__ idx, bf16* __restrict__ cosv) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    float best = -INFINITY; int besti = 0x7fffffff;
    for (int b = tid; b < n_blk; b += 256) {
        const unsigned long long u = part[r * ld + b];
        argmax_merge(best, besti, __uint_as_float((unsigned)(u >> 32)), (int)(unsigned)u);
    }
    bv[tid] = best; bi[tid] = besti;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { float v = bv[tid]; int c = bi[tid]; argmax_merge(v, c, bv[tid + o], bi[tid + o]); bv[tid] = v; bi[tid] = c; }
        __syncthreads();
    }
    if (tid == 0) { idx[r] = bi[0]; if (cosv) cosv[r] = f2bf(bv[0]); }
}

// calli_align tail (modeling_internvl_chat.py:602-640): row compaction for drop_zero (order-preserving; n is a few
// hundred, one thread scans), then one workgroup per kept row.
__global__ void denorm_index_kernel(const int64_t* __restrict__ idx, int n, int flags, int32_t* __restrict__ n_out,
                                    int32_t* __restrict__ dst_row) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int k = 0;
    for (int r = 0; r < n; r++) {
        const bool keep = !(flags & 1) || idx[r] != 0;
        dst_row[r] = keep ? k : -1;
        k += keep ? 1 : 0;
    }
    *n_out = k;
}

template <bool PARAMS_F32>
__global__ __launch_bounds__(256) void denorm_kernel(const bf16* __restrict__ x, const int64_t* __restrict__ idx,
                                                     const bf16* __restrict__ cosv, const bf16* __restrict__ table,
                                                     const void* __restrict__ mu, const void* __restrict__ sigma,
                                                     int flags, bf16* __restrict__ out, const int32_t* __restrict__ dst_row) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int dr = dst_row[r];
    if (dr < 0) return;
    const int64_t id = idx[r];
    // hard VQ: below = (cos <= 0.5); x*(1-below) + table[idx]*below selects one of the two rows (:609-614)
    const bool hard = (flags & 2) && bf2f(cosv[r]) <= 0.5f;
    const bf16* src = hard ? table + id * D : x + (int64_t)r * D;
    for (int c = tid; c < D; c += 256) {
        const float xv = bf2f(src[c]);
        float y;
        if (PARAMS_F32) y = xv * ((const float*)sigma)[id] + ((const float*)mu)[id];
        else y = rbf(xv * bf2f(((const bf16*)sigma)[id])) + bf2f(((const bf16*)mu)[id]);
        out[(int64_t)dr * D + c] = f2bf(y);
    }
}

int gemm(cr_ctx* c, int epi, const bf16* A, int64_t lda, const bf16* Wt, int64_t ldw, void* C, int64_t ldc, const bf16* bias,
         const bf16* res, int64_t ldr, int M, int N, int K, hipStream_t st, bool latent_rows = false) {
    GemmParams p{};
    p.A = A; p.lda = lda; p.W = Wt; p.ldw = ldw; p.C = C; p.ldc = ldc; p.bias = bias; p.res = res; p.ldr = ldr;
    p.M = M; p.N = N; p.K = K;
    // The latents' GEMMs have 3 rows per tile.  Up to 64 rows the dispatcher would pick the weight-streaming kernel, whose waves split K
    // (another summation order than the tiled kernels'): a tile's pseudo tokens would then depend on how many tiles share its call -- 7
    // tiles per rank against 55 in one process flipped a near-tie in scripts/dist_check.py at 8 ranks.  Pinned to the tiled kernel, whose
    // K order is the same in all its forms, a tile's result is the same in every batch and on every rank count.
    if (latent_rows && M <= 64) p.kernel = 128;
    return ctx_gemm(c, epi, p, st);
}

int ln(const bf16* in, bf16* out, const bf16* g, const bf16* b, int64_t rows, int in_group, int out_group, int out_off, hipStream_t st) {
    return launch_layernorm(regroup_norm_params(in, out, g, b, rows, D, 1e-5f, in_group, out_group, out_off), D, 0, st);      // (norm.hpp; cr_op_layernorm_regroup fills its launch there too)
}

}  // namespace

// the resampler's attention launch, made in ONE place for resample_chunk below and for the test entry cr_op_perceiver_attention (api.hip)
int launch_perceiver_attn(int which, const bf16* q, const bf16* kv, bf16* out, int T, hipStream_t st) {
    if (!q || !kv || !out || T <= 0 || (which != 0 && which != 1)) return CR_ERR_ARG;
    if (which == 1) hipLaunchKernelGGL(perceiver_attn_v1_kernel, dim3(T, HEADS), dim3(64), 0, st, q, kv, out, 0.125f);
    else hipLaunchKernelGGL(perceiver_attn_kernel, dim3(T, HEADS), dim3(64), 0, st, q, kv, out, 0.125f);
    return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
}

int calli_finalize(cr_ctx* c, hipStream_t st) {
    const DevTensor* tb = WT(c, "normed_emb.weight");
    if (!tb) return CR_ERR_STATE;
    if (tb->shape.size() != 2 || tb->shape[1] != D) return cr_fail(CR_ERR_ARG, "normed_emb.weight must be [vocab,4096]");
    DevTensor* t = w_put(c, "derived.vq_table", CR_BF16, tb->shape, tb->bytes);
    if (!t) return cr_fail(CR_ERR_NOMEM, "derived.vq_table");
    // F.normalize(embedding_weight, p=2, dim=1) is input-independent: do it once (similarity.py:18 does it per call)
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)tb->shape[0]), dim3(256), 0, st, (const bf16*)tb->ptr, (bf16*)t->ptr, tb->shape[0]);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

// Tiles are independent through the resampler: chunks of RS_CHUNK tiles bound the scratch (the normed cat(x, latents) alone
// is 2.1 MB per tile) and land the to_kv GEMM (259 rows per tile) just under a whole number of 256-CU rounds:
// 252 x 259 = 65 268 rows = 255 row tiles x 4 column tiles = 3.98 rounds.
static constexpr int RS_CHUNK = 252;

static size_t resample_ws(int T) {
    const size_t R = (size_t)T * NQ;
    return ((size_t)T * NKV * D + (size_t)T * NKV * 2 * INNER + R * D * 3 + R * INNER * 2 + R * D * 4) * 2 + 8192;
}

static int resample_chunk(cr_ctx* c, const bf16* x, int T, bf16* out, hipStream_t st) {
    const int64_t R = (int64_t)T * NQ;
    Arena ar(c->ws);
    bf16* kv_in = ar.take<bf16>((size_t)T * NKV * D);
    bf16* kv = ar.take<bf16>((size_t)T * NKV * 2 * INNER);
    bf16* learns = ar.take<bf16>((size_t)R * D);
    bf16* lnl = ar.take<bf16>((size_t)R * D);
    bf16* q = ar.take<bf16>((size_t)R * INNER);
    bf16* ao = ar.take<bf16>((size_t)R * INNER);
    bf16* ff = ar.take<bf16>((size_t)R * D * 4);

    const bf16* l0 = W(c, "resampler.learns");
    if (!l0) return CR_ERR_STATE;
    hipLaunchKernelGGL(bcast_rows_kernel, dim3((unsigned)R), dim3(256), 0, st, l0, learns, NQ, R);

    for (int l = 0; l < c->d.rs_depth; l++) {
        const std::string a = "resampler.layers." + std::to_string(l) + ".0.";
        const std::string f = "resampler.layers." + std::to_string(l) + ".1.net.";
        const bf16 *nmw = W(c, a + "norm_media.weight"), *nmb = W(c, a + "norm_media.bias");
        const bf16 *nlw = W(c, a + "norm_learns.weight"), *nlb = W(c, a + "norm_learns.bias");
        const bf16 *wq = W(c, a + "to_q.weight"), *wkv = W(c, a + "to_kv.weight"), *wo = W(c, a + "to_out.weight");
        const bf16 *fw0 = W(c, f + "0.weight"), *fb0 = W(c, f + "0.bias");
        const bf16 *fw1 = W(c, f + "1.weight"), *fb1 = W(c, f + "1.bias");
        const bf16 *fw3 = W(c, f + "3.weight"), *fb3 = W(c, f + "3.bias");
        if (!nmw || !nmb || !nlw || !nlb || !wq || !wkv || !wo || !fw0 || !fb0 || !fw1 || !fb1 || !fw3 || !fb3) return CR_ERR_STATE;

        // kv_input = cat(norm_media(x), norm_learns(learns))      (:29-30,38)
        CR_TRY(ln(x, kv_in, nmw, nmb, (int64_t)T * 256, 256, NKV, 0, st));
        CR_TRY(ln(learns, kv_in, nlw, nlb, R, NQ, NKV, 256, st));
        CR_TRY(ln(learns, lnl, nlw, nlb, R, 0, 0, 0, st));
        CR_TRY(gemm(c, EPI_STORE, lnl, D, wq, D, q, INNER, nullptr, nullptr, 0, (int)R, INNER, D, st, true));        // :35
        CR_TRY(gemm(c, EPI_STORE, kv_in, D, wkv, D, kv, 2 * INNER, nullptr, nullptr, 0, T * NKV, 2 * INNER, D, st));  // :39
        CR_TRY(launch_perceiver_attn(c->perceiver_v1 ? 1 : 0, q, kv, ao, T, st));
        CR_TRY(gemm(c, EPI_RES, ao, INNER, wo, INNER, learns, D, nullptr, learns, D, (int)R, D, INNER, st, true));    // :51 + :97
        CR_TRY(ln(learns, lnl, fw0, fb0, R, 0, 0, 0, st));                                                         // FeedForward :134
        CR_TRY(gemm(c, EPI_GELU, lnl, D, fw1, D, ff, 4 * D, fb1, nullptr, 0, (int)R, 4 * D, D, st, true));
        CR_TRY(gemm(c, EPI_RES, ff, 4 * D, fw3, 4 * D, learns, D, fb3, learns, D, (int)R, D, 4 * D, st, true));       // :98
    }
    const bf16 *nw = W(c, "resampler.norm.weight"), *nb = W(c, "resampler.norm.bias");
    if (!nw || !nb) return CR_ERR_STATE;
    CR_TRY(ln(learns, out, nw, nb, R, 0, 0, 0, st));                                                               // :100
    return CR_OK;
}

extern "C" {

int cr_resample(cr_ctx* c, const void* in, int T, void* out, void* stream) {
    if (!c || !in || !out || T <= 0) return cr_fail(CR_ERR_ARG, "cr_resample: bad argument");
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    CR_TRY(ws_ensure(c, resample_ws(T < RS_CHUNK ? T : RS_CHUNK)));
    for (int t0 = 0; t0 < T; t0 += RS_CHUNK) {
        const int tc = T - t0 < RS_CHUNK ? T - t0 : RS_CHUNK;
        CR_TRY(resample_chunk(c, (const bf16*)in + (size_t)t0 * 256 * D, tc, (bf16*)out + (size_t)t0 * NQ * D, st));
    }
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int cr_vq(cr_ctx* c, const void* in, int n, int64_t* idx, void* cosv, void* stream) {
    if (!c || !in || !idx || n <= 0) return cr_fail(CR_ERR_ARG, "cr_vq: bad argument");
    if (!c->finalized) return cr_fail(CR_ERR_STATE, "cr_vq: call cr_finalize first");
    CR_TRY(ctx_share_ok(c, "cr_vq"));
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const DevTensor* tb = WT(c, "derived.vq_table");
    if (!tb) return CR_ERR_STATE;
    const int V = (int)tb->shape[0];
    // The (n x 92 553) similarity is never written: the GEMM's epilogue keeps, per row and 64-column block, the first
    // maximum of the bf16-rounded products (EPI_ARGMAX, 8 bytes), and vq_pick_kernel merges a row's 1447 partials.
    // Rows go in chunks so that the normalised input and the partials stay under ~400 MB whatever n is.
    const int n_blk = (V + 63) / 64;
    const int64_t ldp = (n_blk + 1) & ~1;                          // 16-byte aligned rows
    const int CH = 18432;                                           // 64 pages x 96 tiles x 3 queries: 72 row tiles of 256
    const int nc = n < CH ? n : CH;
    CR_TRY(ws_ensure(c, (size_t)nc * D * 2 + (size_t)nc * ldp * 8 + 4096));
    Arena ar(c->ws);
    bf16* xn = ar.take<bf16>((size_t)nc * D);
    unsigned long long* part = ar.take<unsigned long long>((size_t)nc * ldp);
    for (int r0 = 0; r0 < n; r0 += CH) {
        const int m = n - r0 < CH ? n - r0 : CH;
        hipLaunchKernelGGL(l2norm_rows_kernel, dim3(m), dim3(256), 0, st, (const bf16*)in + (size_t)r0 * D, xn, (int64_t)m);
        CR_TRY(gemm(c, EPI_ARGMAX, xn, D, (const bf16*)tb->ptr, D, part, ldp, nullptr, nullptr, 0, m, V, D, st));
        hipLaunchKernelGGL(vq_pick_kernel, dim3(m), dim3(256), 0, st, part, ldp, n_blk, idx + r0, cosv ? (bf16*)cosv + r0 : nullptr);
    }
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int cr_denorm(cr_ctx* c, const void* in, const int64_t* idx, const void* cosv, int n, int flags, void* out,
              int32_t* n_out, void* stream) {
    if (!c || !in || !idx || !out || !n_out || n <= 0) return cr_fail(CR_ERR_ARG, "cr_denorm: bad argument");
    if ((flags & 2) && !cosv) return cr_fail(CR_ERR_ARG, "cr_denorm: hard_vq needs the cosine values");
    if ((size_t)n * 4 > c->scratch_bytes) return cr_fail(CR_ERR_ARG, "cr_denorm: n too large");
    CR_HIP(hipSetDevice(c->device));
    const DevTensor *mu = WT(c, "calli.mu"), *sg = WT(c, "calli.sigma"), *tb = WT(c, "normed_emb.weight");
    if (!mu || !sg || !tb) return CR_ERR_STATE;
    if (mu->dtype != sg->dtype) return cr_fail(CR_ERR_ARG, "calli.mu / calli.sigma dtypes differ");
    hipStream_t st = (hipStream_t)stream;
    int32_t* dst_row = (int32_t*)c->scratch;
    hipLaunchKernelGGL(denorm_index_kernel, dim3(1), dim3(64), 0, st, idx, n, flags, n_out, dst_row);
    if (mu->dtype == CR_F32)
        hipLaunchKernelGGL(denorm_kernel<true>, dim3(n), dim3(256), 0, st, (const bf16*)in, idx, (const bf16*)cosv,
                           (const bf16*)tb->ptr, mu->ptr, sg->ptr, flags, (bf16*)out, dst_row);
    else
        hipLaunchKernelGGL(denorm_kernel<false>, dim3(n), dim3(256), 0, st, (const bf16*)in, idx, (const bf16*)cosv,
                           (const bf16*)tb->ptr, mu->ptr, sg->ptr, flags, (bf16*)out, dst_row);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

}  // extern "C"

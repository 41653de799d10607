// Decode attention for gfx950: one new token per sequence over its KV cache (InternLM2 GQA: the 4 query heads of a KV group x 128, modeling_internlm2.py:393-410),
// as a STREAMING kernel on the vector pipe -- the split half of launch_flash_attn_split; the partials it writes are attn_combine_kernel's, unchanged.
//
// Why not the matrix-core kernel (attention.hip: flash_attn_kernel<128, false, true>): decode attention is a byte stream (131 KB of K / V per cached token and
// layer, 4 flops per byte).  That kernel stages 64-key tiles through two LDS buffers of 32 KB, so a CU holds two workgroups with ONE tile each in flight, and a
// split walks its four tiles behind four barriers: at 8 rows x 3 200 keys 832 workgroups move 106 MB in 25.5 us (4.2 TB/s; one row 10.3 us), and every variant
// of that structure measured the same or worse (profiles/round5/04_*: splits of two tiles requested at once, the four waves dividing the keys with a merge in
// LDS).  What bounds it is bytes in flight per CU, and LDS is what caps them.
//
// Here nothing is staged: a workgroup = one split of 256 keys of one (row, KV head), a wave = 64 of them, and a lane owns 16 bytes of every fourth key --
// lane = (key sub-index 0..3, 16-byte chunk 0..15), so one load instruction reads 4 consecutive keys = ONE contiguous KiB -- with all 16 K and 16 V loads of the
// wave issued up front (512 bytes per lane, 32 KB per wave, 256 KB per CU at two workgroups per CU: eight times the old form).  Per key: q . k for the four
// query heads by v_dot2c_f32_bf16 on the lane's 8 dimensions and four DPP rotate-adds over the 16 lanes of the key; the scores' rounding points are the
// reference's (bf16, / sqrt(128), bf16); each 16-lane group keeps ITS 16 keys' scores, so its softmax needs no running maximum (one exponential per lane and
// key: lane c computes query head c & 3, the quad shares them by DPP); P.V by fp32 FMAs on bf16-rounded probabilities.  The 16 (wave, group) partials of the
// workgroup meet in LDS and are merged in index order: a row's result depends on its own key count only, never on the batch.
//
// Everything from the scores to the partial's store is split_row (attention_decode_row.hpp), which the group form for shared prompts
// (attention_decode_group.hip: one load of a split's keys, up to 8 rows over it) inlines as well.  Registers, from hipcc's resource summary
// (-Rpass-analysis=kernel-resource-usage): per-row 190 VGPRs (FOLD: 234), group form 234, none spilled, two workgroups per CU each.
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "attention.hpp"
#include "attention_decode_row.hpp"

namespace {

constexpr int FOLD_MAX_SPLITS = 8;       // K-slices of the wqkv partial-sum GEMM the folded prologue takes (gemm_skinny.hip: partial_geom gives 2..8)

// FOLD: RoPE + split + the cache write of the new token inside this kernel (round-5 verdict, item 3: the 9..64-row decode step ran rope_split_kernel as a
// launch of its own, 6.9 us of a 13-row layer's 133).  Threads 0..95 = (slot 0..5 [4 q heads | k | v], 16-byte chunk c) of this (row, KV group) -- exactly
// rope_split_kernel's thread -- request their chunk of every K-slice BEFORE the K / V stream (loads return in order: the sums then wait for 16 loads, not for the
// stream), add the slices in slice order from 0.f, round once, and rotate with the partner chunk (c + 8) & 15 fetched by a DPP row rotation (the 16 chunks of a
// slot are one DPP row); the six bf16 rows meet in 1.5 KiB of LDS behind one barrier.  q is read from there; the workgroup whose split holds the new position also
// stores the K / V row to the cache and puts it into the registers of the lanes that would have loaded it (every lane at or past the new position: the cache row
// itself is not written yet when they load it).  The same fp32 sums, the same roundings: a row's bits do not depend on which form its batch takes.
// OFF: batch b holds p.sk_off[b] keys more than its slot's length says (cr_llm_decode_draft: the rows of one sequence's draft window sit at consecutive
// positions).  An instance of its own, so a launch without offsets runs the code it always ran; never with FOLD (a row would read cache rows that other workgroups
// of the same launch are still writing).
// SHARE: a launch some of whose rows read a shared prompt (AttnParams::share_*).  Batch b returns at once, without writing, from the splits below
// p.share_skip[b]: decode_attn_group_kernel below writes those partials.  Every other row and split runs as it always did.  An instance of its own, never with
// FOLD or OFF (launch_decode_attn refuses both).
template <bool DIV, bool FOLD = false, bool OFF = false, bool SHARE = false>
__global__ __launch_bounds__(256, 2) void decode_attn_kernel(const AttnParams p) {
    static_assert(!(FOLD && OFF), "the folded form takes one new token per sequence");
    static_assert(!(SHARE && (FOLD || OFF)), "a launch with shares takes the separate RoPE + split and no draft window");
    __shared__ __attribute__((aligned(16))) float s_o[16][NQ][HD];      // the workgroup's 16 partials: un-normalised O ...
    __shared__ float s_ml[16][NQ][2];                                   // ... maximum and row sum
    __shared__ __attribute__((aligned(16))) bf16x8 s_qkv[FOLD ? 6 : 1][16];   // FOLD: the rotated q heads, the new K row, the new V row
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, head = blockIdx.y, batch = blockIdx.z;
    if (SHARE && split < p.share_skip[batch]) return;         // the group form's split (workgroup-uniform)
    const int slot = p.seq_map ? p.seq_map[batch] : batch;
    const int Sk = (p.sk_arr ? p.sk_arr[slot] + p.sk_add : p.Sk) + (OFF ? p.sk_off[batch] : 0);
    const int64_t prow = (((int64_t)batch * p.H + head) * p.nsplit + split) * NQ;
    if (split * 256 >= Sk) {                                  // a shorter row's empty split: (-inf, 0, 0), as the matrix-core kernel leaves it
        for (int idx = tid; idx < NQ * HD; idx += 256) p.part_o[prow * HD + idx] = 0.f;
        if (tid < NQ) { p.part_ml[(prow + tid) * 2] = -INFINITY; p.part_ml[(prow + tid) * 2 + 1] = 0.f; }
        return;
    }
    const int ksub = lane >> 4, c = lane & 15;
    const int key0 = split * 256 + wave * 64 + ksub;          // this lane's keys: key0 + 4 i
    // one uniform 64-bit base per (slot, head) plane + a 32-bit per-lane element offset (a plane is max_tokens x 128 elements: far below 2^31): the 64 x 64-bit
    // products of `key * stride` per load were a fifth of the kernel's vector instructions
    const bf16* Kb = p.K + (int64_t)slot * p.k_bs + (int64_t)head * p.k_hs;
    const bf16* Vb = p.V + (int64_t)slot * p.v_bs + (int64_t)head * p.v_hs;
    const unsigned k_rs = (unsigned)p.k_rs, v_rs = (unsigned)p.v_rs, lane_off = (unsigned)c * 8u;
    // the query rows first, then all 32 K / V loads behind them, and NOTHING else in between: loads return in order, so the first use of q waits for four
    // loads, not for the stream (left to itself the scheduler consumed q before it had issued the stream: a round trip with nothing in flight)
    bf16x8 q[NQ];
    f32x4 pv[FOLD ? FOLD_MAX_SPLITS : 1][2];
    bf16x8 rc = {}, rs = {};
    const int fslot = tid >> 4;                               // FOLD: threads 0..95 = (slot, chunk c)
    if (!FOLD) {
        const bf16* qp = p.Q + (int64_t)batch * p.q_bs + (int64_t)head * p.q_hs + lane_off;
#pragma unroll
        for (int h = 0; h < NQ; h++) q[h] = *(const bf16x8*)(qp + (int64_t)h * p.q_rs);
    } else if (fslot < 6) {
        const float* pp = p.qkv_part + (int64_t)batch * p.qkv_ld + (head * 6 + fslot) * HD + c * 8;
        const int64_t sstep = (int64_t)gridDim.z * p.qkv_ld;
#pragma unroll
        for (int s = 0; s < FOLD_MAX_SPLITS; s++) {
            const f32x4* ps = (const f32x4*)(pp + (int64_t)min(s, p.qkv_splits - 1) * sstep);
            pv[s][0] = ps[0]; pv[s][1] = ps[1];
        }
        rc = *(const bf16x8*)(p.rope_cos + (int64_t)(Sk - 1) * HD + c * 8);
        rs = *(const bf16x8*)(p.rope_sin + (int64_t)(Sk - 1) * HD + c * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 kr[IT], vr[IT];
#pragma unroll
    for (int i = 0; i < IT; i++) kr[i] = __builtin_nontemporal_load((const bf16x8*)(Kb + ((unsigned)min(key0 + 4 * i, Sk - 1) * k_rs + lane_off)));
#pragma unroll
    for (int i = 0; i < IT; i++) vr[i] = __builtin_nontemporal_load((const bf16x8*)(Vb + ((unsigned)min(key0 + 4 * i, Sk - 1) * v_rs + lane_off)));
    __builtin_amdgcn_sched_barrier(0);
    if (FOLD) {
        const bool new_here = (Sk - 1) >> 8 == split;         // this workgroup's split holds the new token's position (workgroup-uniform)
        if (fslot < 6) {
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < FOLD_MAX_SPLITS; s++)
                if (s < p.qkv_splits) {
#pragma unroll
                    for (int e = 0; e < 4; e++) { a[e] += pv[s][0][e]; a[4 + e] += pv[s][1][e]; }
                }
            bf16x8 x;
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = f2bf(a[e]);
            bf16x8 y = x;
            typedef __attribute__((ext_vector_type(4))) int i32x4_t;
            const i32x4_t xi = __builtin_bit_cast(i32x4_t, x);
            i32x4_t xpi;
#pragma unroll
            for (int e = 0; e < 4; e++) xpi[e] = __builtin_amdgcn_update_dpp(0, xi[e], 0x128, 0xf, 0xf, true);      // row_ror:8: chunk (c + 8) & 15 of the same slot
            if (fslot < 5) {
                const bf16x8 xp = __builtin_bit_cast(bf16x8, xpi);
                const float sign = c < 8 ? -1.0f : 1.0f;       // rotate_half: (-x2, x1)
#pragma unroll
                for (int e = 0; e < 8; e++) y[e] = f2bf(rbf(bf2f(x[e]) * bf2f(rc[e])) + rbf(sign * bf2f(xp[e]) * bf2f(rs[e])));
            }
            s_qkv[fslot][c] = y;
            if (new_here && fslot >= 4) {                       // the cache row of the new token (read by the next steps)
                bf16* dst = const_cast<bf16*>(fslot == 4 ? Kb : Vb) + ((unsigned)(Sk - 1) * (fslot == 4 ? k_rs : v_rs) + lane_off);
                *(bf16x8*)dst = y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < NQ; h++) q[h] = s_qkv[h][c];
        if (new_here) {
            const bf16x8 kn = s_qkv[4][c], vn = s_qkv[5][c];
#pragma unroll
            for (int i = 0; i < IT; i++)
                if (key0 + 4 * i >= Sk - 1) { kr[i] = kn; vr[i] = vn; }
        }
    }
    split_row<DIV>(p, q, kr, vr, key0, Sk, prow, s_o, s_ml);
}

// ---- e4m3 cache (cr_kv_alloc_ex CR_KV_E4M3): the same streaming structure over 128-byte keys ----
// A lane owns 16 bytes (16 dimensions) of every eighth key -- lane = (key sub-index 0..7, 16-byte chunk 0..7) -- so one load instruction still reads
// 8 consecutive keys = ONE contiguous KiB; a wave's 64 keys are 8 K and 8 V loads per lane, all issued up front (256 bytes per lane), plus one fp32 scale
// of K and of V per lane (key = the wave's first + lane: 256 contiguous bytes each), handed to the key's lanes by ds_bpermute.  Per key: 16 bytes -> 16
// bf16 (exact: e4m3 is a subset of bf16), q . k by v_dot2c_f32_bf16, summed over the key's 8 lanes (quad_perm xor 1, xor 2, row_half_mirror: every
// lane ends with the same sum), times the key's scale in fp32, then the bf16 kernel's rounding points (bf16, / sqrt(128), bf16).  P . V: the bf16
// probability times the key's V scale in fp32, FMAs on the converted bytes, fp32 accumulation.  The two 8-key groups of a DPP row merge their partials
// in registers (row_ror:8) in a fixed order, so the workgroup leaves 16 partials in LDS as the bf16 kernel does and merges them in index order: a row's
// result depends on its own key count only.
constexpr int IT8 = 8;                   // keys per lane group and wave (8 groups x 8 = 64 keys per wave)

// sum over the 8 lanes of a half DPP row, left in every lane (the same adds, in the same order, in every lane group)
__device__ __forceinline__ float half_row_sum8(float v) {
    v += dpp<0xb1>(v);       // quad_perm [1, 0, 3, 2]
    v += dpp<0x4e>(v);       // quad_perm [2, 3, 0, 1]
    v += dpp<0x141>(v);      // row_half_mirror
    return v;
}
__device__ __forceinline__ void e4m3x4_to_bf16(unsigned w, bf16x2_t& lo, bf16x2_t& hi) {
    lo = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), bf16x2_t);     // exact both ways
    hi = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)w, true), bf16x2_t);
}

template <bool DIV>
__global__ __launch_bounds__(256, 2) void decode_attn8_kernel(const AttnParams p) {
    __shared__ __attribute__((aligned(16))) float s_o[16][NQ][HD];      // the workgroup's 16 partials: un-normalised O ...
    __shared__ float s_ml[16][NQ][2];                                   // ... maximum and row sum
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, head = blockIdx.y, batch = blockIdx.z;
    const int slot = p.seq_map ? p.seq_map[batch] : batch;
    const int Sk = p.sk_arr ? p.sk_arr[slot] + p.sk_add : p.Sk;
    const int64_t prow = (((int64_t)batch * p.H + head) * p.nsplit + split) * NQ;
    if (split * 256 >= Sk) {                                  // a shorter row's empty split: (-inf, 0, 0)
        for (int idx = tid; idx < NQ * HD; idx += 256) p.part_o[prow * HD + idx] = 0.f;
        if (tid < NQ) { p.part_ml[(prow + tid) * 2] = -INFINITY; p.part_ml[(prow + tid) * 2 + 1] = 0.f; }
        return;
    }
    const int ksub = lane >> 3, c = lane & 7, own = c & 3;
    const int kw = split * 256 + wave * 64;                   // the wave's first key
    const int key0 = kw + ksub;                               // this lane's keys: key0 + 8 i
    const unsigned char* Kb = p.K8 + (int64_t)slot * p.k_bs + (int64_t)head * p.k_hs;
    const unsigned char* Vb = p.V8 + (int64_t)slot * p.v_bs + (int64_t)head * p.v_hs;
    const float* KSb = p.k_scale + (int64_t)slot * p.s_bs + (int64_t)head * p.s_hs;
    const float* VSb = p.v_scale + (int64_t)slot * p.s_bs + (int64_t)head * p.s_hs;
    const unsigned k_rs = (unsigned)p.k_rs, v_rs = (unsigned)p.v_rs, lane_off = (unsigned)c * 16u;
    bf16x8 q[NQ][2];                                          // dimensions 16 c .. 16 c + 15 of the four query heads
    {
        const bf16* qp = p.Q + (int64_t)batch * p.q_bs + (int64_t)head * p.q_hs + c * 16;
#pragma unroll
        for (int h = 0; h < NQ; h++) { q[h][0] = *(const bf16x8*)(qp + (int64_t)h * p.q_rs); q[h][1] = *(const bf16x8*)(qp + (int64_t)h * p.q_rs + 8); }
    }
    __builtin_amdgcn_sched_barrier(0);
    u32x4_t kr[IT8], vr[IT8];
#pragma unroll
    for (int i = 0; i < IT8; i++) kr[i] = __builtin_nontemporal_load((const u32x4_t*)(Kb + ((unsigned)min(key0 + 8 * i, Sk - 1) * k_rs + lane_off)));
#pragma unroll
    for (int i = 0; i < IT8; i++) vr[i] = __builtin_nontemporal_load((const u32x4_t*)(Vb + ((unsigned)min(key0 + 8 * i, Sk - 1) * v_rs + lane_off)));
    const float ks_lane = KSb[min(kw + lane, Sk - 1)], vs_lane = VSb[min(kw + lane, Sk - 1)];
    __builtin_amdgcn_sched_barrier(0);
    const float inv_div = 1.0f / p.s_div;

    // ---- scores of this lane's own query head for its group's 8 keys: s_k . (q . k^) in fp32, then bf16, / sqrt(128), bf16 ----
    float sc[IT8];
#pragma unroll
    for (int i = 0; i < IT8; i++) {
        bf16x2_t kk[8];
#pragma unroll
        for (int w = 0; w < 4; w++) e4m3x4_to_bf16(kr[i][w], kk[2 * w], kk[2 * w + 1]);
        float d[NQ];
#pragma unroll
        for (int h = 0; h < NQ; h++) {
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const bf16x2_t qq = {q[h][e >> 2][2 * (e & 3)], q[h][e >> 2][2 * (e & 3) + 1]};
                a = __builtin_amdgcn_fdot2_f32_bf16(qq, kk[e], a, false);
            }
            d[h] = half_row_sum8(a);
        }
        float s = own == 0 ? d[0] : own == 1 ? d[1] : own == 2 ? d[2] : d[3];
        s = rbf1(s * __shfl(ks_lane, ksub + 8 * i, 64));
        if (DIV) s = rbf1(s * inv_div);
        sc[i] = key0 + 8 * i < Sk ? s : -INFINITY;
    }
    float m = sc[0];
#pragma unroll
    for (int i = 1; i < IT8; i++) m = fmaxf(m, sc[i]);
    const float m2 = (m == -INFINITY ? 0.f : m) * LOG2E;      // a group with no key below Sk: every P is exp(-inf) = 0
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < IT8; i++) {
        const float pe = __builtin_amdgcn_exp2f(fmaf(sc[i], LOG2E, -m2));
        l += pe;                                              // fp32 softmax: the sum of the un-rounded exponentials
        sc[i] = rbf1(pe);                                     // probabilities go to bf16 before .V
    }

    // ---- O[h][16 dims of this lane] += bf16(P[h]) * s_v . V^ ----
    float o[NQ][16];
#pragma unroll
    for (int h = 0; h < NQ; h++)
#pragma unroll
        for (int e = 0; e < 16; e++) o[h][e] = 0.f;
#pragma unroll
    for (int i = 0; i < IT8; i++) {
        float v[16];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vr[i][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vr[i][w], true);
            v[4 * w] = lo[0]; v[4 * w + 1] = lo[1]; v[4 * w + 2] = hi[0]; v[4 * w + 3] = hi[1];
        }
        const float sv = __shfl(vs_lane, ksub + 8 * i, 64);
        const float p0 = dpp<0x00>(sc[i]) * sv, p1 = dpp<0x55>(sc[i]) * sv, p2 = dpp<0xaa>(sc[i]) * sv, p3 = dpp<0xff>(sc[i]) * sv;     // quad_perm: lane (quad, h) holds head h's P
#pragma unroll
        for (int e = 0; e < 16; e++) {
            o[0][e] = fmaf(p0, v[e], o[0][e]);
            o[1][e] = fmaf(p1, v[e], o[1][e]);
            o[2][e] = fmaf(p2, v[e], o[2][e]);
            o[3][e] = fmaf(p3, v[e], o[3][e]);
        }
    }

    // ---- groups 2k and 2k + 1 of a wave (one DPP row) merge in registers; the even group's lanes hold the result ----
    float mh[NQ] = {dpp<0x00>(m), dpp<0x55>(m), dpp<0xaa>(m), dpp<0xff>(m)};
    float lh[NQ] = {dpp<0x00>(l), dpp<0x55>(l), dpp<0xaa>(l), dpp<0xff>(l)};
#pragma unroll
    for (int h = 0; h < NQ; h++) {
        const float mp = dpp<0x128>(mh[h]), lp = dpp<0x128>(lh[h]);      // row_ror:8: the other group of the row
        const float mx = fmaxf(mh[h], mp);
        const float wa = mh[h] == -INFINITY ? 0.f : __expf(mh[h] - mx), wb = mp == -INFINITY ? 0.f : __expf(mp - mx);
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float op = dpp<0x128>(o[h][e]);
            o[h][e] = wa * o[h][e] + wb * op;
        }
        lh[h] = wa * lh[h] + wb * lp;
        mh[h] = mx;
    }
    const int j = wave * 4 + (ksub >> 1);
    if (!(ksub & 1)) {
#pragma unroll
        for (int h = 0; h < NQ; h++)
#pragma unroll
            for (int e = 0; e < 16; e += 4) *(f32x4*)&s_o[j][h][c * 16 + e] = f32x4{o[h][e], o[h][e + 1], o[h][e + 2], o[h][e + 3]};
        if (c == 0) {
#pragma unroll
            for (int h = 0; h < NQ; h++) { s_ml[j][h][0] = mh[h]; s_ml[j][h][1] = lh[h]; }
        }
    }
    __syncthreads();
    {
        const int h = tid >> 6, d0 = (tid & 63) * 2;
        float M = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < 16; jj++) M = fmaxf(M, s_ml[jj][h][0]);
        float L = 0.f, a0 = 0.f, a1 = 0.f;
        if (M != -INFINITY) {
#pragma unroll
            for (int jj = 0; jj < 16; jj++) {
                const float mj = s_ml[jj][h][0];
                const float w = mj == -INFINITY ? 0.f : __expf(mj - M);
                L += w * s_ml[jj][h][1];
                a0 += w * s_o[jj][h][d0];
                a1 += w * s_o[jj][h][d0 + 1];
            }
        }
        *(f32x2_t*)(p.part_o + (prow + h) * HD + d0) = f32x2_t{a0, a1};
        if ((tid & 63) == 0) { p.part_ml[(prow + h) * 2] = M; p.part_ml[(prow + h) * 2 + 1] = L; }
    }
}

bool decode_attn_off() {
    static const bool off = [] { const char* e = getenv("CR_DECODE_ATTN"); return e && e[0] == '0'; }();      // A/B aid: the matrix-core split kernel
    return off;
}

}  // namespace

bool decode_attn8_available() { return !decode_attn_off(); }

// the e4m3 kernel's shape: the streaming kernel's, with 128-byte keys (16-byte aligned rows and planes) and fp32 scales
bool decode_attn8_supported(const AttnParams& p, int head_dim) {
    return decode_attn8_available() && !p.force_matrix_core && p.K8 && p.V8 && p.k_scale && p.v_scale && !p.qkv_part && !p.sk_off && p.kv_group == 1 && head_dim == HD &&
           p.Sq == NQ && ATTN_SPLIT_TILES == 4 && p.q_prescale == 1.0f && p.part_ml && p.part_o && p.nsplit > 0 &&
           (p.q_rs & 7) == 0 && (p.q_hs & 7) == 0 && (p.q_bs & 7) == 0 && (p.k_rs & 15) == 0 && (p.v_rs & 15) == 0 && (p.k_hs & 15) == 0 && (p.v_hs & 15) == 0 &&
           (p.k_bs & 15) == 0 && (p.v_bs & 15) == 0 && (p.sk_arr || p.Sk > 0) && p.k_rs > 0 && p.v_rs > 0 && p.k_rs < 65536 && p.v_rs < 65536 &&
           (int64_t)p.nsplit * 256 * (p.k_rs > p.v_rs ? p.k_rs : p.v_rs) < (1ll << 32) &&
           (((uintptr_t)p.Q | (uintptr_t)p.K8 | (uintptr_t)p.V8) & 15) == 0 && (((uintptr_t)p.k_scale | (uintptr_t)p.v_scale) & 3) == 0 &&
           ((uintptr_t)p.part_o & 7) == 0;
}

// the shape the kernel is written for: d = 128, four query rows per (batch, head) (the GQA group), splits of 256 keys (ATTN_SPLIT_TILES = 4)
bool decode_attn_supported(const AttnParams& p, int head_dim) {
    // kv_group == 1: the kernel indexes K / V by blockIdx.y itself, i.e. H counts KV heads and the GQA group is the Sq = 4 query rows
    return !decode_attn_off() && !p.K8 && !p.force_matrix_core && p.kv_group == 1 && head_dim == HD && p.Sq == NQ && ATTN_SPLIT_TILES == 4 && p.q_prescale == 1.0f && p.part_ml && p.part_o && p.nsplit > 0 &&
           (p.q_rs & 7) == 0 && (p.q_hs & 7) == 0 && (p.q_bs & 7) == 0 && (p.k_rs & 7) == 0 && (p.v_rs & 7) == 0 && (p.k_hs & 7) == 0 && (p.v_hs & 7) == 0 &&
           (p.k_bs & 7) == 0 && (p.v_bs & 7) == 0 && (p.sk_arr || p.Sk > 0) && p.k_rs > 0 && p.v_rs > 0 && p.k_rs < 65536 && p.v_rs < 65536 &&
           (int64_t)p.nsplit * 256 * (p.k_rs > p.v_rs ? p.k_rs : p.v_rs) < (1ll << 32) &&      // key * row stride stays in the 32-bit per-lane offset
           (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V) & 15) == 0 && ((uintptr_t)p.part_o & 7) == 0;      // 16-byte loads, 8-byte partial stores
}

// the folded form on top: partial sums of the [H groups][4 q | k | v][128] row, at most FOLD_MAX_SPLITS slices, one new token per row at position sk_arr[slot]
bool decode_attn_fold_supported(const AttnParams& p, int head_dim) {
    return decode_attn_supported(p, head_dim) && !p.sk_off && p.qkv_part && p.rope_cos && p.rope_sin && p.qkv_splits >= 1 && p.qkv_splits <= FOLD_MAX_SPLITS &&
           p.sk_arr && p.sk_add == 1 && p.k_rs == HD && p.v_rs == HD && (p.qkv_ld & 3) == 0 && p.qkv_ld >= (int64_t)p.H * 6 * HD &&
           (((uintptr_t)p.qkv_part | (uintptr_t)p.rope_cos | (uintptr_t)p.rope_sin) & 15) == 0;
}

int attn_share_table(const int32_t* seqs, const int32_t* pfx_src, const int32_t* pfx_len, int B, std::vector<int32_t>& table, int* max_splits) {
    table.clear();
    *max_splits = 0;
    bool any = false;
    for (int b = 0; b < B; b++) any |= pfx_src[b] >= 0 && pfx_len[b] >= 256;
    if (!any) return 0;
    table.assign(B, 0);
    std::vector<char> placed(B, 0);
    int n_chunks = 0;
    for (int b = 0; b < B; b++) {
        if (placed[b] || pfx_src[b] < 0 || pfx_len[b] < 256) continue;
        const int src = pfx_src[b], len = pfx_len[b];
        std::vector<int> rows;
        for (int r = 0; r < B; r++) {
            // the group's sharers, and the source's own row (the longest share of a source only: its row joins one group)
            const bool sharer = pfx_src[r] == src && pfx_len[r] == len;
            bool source = seqs[r] == src && pfx_src[r] < 0 && !placed[r];
            for (int t = 0; source && t < B; t++) source = !(pfx_src[t] == src && pfx_len[t] > len);
            if (sharer || source) { rows.push_back(r); placed[r] = 1; }
        }
        for (size_t r0 = 0; r0 < rows.size(); r0 += ATTN_SHARE_ROWS) {
            const int n = (int)std::min<size_t>(ATTN_SHARE_ROWS, rows.size() - r0);
            table.insert(table.end(), {src, len / 256, n, 0});
            for (int j = 0; j < ATTN_SHARE_ROWS; j++) table.push_back(rows[r0 + (j < n ? j : 0)]);
            n_chunks++;
        }
        for (int r : rows) table[r] = len / 256;
        *max_splits = std::max(*max_splits, len / 256);
    }
    return n_chunks;
}

int launch_decode_attn(const AttnParams& p, hipStream_t stream) {
    const dim3 grid(p.nsplit, p.H, p.B);
    if (p.share_n > 0) {
        // shares: bf16, the separate RoPE + split, no draft window; the chunks' splits lie inside the launch's
        if (p.K8 || p.qkv_part || p.sk_off || !p.share_chunks || !p.share_skip || p.share_splits < 1 || p.share_splits > p.nsplit || !p.Q) return CR_ERR_ARG;
        if (launch_decode_attn_group(p, stream) != CR_OK) return CR_ERR_HIP;
        if (p.s_div != 1.0f) hipLaunchKernelGGL((decode_attn_kernel<true, false, false, true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((decode_attn_kernel<false, false, false, true>), grid, dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
    }
    if (p.K8) {
        if (!decode_attn8_supported(p, HD)) return CR_ERR_ARG;
        if (p.s_div != 1.0f) hipLaunchKernelGGL((decode_attn8_kernel<true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((decode_attn8_kernel<false>), grid, dim3(256), 0, stream, p);
    } else if (p.qkv_part) {
        if (!decode_attn_fold_supported(p, HD)) return CR_ERR_ARG;
        if (p.s_div != 1.0f) hipLaunchKernelGGL((decode_attn_kernel<true, true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((decode_attn_kernel<false, true>), grid, dim3(256), 0, stream, p);
    } else if (p.sk_off) {
        if (p.s_div != 1.0f) hipLaunchKernelGGL((decode_attn_kernel<true, false, true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((decode_attn_kernel<false, false, true>), grid, dim3(256), 0, stream, p);
    } else if (p.s_div != 1.0f) hipLaunchKernelGGL((decode_attn_kernel<true, false>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((decode_attn_kernel<false, false>), grid, dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
}

// The per-row arithmetic of the streaming decode attention (attention_decode.hip), in a header of its own so that the per-row kernel and the group form
// (attention_decode_group.hip: a shared prompt, one load of the keys for several rows) inline the SAME device function: a row's bits cannot depend on which of
// them ran a split.
#pragma once
#include <stdint.h>

#include "attention.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int HD = 128, NQ = 4, IT = 16;      // head dimension, query heads per KV head, keys per lane group and wave (4 groups x 16 = 64 keys per wave)
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

__device__ __forceinline__ float rbf1(float x) {           // round to bf16, as an fp32 value, in one v_cvt_pk_bf16_f32 (attention.hip)
    const f32x2_t v = {0.f, x};
    return __uint_as_float(__builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2)));
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum over the 16 lanes of a DPP row, left in every lane (rotations: the order of the adds is the same in every lane group of every launch)
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp<0x128>(v);      // row_ror:8
    v += dpp<0x124>(v);      // row_ror:4
    v += dpp<0x122>(v);      // row_ror:2
    v += dpp<0x121>(v);      // row_ror:1
    return v;
}

// acc + round(a * b): the product is rounded to fp32 before the add, whatever -ffp-contract says
__device__ __forceinline__ float add_rounded_product(float acc, float a, float b) {
#pragma clang fp contract(off)
    const float prod = a * b;
    return acc + prod;
}

// One row's share of one split, from the 16 keys per lane group in kr / vr to the row's partial for that split: the scores with their rounding points, the
// 16-key softmax, P.V, the 16 partials of the workgroup merged in LDS in index order, the store to part_o / part_ml at prow.  The ONE statement of this
// arithmetic: the per-row kernel and the group form (a shared prompt: one load of the keys, several rows) both inline it, so a row's bits cannot depend on which
// of them ran its split.  Sk: the row's key count (keys at or past it score -inf); the caller passes the largest int where the split is known to be full.
// Ends with the workgroup's LDS read: a caller that runs another row puts a barrier in between.
template <bool DIV>
__device__ __forceinline__ void split_row(const AttnParams& p, const bf16x8 (&q)[NQ], const bf16x8 (&kr)[IT], const bf16x8 (&vr)[IT], int key0, int Sk, int64_t prow,
                                          float (&s_o)[16][NQ][HD], float (&s_ml)[16][NQ][2]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ksub = lane >> 4, c = lane & 15, own = c & 3;
    const float inv_div = 1.0f / p.s_div;

    // ---- scores of this lane's own query head for its group's 16 keys ----
    float sc[IT];
#pragma unroll
    for (int i = 0; i < IT; i++) {
        float d[NQ];
#pragma unroll
        for (int h = 0; h < NQ; h++) {
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bf16x2_t qq = {q[h][2 * e], q[h][2 * e + 1]}, kk = {kr[i][2 * e], kr[i][2 * e + 1]};
                a = __builtin_amdgcn_fdot2_f32_bf16(qq, kk, a, false);
            }
            d[h] = row_sum16(a);
        }
        float s = own == 0 ? d[0] : own == 1 ? d[1] : own == 2 ? d[2] : d[3];
        s = rbf1(s);                                          // scores are bf16 (:393), divided by sqrt(d) -> bf16
        if (DIV) s = rbf1(s * inv_div);
        sc[i] = key0 + 4 * i < Sk ? s : -INFINITY;
    }
    float m = sc[0];
#pragma unroll
    for (int i = 1; i < IT; i++) m = fmaxf(m, sc[i]);
    const float m2 = (m == -INFINITY ? 0.f : m) * LOG2E;      // a group with no key below Sk: every P is exp(-inf) = 0
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < IT; i++) {
        const float pe = __builtin_amdgcn_exp2f(fmaf(sc[i], LOG2E, -m2));
        l += pe;                                              // fp32 softmax (:409): the sum of the un-rounded exponentials
        sc[i] = rbf1(pe);                                     // probabilities go to bf16 before .V
    }

    // ---- O[h][8 dims of this lane] += P[h] . V ----
    float o[NQ][8];
#pragma unroll
    for (int h = 0; h < NQ; h++)
#pragma unroll
        for (int e = 0; e < 8; e++) o[h][e] = 0.f;
#pragma unroll
    for (int i = 0; i < IT; i++) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = (float)vr[i][e];
        const float p0 = dpp<0x00>(sc[i]), p1 = dpp<0x55>(sc[i]), p2 = dpp<0xaa>(sc[i]), p3 = dpp<0xff>(sc[i]);     // quad_perm: lane (quad, h) holds head h's P
#pragma unroll
        for (int e = 0; e < 8; e++) {
            o[0][e] = fmaf(p0, v[e], o[0][e]);
            o[1][e] = fmaf(p1, v[e], o[1][e]);
            o[2][e] = fmaf(p2, v[e], o[2][e]);
            o[3][e] = fmaf(p3, v[e], o[3][e]);
        }
    }

    // ---- the 16 partials of the workgroup (wave, group) in LDS, merged in index order ----
    const int j = wave * 4 + ksub;
#pragma unroll
    for (int h = 0; h < NQ; h++) {
        *(f32x4*)&s_o[j][h][c * 8] = f32x4{o[h][0], o[h][1], o[h][2], o[h][3]};
        *(f32x4*)&s_o[j][h][c * 8 + 4] = f32x4{o[h][4], o[h][5], o[h][6], o[h][7]};
    }
    if (c < NQ) { s_ml[j][c][0] = m; s_ml[j][c][1] = l; }     // lane c of a group holds head c's (m, l) (so do lanes c + 4, c + 8, c + 12)
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
                // Every rounding point written out.  Left as `a1 += w * o`, fusing is the compiler's choice per translation unit, and it chose differently for the
                // per-row kernel (it packs (a0, L) into fused v_pk_fma_f32 and leaves a1 alone: partials 0..3 fused, 4..15 a rounded product then an add -- what this
                // says, and what every build so far computed) and for the group form (all fused): one bf16 step of an odd output dimension now and then.
                L = fmaf(w, s_ml[jj][h][1], L);
                a0 = fmaf(w, s_o[jj][h][d0], a0);
                a1 = jj < 4 ? fmaf(w, s_o[jj][h][d0 + 1], a1) : add_rounded_product(a1, w, s_o[jj][h][d0 + 1]);
            }
        }
        *(f32x2_t*)(p.part_o + (prow + h) * HD + d0) = f32x2_t{a0, a1};
        if ((tid & 63) == 0) { p.part_ml[(prow + h) * 2] = M; p.part_ml[(prow + h) * 2 + 1] = L; }
    }
}

}  // namespace

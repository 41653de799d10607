// Span mass for gfx950: how much attention probability a row puts on each of a list of key ranges, summed over heads.
//
// One workgroup = ONE wave = up to 32 grounded rows of one sequence x one KV head; the wave holds the queries of the KV head's four query heads, so a K block
// is fetched once per GQA group and the four heads' probabilities are added in registers, in head order -- no LDS, no barrier, no atomics.
//   S^T = K . Q^T        v_mfma_f32_32x32x16_bf16 with the prefill kernel's swapped operands (attention.hip): the QUERY sits on the lane, 16 keys of a 32-key
//                        block in its accumulator registers, the other 16 on lane + 32.  A span sum is register adds plus one __shfl_xor(., 32).
// Scores follow the prefill attention's DIV path bit for bit: bf16(bf16(q . k) * (1 / s_div)), fp32 dot product, causal mask.
//   pass 1   every 32-key block up to the group's last position: running maximum m and sum l of exp(s - m) per head.  Each lane rescales by ITS row's maximum
//            alone (no wave-wide vote), so a row's (m, l) depends on its own keys only; a block wholly behind a row leaves its m and l bit for bit alone.
//   pass 2   only the blocks that a span touches: P = exp(s - m) * (1 / l), never rounded, the four heads added, then per span the registers whose key lies in
//            it, in register order, block after block; the two lane halves meet once per span.
// Every sum has a fixed order that depends on absolute key positions only: the same row alone and in a larger call gives the same bits.
// The partials [KV head][row][span] of a layer are added in KV-head order by span_mass_add_kernel into mass; layers add in launch order.
#include "ground.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int HD = 128, KS = HD / 16, NHG = GROUND_GROUP_HEADS;

__global__ __launch_bounds__(64) void span_mass_kernel(const SpanMassParams p) {
    const int lane = threadIdx.x, l31 = lane & 31, hh = lane >> 5;
    const int kvh = blockIdx.y, nkv = p.H / NHG;
    const int32_t* gr = p.ix.group + 4 * blockIdx.x;
    const int r0 = __builtin_amdgcn_readfirstlane(gr[0]), cnt = __builtin_amdgcn_readfirstlane(gr[1]);
    const int slot = __builtin_amdgcn_readfirstlane(gr[2]), sq = __builtin_amdgcn_readfirstlane(gr[3]);
    const int ri = r0 + min(l31, cnt - 1);                    // lanes past the group's rows repeat its last row and store nothing
    const int qrow = p.ix.row_q[ri], qpos = p.ix.row_pos[ri];
    const int pmax = __builtin_amdgcn_readfirstlane(p.ix.row_pos[r0 + cnt - 1]);      // rows are in position order: no key behind it is ever read
    const float inv_div = 1.0f / p.s_div;

    // ---- Q fragments (B operand): lane (query l31, half hh) holds Q[q][head][16 ks + 8 hh .. + 7]
    bf16x8 qf[NHG][KS];
    {
        const bf16* qp = p.q + ((int64_t)qrow * p.H + (int64_t)kvh * NHG) * HD + hh * 8;
#pragma unroll
        for (int h = 0; h < NHG; h++)
#pragma unroll
            for (int ks = 0; ks < KS; ks++) qf[h][ks] = *(const bf16x8*)(qp + h * HD + ks * 16);
    }
    const bf16* Kb = p.k + ((int64_t)slot * nkv + kvh) * (int64_t)p.max_tokens * HD + hh * 8;

    // masked scores of 32-key block `blk` for the four heads: register e of a lane holds key 32 blk + (e & 3) + 8 (e >> 2) + 4 hh
    auto scores = [&](int blk, f32x16 (&s)[NHG]) {
        const int krow = min(blk * 32 + l31, pmax);            // keys past the last position are masked for every row: any cached row stands in
        const bf16* kp = Kb + (int64_t)krow * HD;
        bf16x8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ks++) kf[ks] = *(const bf16x8*)(kp + ks * 16);
#pragma unroll
        for (int h = 0; h < NHG; h++) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; e++) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ks++) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[h][ks], acc, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                float a, b;
                round_pair_bf16(acc[e], acc[e + 1], a, b);
                round_pair_bf16(a * inv_div, b * inv_div, a, b);
                const int key = blk * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                s[h][e] = key <= qpos ? a : -INFINITY;
                s[h][e + 1] = key + 1 <= qpos ? b : -INFINITY;
            }
        }
    };

    // ---- pass 1: m and l per head (key 0 is in front of every row, so m is finite from the first block on)
    float m[NHG], inv[NHG];
    {
        float l[NHG];
#pragma unroll
        for (int h = 0; h < NHG; h++) { m[h] = -INFINITY; l[h] = 0.f; }
        const int nblk = pmax / 32 + 1;
        for (int blk = 0; blk < nblk; blk++) {
            f32x16 s[NHG];
            scores(blk, s);
#pragma unroll
            for (int h = 0; h < NHG; h++) {
                float mx = s[h][0];
#pragma unroll
                for (int e = 1; e < 16; e++) mx = fmaxf(mx, s[h][e]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mn = fmaxf(m[h], mx);
                const float alpha = m[h] == mn ? 1.0f : __builtin_amdgcn_exp2f((m[h] - mn) * LOG2E);
                float sum = 0.f;
#pragma unroll
                for (int e = 0; e < 16; e++) sum += __builtin_amdgcn_exp2f((s[h][e] - mn) * LOG2E);
                l[h] = l[h] * alpha + sum;
                m[h] = mn;
            }
        }
#pragma unroll
        for (int h = 0; h < NHG; h++) inv[h] = 1.0f / (l[h] + __shfl_xor(l[h], 32, 64));
    }

    // ---- pass 2: the spans, in order; a block is computed once (spans are sorted, so the block index never goes back)
    const int sp0 = __builtin_amdgcn_readfirstlane(p.ix.span_off[sq]);
    const int ns = __builtin_amdgcn_readfirstlane(p.ix.span_off[sq + 1]) - sp0;
    const int32_t* sp = p.ix.spans + 2 * (int64_t)sp0;
    float* out = p.partial + ((int64_t)kvh * p.R + r0 + l31) * p.W;
    const bool store = hh == 0 && l31 < cnt;
    int cur = -1;
    f32x16 c;
    for (int b = 0; b < ns; b++) {
        const int s0 = __builtin_amdgcn_readfirstlane(sp[2 * b]);
        const int s1 = min(__builtin_amdgcn_readfirstlane(sp[2 * b + 1]), pmax + 1);      // keys behind every row of the group add 0
        float acc = 0.f;
        for (int blk = s0 >> 5; s0 < s1 && blk * 32 < s1; blk++) {      // no round for an empty span, nor for one behind the whole group
            if (blk != cur) {
                f32x16 s[NHG];
                scores(blk, s);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    float v = __builtin_amdgcn_exp2f((s[0][e] - m[0]) * LOG2E) * inv[0];
#pragma unroll
                    for (int h = 1; h < NHG; h++) v += __builtin_amdgcn_exp2f((s[h][e] - m[h]) * LOG2E) * inv[h];
                    c[e] = v;
                }
                cur = blk;
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int key = blk * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                acc += (key >= s0 && key < s1) ? c[e] : 0.f;
            }
        }
        acc += __shfl_xor(acc, 32, 64);
        if (store) out[b] = acc;
    }
}

// mass[r][b] (+)= sum over KV heads, in KV-head order; the scale once, with the last layer
__global__ __launch_bounds__(256) void span_mass_add_kernel(const SpanMassParams p) {
    const int r = blockIdx.x, nkv = p.H / NHG;
    const int sq = p.ix.row_seq[r];
    const int ns = p.ix.span_off[sq + 1] - p.ix.span_off[sq];
    for (int b = threadIdx.x; b < p.mass_ld; b += 256) {
        float v = 0.f;
        if (b < ns) {
            if (!p.first) v = p.mass[(int64_t)r * p.mass_ld + b];
            float s = 0.f;
            for (int h = 0; h < nkv; h++) s += p.partial[((int64_t)h * p.R + r) * p.W + b];
            v += s;
            if (p.last) v *= p.scale;
        }
        p.mass[(int64_t)r * p.mass_ld + b] = v;
    }
}

}  // namespace

int ground_check_spans(const int32_t* spans, int count, int limit) {
    int prev = 0;
    for (int b = 0; b < count; b++) {
        const int s = spans[2 * b], e = spans[2 * b + 1];
        if (s < prev || e < s || e > limit) return b + 1;
        prev = e;
    }
    return 0;
}

int ground_groups(const std::vector<GroundSeq>& seqs) {
    int G = 0;
    for (const GroundSeq& q : seqs) G += ((int)q.row_q.size() + GROUND_ROWS - 1) / GROUND_ROWS;
    return G;
}

void ground_fill_index(const std::vector<GroundSeq>& seqs, int32_t* h) {
    int R = 0, total = 0;
    const int n = (int)seqs.size(), G = ground_groups(seqs);
    for (const GroundSeq& q : seqs) { R += (int)q.row_q.size(); total += q.n_spans; }
    const GroundIndex ix = ground_index(h, R, G, n, total);
    int r = 0, g = 0, t = 0;
    for (int i = 0; i < n; i++) {
        const GroundSeq& q = seqs[i];
        const int k = (int)q.row_q.size();
        for (int j0 = 0; j0 < k; j0 += GROUND_ROWS, g++) {
            ix.group[4 * g] = r + j0; ix.group[4 * g + 1] = std::min(GROUND_ROWS, k - j0); ix.group[4 * g + 2] = q.slot; ix.group[4 * g + 3] = i;
        }
        for (int j = 0; j < k; j++, r++) { ix.row_q[r] = q.row_q[j]; ix.row_pos[r] = q.row_pos[j]; ix.row_seq[r] = i; }
        ix.span_off[i] = t;
        for (int b = 0; b < 2 * q.n_spans; b++) ix.spans[2 * t + b] = q.spans[b];
        t += q.n_spans;
    }
    ix.span_off[n] = t;
}

int launch_span_mass(const SpanMassParams& p, hipStream_t stream) {
    if (!p.q || !p.k || !p.partial || !p.mass || !p.ix.row_q || p.H <= 0 || p.H % NHG != 0 || p.max_tokens <= 0 || p.R <= 0 || p.G <= 0 || p.W < 0 ||
        p.mass_ld < p.W || !(p.s_div > 0.f))
        return CR_ERR_ARG;
    if (p.W > 0) hipLaunchKernelGGL(span_mass_kernel, dim3(p.G, p.H / NHG), dim3(64), 0, stream, p);
    if (p.mass_ld > 0) hipLaunchKernelGGL(span_mass_add_kernel, dim3(p.R), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
}

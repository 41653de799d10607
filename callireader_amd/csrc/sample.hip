// Sampled token choice: transformers 4.45.2 GenerationMixin._sample with do_sample=True (the processor order of
// _get_logits_processor): RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
// one draw from the softmax of what remains.  One workgroup of 1024 threads per row (as pick_kernel).
//
//   z_i    = penalised logit / temperature (fp32 division, skipped at temperature 1)
//   top-k  : keep z_i >= the k-th largest z (ties at the k-th value all kept); skipped at k == 0 or k >= vocab
//   top-p  : over the top-k survivors, S(v) = sum of softmax(z) over z <= v; keep z_i with S(z_i) > fp32(1 - top_p) (HF removes
//            ascending cumsum <= 1 - top_p), always keeping the maximum; skipped at top_p >= 1.  At an exact tie of the boundary value
//            every tied id is kept (HF's torch.sort order keeps some of them).
//   draw   : argmax over kept i of (double)z_i + g_i, g_i = -log(-log u_i) in double, lowest id on a tie (Gumbel-max: exactly softmax(z)
//            over the kept set).  u_i = ((x >> 8) + 0.5) * 2^-24, x = word i % 4 of Philox-4x32-10(counter = (i / 4, step, 0, 0),
//            key = (seed low 32 bits, seed high 32 bits)); step = the sequence's generated-id count before this pick.
//
// Thresholds: a selection over the row's values with linear value bins (2048 per pass, bin = floor((z - lo) * 2048 / (hi - lo)) in double,
// monotone in z) weighted by counts (top-k) or by fixed-point softmax mass (top-p: floor(exp(z - max) * 2^40), integer sums, so the
// result does not depend on the order of the LDS atomics); the bin holding the boundary is gathered into LDS when it holds <= 2048 ids
// (sorted there, the boundary found by a prefix scan), otherwise narrowed to its own value range and binned again (each round shrinks the
// range 2048-fold).  Passes over the row: penalty, min/max, one per threshold + its gather, the draw.
// Non-finite scores (a NaN logit, or a temperature whose division overflows): NaN ids are never kept; +-inf take part in the thresholds by key
// (no value bins, zero softmax weight) and a +inf score wins the draw (the lowest such id); a row with no kept score above -inf gets the greedy
// pick's id.  Every selection loop is bounded.
#include <stdio.h>

#include "ctx.hpp"
#include "pick.hpp"

namespace {

constexpr int NB = 2048;       // bins of one selection pass
constexpr int CAP = 2048;      // ids a boundary bin may hold to be sorted in LDS

__host__ __device__ inline void philox_round(uint32_t (&c)[4], const uint32_t (&k)[2]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c[1] ^ k[0], n2 = hi0 ^ c[3] ^ k[1];
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

// Philox-4x32-10 (Salmon et al., SC'11; the Random123 / rocRAND constants)
__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint64_t seed) {
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < 10; r++) {
        if (r) { k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u; }
        philox_round(c, k);
    }
}

// order-preserving uint32 key of a float (finite values and +-inf)
__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float kfloat(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// fixed-point softmax weight; 0 where exp(z - zmax) is not a number in (0, 1] (z or zmax infinite)
__device__ __forceinline__ uint64_t fixmass(float z, float zmax) {
    const float e = expf(z - zmax);
    return (e > 0.f && e <= 1.f) ? (uint64_t)(e * 0x1p40f) : 0ull;
}

// Bin of an id in a selection round over the keys [klo, khi]: linear in the value when both ends are finite and apart (the common case), else
// linear in the key (infinite scores, only +-0, or a round that did not narrow the interval).  Both are monotone in the key, and both put klo
// in bin 0 and khi in a later bin, so every round strictly narrows the interval that holds the boundary.
struct Binner {
    bool by_key;
    double dlo, sc;
    uint32_t klo;
    uint64_t span;
    __device__ Binner(uint32_t lo, uint32_t hi, bool force_key) : klo(lo), span((uint64_t)(hi - lo) + 1) {
        dlo = (double)kfloat(lo);
        const double dhi = (double)kfloat(hi);
        sc = (double)NB / (dhi - dlo);
        by_key = force_key || !(isfinite(dlo) && isfinite(dhi) && isfinite(sc) && sc > 0.0);
    }
    __device__ __forceinline__ int operator()(float z, uint32_t k) const {
        if (by_key) return (int)(((uint64_t)(k - klo) * NB) / span);
        const int b = (int)(((double)z - dlo) * sc);
        return b > NB - 1 ? NB - 1 : b;
    }
};

struct SelShared {
    unsigned long long mass[NB];   // per-bin weight (top-p: fixed-point mass; top-k: count)
    uint32_t cnt[NB];              // per-bin count
    uint32_t cand[CAP];            // gathered keys of the boundary bin
    unsigned long long wtot[16];   // block scan: per-wave totals
    unsigned long long below, total;
    int bin, n;
    uint32_t kmin, kmax;
};

// Inclusive block scan (1024 threads) of one value per thread.
__device__ unsigned long long block_scan(unsigned long long v, SelShared& s, int tid) {
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    __syncthreads();
    if (lane == 63) s.wtot[w] = v;
    __syncthreads();
    unsigned long long off = 0;
    for (int i = 0; i < w; i++) off += s.wtot[i];
    return v + off;
}

// Pairs (2 tid, 2 tid + 1) of the weights w[0, 2048): the index j whose inclusive prefix first exceeds thr - base goes to s.bin (-1 if none),
// the prefix before it to s.below (added to base).
__device__ void find_cross(const unsigned long long* w, unsigned long long base, unsigned long long thr, SelShared& s, int tid, bool set_total) {
    const unsigned long long a = w[2 * tid], b = w[2 * tid + 1];
    const unsigned long long incl = block_scan(a + b, s, tid);
    const unsigned long long excl = incl - a - b;
    if (tid == 0) s.bin = -1;
    if (set_total && tid == 1023) s.total = incl;
    __syncthreads();
    if (base + excl <= thr && thr < base + excl + a) { s.bin = 2 * tid; s.below = base + excl; }
    else if (base + excl + a <= thr && thr < base + incl) { s.bin = 2 * tid + 1; s.below = base + excl + a; }
    __syncthreads();
}

__device__ __forceinline__ float zval(const float* lg, int i, float temp) {
    const float v = lg[i];
    return temp != 1.0f ? v / temp : v;
}

// Key of the boundary: the smallest key K in [klo, khi] whose weight of ids with keys in [klo, K] exceeds thr (MASS: thr = fp32(1 - top_p) *
// total mass of [klo, khi]; else thr is given).  Keys, weights and bins depend only on the row's values: the result is deterministic.
// At most MAX_ROUNDS rounds: value bins narrow the range 2048-fold per round and key bins at least 1024-fold (a 32-bit key range resolves in
// 4); the bound only guarantees termination, a row that reaches it keeps [khi] (its maximum).
constexpr int MAX_ROUNDS = 40;
template <bool MASS>
__device__ uint32_t select_key(const float* lg, int vocab, float temp, float zmax, uint32_t klo, uint32_t khi, unsigned long long thr, float omp,
                               SelShared& s, int tid) {
    unsigned long long below = 0;
    bool first = true, force_key = false;
    for (int round = 0; round < MAX_ROUNDS; round++) {
        if (klo == khi) return klo;
        const Binner bin(klo, khi, force_key);
        for (int b = tid; b < NB; b += 1024) { s.mass[b] = 0; s.cnt[b] = 0; }
        __syncthreads();
        for (int i = tid; i < vocab; i += 1024) {
            const float z = zval(lg, i, temp);
            const uint32_t k = fkey(z);
            if (k < klo || k > khi) continue;
            const int b = bin(z, k);
            atomicAdd(&s.cnt[b], 1u);
            if (MASS) atomicAdd(&s.mass[b], (unsigned long long)fixmass(z, zmax));
        }
        __syncthreads();
        if (!MASS) {
            for (int b = tid; b < NB; b += 1024) s.mass[b] = s.cnt[b];
            __syncthreads();
        }
        find_cross(s.mass, below, MASS && first ? ~0ull : thr, s, tid, MASS && first);
        if (MASS && first) {
            // the threshold needs the total mass of the interval (the top-k survivors): fp32(1 - top_p) * total, as HF compares the fp32 cumsum
            thr = (unsigned long long)((double)omp * (double)s.total);
            if (thr >= s.total) return khi;                   // nothing exceeds it (top_p = 0): the maximum alone
            find_cross(s.mass, below, thr, s, tid, false);
        }
        first = false;
        const int bsel = s.bin;
        if (bsel < 0) return khi;
        below = s.below;
        const uint32_t n = s.cnt[bsel];
        if (n <= (uint32_t)CAP) {
            if (tid == 0) s.n = 0;
            for (int j = tid; j < CAP; j += 1024) s.cand[j] = 0xffffffffu;
            __syncthreads();
            for (int i = tid; i < vocab; i += 1024) {
                const float z = zval(lg, i, temp);
                const uint32_t k = fkey(z);
                if (k < klo || k > khi) continue;
                if (bin(z, k) == bsel) s.cand[atomicAdd(&s.n, 1)] = k;
            }
            __syncthreads();
            // bitonic sort, ascending, CAP keys (the padding 0xffffffff sorts last)
            for (int kk = 2; kk <= CAP; kk <<= 1)
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    const int i0 = (tid / j) * 2 * j + (tid % j), i1 = i0 + j;
                    const uint32_t a = s.cand[i0], b = s.cand[i1];
                    const bool up = (i0 & kk) == 0;
                    if ((a > b) == up) { s.cand[i0] = b; s.cand[i1] = a; }
                    __syncthreads();
                }
            // weights of the sorted candidates into the bin arrays' room, then the same crossing search
            for (int j = tid; j < CAP; j += 1024)
                s.mass[j] = j < (int)n ? (MASS ? (unsigned long long)fixmass(kfloat(s.cand[j]), zmax) : 1ull) : 0ull;
            __syncthreads();
            find_cross(s.mass, below, thr, s, tid, false);
            const int j = s.bin;
            const uint32_t r = j >= 0 ? s.cand[j] : khi;
            __syncthreads();
            return r;
        }
        // too many ids in the boundary bin: narrow the interval to the bin's own value range and bin again
        if (tid == 0) { s.kmin = 0xffffffffu; s.kmax = 0; }
        __syncthreads();
        for (int i = tid; i < vocab; i += 1024) {
            const float z = zval(lg, i, temp);
            const uint32_t k = fkey(z);
            if (k < klo || k > khi) continue;
            if (bin(z, k) == bsel) { atomicMin(&s.kmin, k); atomicMax(&s.kmax, k); }
        }
        __syncthreads();
        force_key = s.kmin == klo && s.kmax == khi;             // no progress in the value: bin by key from now on
        klo = s.kmin; khi = s.kmax;
        __syncthreads();
    }
    return khi;
}

// The pick of one row by its workgroup of 1024: the body of both kernels below.  lg: the row's scores, read only; lgw: the same row where the penalty may
// write it, NULL for a row that is never written (sample_fan_kernel: several workgroups read one row).
__device__ __forceinline__ void sample_row(const float* lg, float* lgw, int row, int seq, int vocab, float penalty, const float* orig_row, const SeqState& st,
                                           const SampleLaunch& p) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    __shared__ SelShared s;
    __shared__ double rs[16];
    __shared__ int ri[16], rk[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ng = st.ngen[seq] < st.gen_cap ? st.ngen[seq] : st.gen_cap;       // (a KV cache never holds more; cr_op_sample's hist_len may)
    if (lgw && penalty != 1.0f && ng > 0) apply_penalty(lgw, st.hist(seq), ng, penalty, tid, orig_row);
    const float temp = st.temp[seq];
    int64_t id;
    int kept = 0;
    if (!(temp > 0.f)) {                                    // greedy row: pick_kernel's argmax
        argmax_row(lg, vocab, tid, bv, bi);
        id = bi[0];
    } else {
        // min / max of z; a NaN score is never kept (its key lies above every other, so it stays outside [kmin, kmax])
        uint32_t kmn = 0xffffffffu, kmx = 0;
        for (int i = tid; i < vocab; i += 1024) {
            const float z = zval(lg, i, temp);
            if (isnan(z)) continue;
            const uint32_t k = fkey(z);
            kmn = k < kmn ? k : kmn; kmx = k > kmx ? k : kmx;
        }
        if (tid == 0) { s.kmin = 0xffffffffu; s.kmax = 0; }
        __syncthreads();
        atomicMin(&s.kmin, kmn); atomicMax(&s.kmax, kmx);
        __syncthreads();
        const uint32_t kmin = s.kmin, kmax = s.kmax;
        __syncthreads();
        const float zmax = kfloat(kmax);
        const int K = st.topk[seq];
        const float P = st.topp[seq];
        uint32_t thr = kmin;
        const bool usable = kmin <= kmax;                       // false: every score is NaN
        if (usable && K > 0 && K < vocab) thr = select_key<false>(lg, vocab, temp, zmax, kmin, kmax, (unsigned long long)(vocab - K), 0.f, s, tid);
        if (usable && P < 1.0f) thr = select_key<true>(lg, vocab, temp, zmax, thr, kmax, 0ull, (float)(1.0 - (double)P), s, tid);
        // the draw over the kept ids: Philox words per group of four ids
        const uint64_t seed = st.seed[seq];
        const uint32_t stp = (uint32_t)(p.step ? p.step[row] : ng);
        double best = -INFINITY; int besti = 0x7fffffff;
        for (int q = tid; q * 4 < vocab; q += 1024) {
            bool have = false;
            uint32_t x[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = q * 4 + e;
                if (i >= vocab) break;
                const float z = zval(lg, i, temp);
                const uint32_t k = fkey(z);
                if (!usable || k < thr || k > kmax) continue;
                kept++;
                if (!have) {
                    x[0] = (uint32_t)q; x[1] = stp; x[2] = 0; x[3] = 0;
                    philox4x32_10(x, seed);
                    have = true;
                }
                const double u = ((double)(x[e] >> 8) + 0.5) * 0x1p-24;
                const double sc = (double)z - log(-log(u));
                if (sc > best) { best = sc; besti = i; }          // ids ascend within a thread: the first of equal scores stays
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double b2 = __shfl_xor(best, o, 64);
            const int i2 = __shfl_xor(besti, o, 64);
            if (b2 > best || (b2 == best && i2 < besti)) { best = b2; besti = i2; }
            kept += __shfl_xor(kept, o, 64);
        }
        if (lane == 0) { rs[w] = best; ri[w] = besti; rk[w] = kept; }
        __syncthreads();
        best = rs[0]; besti = ri[0]; kept = rk[0];
        for (int k = 1; k < 16; k++) {
            if (rs[k] > best || (rs[k] == best && ri[k] < besti)) { best = rs[k]; besti = ri[k]; }
            kept += rk[k];
        }
        id = besti;
        if (besti == 0x7fffffff) {                             // no kept score above -inf (all -inf or NaN): the greedy pick's id
            __syncthreads();
            argmax_row(lg, vocab, tid, bv, bi);
            id = bi[0];
        }
    }
    if (tid == 0) {
        if (p.out_ids) p.out_ids[row] = id;
        if (p.out_kept) p.out_kept[row] = kept;
        if (p.append) st.append(seq, id, ng, p.len_add);
    }
}

__global__ __launch_bounds__(1024) void sample_kernel(Rows r, SeqState s, SampleLaunch p) {
    const int row = blockIdx.x;
    const int seq = r.seq(row);
    if (s.beam_row(seq)) return;                            // a beam row: beam.hip picks for it
    float* lg = r.row(row);
    sample_row(lg, lg, row, seq, r.vocab, r.penalty, r.orig_row(row), s, p);
}

// cr_kv_fanout's picks: workgroup j draws the first id of sequence dsts.seq[j] from the ONE row `lg` (the raw last row of the source's prefill), which no
// workgroup writes -- the sequences hold no ids yet, so there is no penalty to apply -- and appends it with the stop check; the cached length stays.
__global__ __launch_bounds__(1024) void sample_fan_kernel(const float* __restrict__ lg, int vocab, FanSeqs dsts, SeqState s) {
    const int row = blockIdx.x;
    sample_row(lg, nullptr, row, dsts.seq[row], vocab, 1.0f, nullptr, s, SampleLaunch{nullptr, 1, 0, nullptr, nullptr});
}

}  // namespace

int launch_sample_fan(const float* row, int vocab, const FanSeqs& dsts, const SeqState& s, hipStream_t st) {
    hipLaunchKernelGGL(sample_fan_kernel, dim3(dsts.n), dim3(1024), 0, st, row, vocab, dsts, s);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_sample(const Rows& r, const SeqState& s, const SampleLaunch& p, hipStream_t st) {
    hipLaunchKernelGGL(sample_kernel, dim3(r.n), dim3(1024), 0, st, r, s, p);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

extern "C" int cr_op_sample(cr_ctx* c, const float* logits, int n, int vocab, const int64_t* history, int hist_cap, const int32_t* hist_len,
                            float penalty, const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seed,
                            const int32_t* step, int64_t* out_ids, int32_t* out_kept, void* stream) {
    if (!c || !logits || n <= 0 || vocab <= 0 || !hist_len || (!history && hist_cap > 0) || hist_cap < 0 || hist_cap > 4096 || !temperature ||
        !top_k || !top_p || !seed || !step || !out_ids || !out_kept || !(penalty > 0.f))
        return cr_fail(CR_ERR_ARG, "cr_op_sample: bad argument");
    CR_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    CR_TRY(ws_ensure(c, (size_t)n * vocab * 4));
    float* lg = (float*)c->ws;
    CR_HIP(hipMemcpyAsync(lg, logits, (size_t)n * vocab * 4, hipMemcpyDeviceToDevice, st));
    SeqState s{};                                            // the arrays stand for per-sequence state: row = sequence, nothing is appended
    s.ngen = const_cast<int32_t*>(hist_len); s.gen = const_cast<int64_t*>(history); s.gen_cap = hist_cap;
    s.temp = const_cast<float*>(temperature); s.topk = const_cast<int32_t*>(top_k); s.topp = const_cast<float*>(top_p); s.seed = const_cast<uint64_t*>(seed);
    return launch_sample({lg, vocab, vocab, n, nullptr, nullptr, penalty}, s, {step, 0, 0, out_ids, out_kept}, st);
}

// Cache operations between turns of a conversation about one page (cr_kv_truncate, cr_kv_fork; session.py).
//
//   kv_truncate_kernel  state only: the listed sequences hold n_tokens cached positions and nothing else that cr_kv_reset forgets.  Cache rows are not touched:
//                       rows at positions >= n_tokens are dead and the next append overwrites them.
//   kv_fork_kernel      the prefix [0, n_tokens) of one sequence to up to 64 others.  The cache is [layers][n_seqs][8][max_tokens][128] bf16, so the prefix of one
//                       (layer, KV head, K|V) is ONE contiguous run of n_tokens * 256 bytes: blockIdx.y names the run, blockIdx.x a 16 KiB tile of it.  A thread
//                       loads four 16-byte pieces of the source (all four in flight before the first store) and stores them to every destination, so the source
//                       is read once however many branches there are: traffic (1 + n_dst) * layers * 16 * n_tokens * 256 bytes.  The grid follows the byte
//                       count; positions >= n_tokens of a destination are never written.  The first workgroup also writes the destinations' state, which no
//                       other workgroup reads.  src is never a destination (checked on the host), so no address is both read and written.
// No atomics of any kind; plain vector stores only.
#include "ctx.hpp"
#include "kvops.hpp"

namespace {

constexpr int FORK_THREADS = 256, FORK_PIECES = 4, FORK_TILE = FORK_THREADS * FORK_PIECES;      // 16-byte pieces per workgroup

__device__ __forceinline__ void kv_clear_state(const KvState& s, int seq, int n_tokens) {
    s.len[seq] = n_tokens;
    s.ngen[seq] = 0;
    s.stop[1 + s.n_seqs + seq] = 0;                 // not stopped
    s.stop[1 + 2 * s.n_seqs + seq] = -1;            // no EOS id
    s.stop[1 + 3 * s.n_seqs + seq] = 0;             // no budget
    s.temp[seq] = 0.f;                              // greedy
    if (s.lpn) { s.lpn[seq] = 0; s.lpdone[seq] = 0; }
    if (s.con_on) s.con_on[seq] = 0;
}

__global__ __launch_bounds__(64) void kv_truncate_kernel(KvState s, KvSeqs seqs, int n_tokens) {
    if ((int)threadIdx.x < seqs.n) kv_clear_state(s, seqs.seq[threadIdx.x], n_tokens);
}

__global__ __launch_bounds__(FORK_THREADS) void kv_fork_kernel(KvState s, bf16* __restrict__ k, bf16* __restrict__ v, int64_t per_layer, int max_tokens, int src,
                                                               KvSeqs dsts, int n_tokens) {
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < dsts.n) kv_clear_state(s, dsts.seq[tid], n_tokens);
    const int run = blockIdx.y;                     // (layer, KV head, K|V)
    const int layer = run >> 4, head = (run >> 1) & 7;
    bf16* base = ((run & 1) ? v : k) + (int64_t)layer * per_layer + (int64_t)head * max_tokens * 128;
    const int64_t per_seq = (int64_t)8 * max_tokens * 128;
    const int pieces = n_tokens * 16;               // 16-byte pieces of the run (max_tokens <= 32768: fits an int)
    const int p0 = blockIdx.x * FORK_TILE + tid;
    const uint4* sp = (const uint4*)(base + src * per_seq);
    uint4 r[FORK_PIECES];
#pragma unroll
    for (int u = 0; u < FORK_PIECES; u++) {
        const int p = p0 + u * FORK_THREADS;
        if (p < pieces) r[u] = sp[p];
    }
    for (int j = 0; j < dsts.n; j++) {
        uint4* dp = (uint4*)(base + dsts.seq[j] * per_seq);
#pragma unroll
        for (int u = 0; u < FORK_PIECES; u++) {
            const int p = p0 + u * FORK_THREADS;
            if (p < pieces) dp[p] = r[u];
        }
    }
}

}  // namespace

int launch_kv_truncate(const KvState& s, const KvSeqs& seqs, int n_tokens, hipStream_t st) {
    hipLaunchKernelGGL(kv_truncate_kernel, dim3(1), dim3(64), 0, st, s, seqs, n_tokens);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int launch_kv_fork(const KvState& s, bf16* k, bf16* v, int64_t per_layer, int layers, int max_tokens, int src, const KvSeqs& dsts, int n_tokens, hipStream_t st) {
    const int pieces = n_tokens * 16;
    hipLaunchKernelGGL(kv_fork_kernel, dim3((pieces + FORK_TILE - 1) / FORK_TILE, layers * 16), dim3(FORK_THREADS), 0, st, s, k, v, per_layer, max_tokens, src, dsts,
                       n_tokens);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

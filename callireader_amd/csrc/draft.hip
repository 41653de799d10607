// Draft-verified greedy decoding: the device side of cr_llm_decode_draft behind the LM head (llm.hip runs the decoder over the rows).
//
// A sequence with G generated ids and k drafted ids d[0 .. k) is k + 1 rows of the step: row r was fed g[G - 1] (r = 0) or d[r - 1] and sits at position L + r, so
// its logits are the model's after g ++ d[0 .. r).  Three kernels:
//   draft_stage_kernel   d[0 .. k) into the history slots g[G .. G + k): dead slots (the count stays G) that make "history plus draft prefix" one contiguous run,
//                        which is what the embedding of the rows and pick.hpp's apply_penalty read.
//   draft_pick_kernel    pick_kernel's penalty and first-max-wins argmax per row, over g[0 .. G + r), appending nothing: the pick p_r goes to a scratch array.
//   draft_accept_kernel  one thread per sequence: a = the longest prefix with p_j == d[j]; p_0 .. p_a are appended in order (p_j == d[j] below a, so only slot
//                        G + a changes), each with seqstate.hpp's stop check at its own count, ending behind the first id that stops the sequence; the id count and
//                        the cached length grow by the ids appended.  Cache rows past the new length are dead, as after cr_kv_truncate.
// An accepted id is by construction the id the plain greedy step would have picked, so the ids never depend on what the draft holds.
#include "draft.hpp"

namespace {

__global__ __launch_bounds__(64) void draft_stage_kernel(const int32_t* __restrict__ seqs, const DraftIndex ix, int n, SeqState s) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const int q = seqs[ix.row0[i]], k = ix.klen[i], ng = s.ngen[q];
    for (int j = 0; j < k && ng + j < s.gen_cap; j++) s.hist(q)[ng + j] = ix.ids[i * DRAFT_MAX + j];
}

// One workgroup of 1024 per row, as pick_kernel; off == NULL: every row is its sequence's only one
__global__ __launch_bounds__(1024) void draft_pick_kernel(Rows r, SeqState s, const int32_t* __restrict__ off, int32_t* __restrict__ picks) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int seq = r.seqs[row];
    float* lg = r.row(row);
    const int ng = min(s.ngen[seq] + (off ? off[row] : 0), s.gen_cap);      // the history and the drafted ids before this row
    if (r.penalty != 1.0f && ng > 0) apply_penalty(lg, s.hist(seq), ng, r.penalty, tid, r.orig_row(row));
    argmax_row(lg, r.vocab, tid, bv, bi);
    if (tid == 0) picks[row] = bi[0];
}

__global__ __launch_bounds__(64) void draft_accept_kernel(const int32_t* __restrict__ seqs, const DraftIndex ix, int n, SeqState s) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const int r0 = ix.row0[i], k = ix.klen[i], q = seqs[r0], ng = s.ngen[q];
    int64_t* g = s.hist(q);
    int a = 0;
    while (a < k && ng + a < s.gen_cap && ix.picks[r0 + a] == g[ng + a]) a++;
    int m = 0;
    for (int j = 0; j <= a && ng + j < s.gen_cap; j++) {
        const int64_t id = ix.picks[r0 + j];
        g[ng + j] = id;
        m = j + 1;
        if (s.stop.check(q, id, ng + m)) break;              // this id stopped the sequence: nothing is appended behind it
    }
    s.ngen[q] = ng + m;
    s.len[q] += m;
    ix.app[i] = m;
}

}  // namespace

int launch_draft_stage(const Rows& r, const SeqState& s, const DraftLaunch& p, hipStream_t st) {
    if (p.n < 1 || p.n > 64 || r.n < p.n) return CR_ERR_ARG;
    if (!p.windows) return CR_OK;
    hipLaunchKernelGGL(draft_stage_kernel, dim3(1), dim3(64), 0, st, r.seqs, p.ix, p.n, s);
    return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
}

int launch_draft_pick_accept(const Rows& r, const SeqState& s, const DraftLaunch& p, hipStream_t st) {
    if (p.n < 1 || p.n > 64 || r.n < p.n) return CR_ERR_ARG;
    hipLaunchKernelGGL(draft_pick_kernel, dim3(r.n), dim3(1024), 0, st, r, s, p.windows ? p.ix.off : nullptr, p.ix.picks);
    hipLaunchKernelGGL(draft_accept_kernel, dim3(1), dim3(64), 0, st, r.seqs, p.ix, p.n, s);
    return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
}

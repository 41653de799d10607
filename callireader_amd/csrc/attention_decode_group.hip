// The group form of the streaming decode attention (attention_decode.hip) for rows that share a prompt (cr_kv_fork_shared).  A translation unit of its own:
// it is compiled with -fno-slp-vectorize (callireader_amd/build.py).  With the keys of a split live across the rows of a chunk, the SLP pass's packed P.V (every V
// converted to fp32 up front, v_pk_fma_f32 over all 16 keys per output pair) no longer fits 256 registers and spills the keys themselves (142 VGPRs to scratch);
// scalar FMAs in key order give the same bits (fma per element either way) in 234 registers.  attention_decode.hip keeps its flags, so a launch without shares
// runs the code it always ran.
#include "attention_decode_row.hpp"

namespace {

// The group form (a shared prompt, cr_kv_fork_shared): a workgroup = one 256-key split of one (chunk of up to 8 rows, KV head), below the chunk's shared length.
// It issues the 16 K and 16 V loads of each wave from the SOURCE slot exactly once, as the per-row kernel does, keeps them in registers and runs split_row for
// every row of the chunk: the row's four q heads (the next row's are requested before the current row's arithmetic), then the partial into THAT row's slot of
// part_o / part_ml.  A shared split is full for every member (split * 256 + 255 < shared length <= every member's key count): no clamp, no -inf.  LDS is
// reused across the rows behind a barrier.  HBM traffic of the shared splits falls by the chunk's size; the vector work per row is what it was.
// Resource summary (hipcc -O3 --offload-arch=gfx950 -fno-slp-vectorize -Rpass-analysis=kernel-resource-usage): 234 VGPRs, 0 spilled, no scratch, 33 280 bytes of LDS,
// two workgroups per CU -- beside the per-row kernel's 190 (the FOLD instances 234), read from the same summary.
template <bool DIV>
__global__ __launch_bounds__(256, 2) void decode_attn_group_kernel(const AttnParams p) {
    __shared__ __attribute__((aligned(16))) float s_o[16][NQ][HD];
    __shared__ float s_ml[16][NQ][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, head = blockIdx.y;
    const int32_t* ch = p.share_chunks + (int64_t)blockIdx.z * ATTN_SHARE_CHUNK_INTS;
    const int src = __builtin_amdgcn_readfirstlane(ch[0]), nsp = __builtin_amdgcn_readfirstlane(ch[1]), n = __builtin_amdgcn_readfirstlane(ch[2]);
    if (split >= nsp) return;                                 // a chunk with fewer shared splits than the launch's longest
    const int ksub = lane >> 4, c = lane & 15;
    const int key0 = split * 256 + wave * 64 + ksub;
    const bf16* Kb = p.K + (int64_t)src * p.k_bs + (int64_t)head * p.k_hs;
    const bf16* Vb = p.V + (int64_t)src * p.v_bs + (int64_t)head * p.v_hs;
    const unsigned k_rs = (unsigned)p.k_rs, v_rs = (unsigned)p.v_rs, lane_off = (unsigned)c * 8u;
    bf16x8 q[NQ];
    {
        const bf16* qp = p.Q + (int64_t)__builtin_amdgcn_readfirstlane(ch[4]) * p.q_bs + (int64_t)head * p.q_hs + lane_off;
#pragma unroll
        for (int h = 0; h < NQ; h++) q[h] = *(const bf16x8*)(qp + (int64_t)h * p.q_rs);
    }
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 kr[IT], vr[IT];
#pragma unroll
    for (int i = 0; i < IT; i++) kr[i] = __builtin_nontemporal_load((const bf16x8*)(Kb + ((unsigned)(key0 + 4 * i) * k_rs + lane_off)));
#pragma unroll
    for (int i = 0; i < IT; i++) vr[i] = __builtin_nontemporal_load((const bf16x8*)(Vb + ((unsigned)(key0 + 4 * i) * v_rs + lane_off)));
    __builtin_amdgcn_sched_barrier(0);
    for (int m = 0; m < n; m++) {
        const int batch = __builtin_amdgcn_readfirstlane(ch[4 + m]);      // uniform: the row's addresses stay scalar
        const int64_t prow = (((int64_t)batch * p.H + head) * p.nsplit + split) * NQ;
        // the keys are the same for every row, and left to itself the compiler hoists what split_row derives from them alone (V as fp32: 128 registers) out of
        // this loop and spills; an empty asm that "writes" them keeps each row's code the per-row kernel's
#pragma unroll
        for (int i = 0; i < IT; i++) {
            u32x4_t a = __builtin_bit_cast(u32x4_t, kr[i]), b = __builtin_bit_cast(u32x4_t, vr[i]);
            asm volatile("" : "+v"(a), "+v"(b));
            kr[i] = __builtin_bit_cast(bf16x8, a); vr[i] = __builtin_bit_cast(bf16x8, b);
        }
        if (m > 0) {
            const bf16* qp = p.Q + (int64_t)batch * p.q_bs + (int64_t)head * p.q_hs + lane_off;
#pragma unroll
            for (int h = 0; h < NQ; h++) q[h] = *(const bf16x8*)(qp + (int64_t)h * p.q_rs);
        }
        split_row<DIV>(p, q, kr, vr, key0, 0x7fffffff, prow, s_o, s_ml);
        __syncthreads();                                      // the next row writes the LDS this one has just read
    }
}

}  // namespace

int launch_decode_attn_group(const AttnParams& p, hipStream_t stream) {
    const dim3 grid(p.share_splits, p.H, p.share_n);
    if (p.s_div != 1.0f) hipLaunchKernelGGL((decode_attn_group_kernel<true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((decode_attn_group_kernel<false>), grid, dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? CR_OK : CR_ERR_HIP;
}

"""The attention reference shared by test_gpu_ops.py and test_gpu_prefill_attention.py: plain PyTorch fp32 with the reference model's bf16 rounding
points written out (attn_ref), the same operation in float64 without any rounding (attn_f64: what attn_ref's own error is measured against), and both
over the segments of a prefill launch (segments_ref); the resampler's attention with ITS rounding points (perceiver_attn_ref, test_gpu_calli_ops.py)."""
import torch


def rb(t):
    return t.to(torch.bfloat16).float()


def attn_ref(q, k, v, causal, q_pos0, prescale, s_div):
    """q (B,H,Sq,D), k/v (B,H,Sk,D) float tensors holding bf16 values; reference rounding points."""
    if prescale != 1.0:
        q = rb(q * prescale)
    s = rb(q @ k.transpose(-1, -2))
    if s_div != 1.0:
        s = rb(s / s_div)
    if causal:
        Sq, Sk = s.shape[-2:]
        qpos = q_pos0 + torch.arange(Sq, device=s.device)[:, None]
        s = s.masked_fill(torch.arange(Sk, device=s.device)[None, :] > qpos, float('-inf'))
    p = rb(torch.softmax(s, dim=-1))
    return rb(p @ v)


def attn_f64(q, k, v, causal, q_pos0, prescale, s_div):
    """The same attention in float64, nothing rounded: softmax(q k^T * prescale / s_div + mask) v."""
    q, k, v = q.double(), k.double(), v.double()
    s = (q * prescale) @ k.transpose(-1, -2) / s_div
    if causal:
        Sq, Sk = s.shape[-2:]
        qpos = q_pos0 + torch.arange(Sq, device=s.device)[:, None]
        s = s.masked_fill(torch.arange(Sk, device=s.device)[None, :] > qpos, float('-inf'))
    return torch.softmax(s, dim=-1) @ v


def segments_ref(q, kc, vc, segs, s_div, fn=attn_ref):
    """Causal GQA attention of a segment launch, evaluated per KV head with `fn`.  q (rows, H, D), kc / vc (slots, H_kv, max_tokens, D) bf16,
    segs = [(first row, rows S, first position pos0, cache slot)]: row r of a segment attends over positions 0 .. pos0 + r of its slot, and ONLY
    positions < pos0 + S of that slot are read.  Returns {segment index: (S, H, D)} in fn's precision."""
    H, n_kv = q.shape[1], kc.shape[1]
    g = H // n_kv
    out = {}
    for i, (row0, S, pos0, slot) in enumerate(segs):
        Sk = pos0 + S
        heads = []
        for kvh in range(n_kv):
            qh = q[row0:row0 + S, kvh * g:(kvh + 1) * g].float().permute(1, 0, 2)[None]            # (1, g, S, D)
            kh = kc[slot, kvh, :Sk].float()[None, None].expand(1, g, Sk, -1)
            vh = vc[slot, kvh, :Sk].float()[None, None].expand(1, g, Sk, -1)
            heads.append(fn(qh, kh, vh, True, pos0, 1.0, s_div)[0])                                  # (g, S, D)
        out[i] = torch.cat(heads, 0).permute(1, 0, 2)
    return out


P_NQ, P_NKV, P_HEADS, P_DH = 3, 259, 8, 64


def perceiver_heads(q, kv):
    """cr_op_perceiver_attention's operands per (tile, head): q (T * 3, 512), kv (T * 259, 1024) [K | V] -> q (T, 8, 3, 64), k, v (T, 8, 259, 64), same dtype."""
    T = q.shape[0] // P_NQ
    assert q.shape == (T * P_NQ, P_HEADS * P_DH) and kv.shape == (T * P_NKV, 2 * P_HEADS * P_DH)
    qh = q.reshape(T, P_NQ, P_HEADS, P_DH).permute(0, 2, 1, 3)
    kvh = kv.reshape(T, P_NKV, 2, P_HEADS, P_DH).permute(2, 0, 3, 1, 4)
    return qh, kvh[0], kvh[1]


def perceiver_attn_ref(q, kv, exact=False, *, drop_keys=(), round_sub=True, round_p=True):
    """PerceiverAttention's softmax(q k^T) v (perceiver_resampler.py:43-51) on bf16 q (T * 3, 512) and kv (T * 259, 1024): fp32 with the reference's
    rounding points written out -- q * 0.125 -> bf16 (exact), sim -> bf16, sim - amax -> bf16, fp32 softmax -> bf16, attn @ v summed in fp32 -> bf16.
    Returns (T * 3, 512) fp32 holding bf16 values; exact=True: the same operation in float64, nothing rounded.
    The keyword-only arguments are deliberate MISTAKES for test_attn_ref_cpu.py, which shows which of them the GPU tests' bound can see: keys left out of
    the softmax, sim - amax left unrounded, the probabilities left unrounded."""
    qh, k, v = perceiver_heads(q, kv)
    if exact:
        sim = (qh.double() * 0.125) @ k.double().transpose(-1, -2)
        out = torch.softmax(sim, dim=-1) @ v.double()
    else:
        sim = rb(rb(qh.float() * 0.125) @ k.float().transpose(-1, -2))
        for key in drop_keys:
            sim[..., key] = float('-inf')
        sim = sim - sim.amax(dim=-1, keepdim=True)
        if round_sub:
            sim = rb(sim)
        attn = torch.softmax(sim, dim=-1)
        if round_p:
            attn = rb(attn)
        out = rb(attn @ v.float())
    return out.permute(0, 2, 1, 3).reshape(q.shape[0], P_HEADS * P_DH)

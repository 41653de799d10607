"""Reference of the grounding tests: the decoder stack as a layer loop built from oracle.internlm2's own functions, which keeps every layer's fp32 softmax
(the reference model can only expose it through output_attentions=True), and the span mass computed from that.  TEST INFRASTRUCTURE ONLY."""
import math

import torch
import torch.nn.functional as F

from oracle.internlm2 import apply_rope, causal_mask, mlp, rms_norm, rope_tables


def layer_softmax(sd, n_layers, embeds, dtype=torch.bfloat16, n_heads=32, n_kv=8, eps=1e-5):
    """embeds [S, D] -> per layer the softmax [n_heads, S, S] in fp32, as modeling_internlm2.py:393-409 computes it with activations and weights of `dtype`
    (bfloat16: the model as it runs; float32: the same weights without any rounding of activations)."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith('language_model.model.layers.')}
    x = embeds[None].to(dtype)
    B, S, D = x.shape
    hd, groups = D // n_heads, n_heads // n_kv
    cos_t, sin_t = rope_tables(hd)
    pos = torch.arange(S).unsqueeze(0)
    out = []
    with torch.no_grad():
        for i in range(n_layers):
            p = f'language_model.model.layers.{i}.'
            h = rms_norm(x, sd[p + 'attention_norm.weight'], eps)
            qkv = F.linear(h, sd[p + 'attention.wqkv.weight']).view(B, S, n_kv, groups + 2, hd)
            q = qkv[..., :groups, :].reshape(B, S, n_heads, hd).transpose(1, 2)
            k = qkv[..., -2, :].transpose(1, 2)
            v = qkv[..., -1, :].transpose(1, 2)
            q, k = apply_rope(q, k, cos_t[:S].to(dtype), sin_t[:S].to(dtype), pos)
            kr = k[:, :, None].expand(B, n_kv, groups, S, hd).reshape(B, n_heads, S, hd)
            vr = v[:, :, None].expand(B, n_kv, groups, S, hd).reshape(B, n_heads, S, hd)
            w = torch.matmul(q, kr.transpose(2, 3)) / math.sqrt(hd)
            w = w + causal_mask(S, 0, dtype)
            w = F.softmax(w, dim=-1, dtype=torch.float32)
            out.append(w[0])
            o = torch.matmul(w.to(dtype), vr).transpose(1, 2).contiguous().reshape(B, S, D)
            x = x + F.linear(o, sd[p + 'attention.wo.weight'])
            x = x + mlp(sd, p, rms_norm(x, sd[p + 'ffn_norm.weight'], eps))
    return out


def span_mass(probs, rows, spans, layers):
    """probs = layer_softmax's list, rows = the grounded rows, spans = [(start, end), ...], layers = (layer0, layer1) -> [len(rows), len(spans)] float64: the
    mean over the layers' heads of the probability every row puts on every span"""
    l0, l1 = layers
    out = torch.zeros(len(rows), len(spans), dtype=torch.float64)
    for l in range(l0, l1):
        P = probs[l][:, rows].double()
        for b, (s, e) in enumerate(spans):
            if e > s:
                out[:, b] += P[:, :, s:e].sum(-1).mean(0)
    return out / (l1 - l0)

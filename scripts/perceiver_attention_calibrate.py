#!/usr/bin/env python3
"""The figures behind DATA_FLOOR of tests/test_gpu_calli_ops.py, next to prefill_attention_calibrate.py and by the same rule.  For every data case of
the perceiver attention and its first 1 / 5 / 37 tiles: how far perceiver_attn_ref (the reference model's bf16 rounding points) lies from the same
attention in float64 -- the largest |ref - f64|, and the floor: the smallest atol at which it passes assert_close(rtol = RTOL) against float64.  The test
allows max(ATOL, 2 x floor).  CPU only for those; with a GPU it also prints the kernel's worst excess over rtol * |ref| (cr_op_perceiver_attention).
--stage: the statistics of the stage's own layer-0 q / kv (the oracle on test_gpu_calli.py's features) that random_case copies, and what the
stage-level bound of test_resampler makes of four mistakes in the oracle's attention (the table of DESIGN.md)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_calli_ops as T  # noqa: E402
from attn_ref import perceiver_attn_ref, perceiver_heads  # noqa: E402


def floors():
    gpu = torch.cuda.is_available()
    if gpu:
        from callireader_amd import engine
    for name in T.DATA_CASES:
        q, kv, ref = T.data_case(name)
        exact = perceiver_attn_ref(q, kv, exact=True)
        assert torch.isfinite(ref).all() and torch.isfinite(exact).all()
        fl, notes = [], []
        for n in T.TS:
            r, e = ref[:n * 3].double(), exact[:n * 3]
            dev = (r - e).abs()
            fl.append(max(0.0, float((dev - T.RTOL * e.abs()).max())))
            notes.append(f'T={n}: max |ref - f64| {float(dev.max()):.3e}, max |f64| {float(e.abs().max()):.2f}, allowed {max(T.ATOL, 2 * fl[-1]):.3e}')
        print(f"    '{name}': ({', '.join(f'{f:.3e}' for f in fl)}),      # " + '; '.join(notes), flush=True)
        if gpu:
            for n in T.TS:
                o = T.launch(engine, *T.first_tiles(q, kv, n), 0).float()
                r = ref[:n * 3]
                print(f'        kernel T={n}: worst excess over rtol * |ref| {float(((o - r).abs() - T.RTOL * r.abs()).max()):.3e}, finite {bool(torch.isfinite(o).all())}', flush=True)


def stage():
    import torch.nn.functional as F
    from callireader_amd import synthetic
    from callireader_amd.config import ModelDims
    from oracle import calli_align as o
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=2, vocab=5003)
    sd = synthetic.make_state_dict(dims, parts=('resampler',), seed=0)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(5, 256, 4096, generator=g) * 0.7).to(torch.bfloat16)                     # test_gpu_calli.py's features
    p, D = 'resampler.layers.0.0.', 4096
    xn = F.layer_norm(x, (D,), sd[p + 'norm_media.weight'], sd[p + 'norm_media.bias'])
    ln = F.layer_norm(sd['resampler.learns'].unsqueeze(0).expand(5, -1, -1), (D,), sd[p + 'norm_learns.weight'], sd[p + 'norm_learns.bias'])
    q = F.linear(ln, sd[p + 'to_q.weight']).reshape(15, 512)
    kv = F.linear(torch.cat((xn, ln), -2), sd[p + 'to_kv.weight']).reshape(5 * 259, 1024)
    qh, k, v = perceiver_heads(q, kv)
    sim = (qh.float() * 0.125) @ k.float().transpose(-1, -2)
    pr = sim.softmax(-1)
    print(f'layer 0: std q {float(q.float().std()):.3f}, k {float(k.float().std()):.3f}, v {float(v.float().std()):.3f}, scores {float(sim.std()):.3f}; '
          f'largest weight of a row {float(pr.amax(-1).min()):.3f} .. {float(pr.amax(-1).max()):.3f}, latent mass {float(pr[..., 256:].sum(-1).mean()):.4f}')
    with torch.no_grad():
        ref = o.resampler_forward(sd, x, dims.rs_depth).float()
        true = o.perceiver_softmax_pv

        def mutated(fn):
            o.perceiver_softmax_pv = fn
            try:
                return o.resampler_forward(sd, x, dims.rs_depth).float()
            finally:
                o.perceiver_softmax_pv = true

        def masked(keys):
            def fn(q, k, v, dim_head=64):
                sim = torch.einsum('bhid,bhjd->bhij', q * dim_head ** -0.5, k)
                sim[..., keys] = float('-inf')
                return torch.einsum('bhij,bhjd->bhid', (sim - sim.amax(-1, keepdim=True)).softmax(-1), v)
            return fn

        def swapped(q, k, v, dim_head=64):
            v = v.clone()
            v[..., [256, 258], :] = v[..., [258, 256], :]
            return true(q, k, v, dim_head)
        for what, fn in (('key 258 (last latent) masked out', masked([258])), ('key 255 masked out', masked([255])),
                         ('all three latent keys masked out', masked([256, 257, 258])), ('V rows of keys 256 and 258 swapped', swapped)):
            got = mutated(fn)
            print(f'| {what} | {float((got - ref).norm() / ref.norm()):.2e} | {float((got - ref).abs().max() / ref.abs().max()):.2e} |')


if __name__ == '__main__':
    stage() if '--stage' in sys.argv else floors()

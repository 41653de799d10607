#!/usr/bin/env python3
"""The figures behind PEAKED_FLOOR of tests/test_gpu_prefill_attention.py.  For every peaked case (and the random one) at both first positions:
how far attn_ref (the reference model's bf16 rounding points) lies from a float64 softmax attention of the same inputs -- the largest |ref - f64|, and
the floor: the smallest atol at which attn_ref passes assert_close(rtol = RTOL) against float64.  The test allows max(ATOL, 2 x floor).  CPU only for
those; with a GPU it also prints the kernel's worst excess over rtol * |ref| per case (cr_op_attention_segments)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_prefill_attention as T  # noqa: E402
from attn_ref import attn_f64, segments_ref  # noqa: E402

gpu = torch.cuda.is_available()
if gpu:
    from callireader_amd import engine
for name in T.PEAKED:
    for pos0 in T.PEAK_POS0:
        q, kc, vc, segs = T.peaked_case(name, pos0)
        ref = segments_ref(q, kc, vc, segs, T.SDIV)[0].double()
        exact = segments_ref(q, kc, vc, segs, T.SDIV, fn=attn_f64)[0]
        assert torch.isfinite(ref).all() and torch.isfinite(exact).all()
        dev = (ref - exact).abs()
        floor = max(0.0, float((dev - T.RTOL * exact.abs()).max()))
        line = f"    ('{name}', {pos0}): {floor:.3e},      # max |ref - f64| {float(dev.max()):.3e}, max |f64| {float(exact.abs().max()):.2f}; allowed {max(T.ATOL, 2 * floor):.3e}"
        if gpu:
            dq, dk, dv = T.to_dev(q, kc, vc)
            o = T.launch(engine, dq, dk, dv, segs)[:segs[0][1]].float().cpu().double()
            line += f'; kernel: worst excess over rtol * |ref| {float(((o - ref).abs() - T.RTOL * ref.abs()).max()):.3e}, finite {bool(torch.isfinite(o).all())}'
        print(line, flush=True)

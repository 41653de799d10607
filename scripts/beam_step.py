"""Cost of a beam-search decode step against the greedy step, at full InternVL2-8B dims (random weights, 512-token prompts), device events, one process:

  greedy: cr_llm_decode over 64 greedy rows (the yardstick: the same kernels as before beam search existed);
  beam:   cr_llm_decode over 16 pages x 4 beams = 64 rows, in windows of 16 steps at several generated lengths g -- the re-order moves every generated
          position of every beam whose source changed, so the step grows with g.  Random weights give nearly flat next-token distributions: the beams
          change source often, which is the expensive end of what real pages do.

`python scripts/beam_step.py OUT.json [--short]` (--short: few steps, for a run under rocprofv3 --kernel-trace; scripts/beam_trace_medians.py reads its CSV)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from callireader_amd.config import ModelDims


def window(eng, kv, rows, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        eng.decode(kv, rows, penalty=1.5)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main(out=None, short=False, S=512, P=16, Bn=4):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    max_new = 64 if short else 300
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, max_tokens=S + max_new + 8, max_pages=P * Bn)
    eng = m.engine
    kv = eng.kv_alloc(P * Bn, S + max_new + 8)
    g = torch.Generator(device='cuda').manual_seed(1)
    prompts = [(torch.randn(S, 4096, device='cuda', generator=g) * 0.02).bfloat16() for _ in range(P * Bn)]
    res = {'prompt_tokens': S, 'pages': P, 'num_beams': Bn, 'rows': P * Bn, 'window_steps': 8 if short else 16}
    W = res['window_steps']
    # greedy, 64 rows
    kv.reset()
    for i0 in range(0, P * Bn, 16):
        eng.prefill_batch(kv, list(range(i0, i0 + 16)), prompts[i0:i0 + 16], penalty=1.5)
    rows = list(range(P * Bn))
    window(eng, kv, rows, 4)
    res['greedy_ms'] = round(min(window(eng, kv, rows, W) for _ in range(1 if short else 3)), 3)
    print('greedy step', res['greedy_ms'], 'ms', flush=True)
    # 16 pages x 4 beams
    kv.reset()
    for i in range(P):
        kv.set_beam(i * Bn, Bn, 1.0, False, None, max_new)
    eng.prefill_batch(kv, [i * Bn for i in range(P)], prompts[:P], penalty=1.5)
    res['beam_ms_at_g'] = {}
    gen = 1
    for target in ((8, 32) if short else (8, 32, 64, 128, 256)):
        if target - gen > 0:
            window(eng, kv, rows, target - gen)
            gen = target
        ms = window(eng, kv, rows, W)
        res['beam_ms_at_g'][f'{gen}..{gen + W}'] = {'ms': round(ms, 3), 'vs_greedy': round(ms / res['greedy_ms'], 4)}
        gen += W
        print('beam step at g', gen - W, round(ms, 3), 'ms', flush=True)
    done = [kv.beam_result(i * Bn)[2] for i in range(P)]
    res['groups_done_during_run'] = int(sum(done))
    kv.free()
    m.close()
    txt = json.dumps(res, indent=1)
    if out:
        with open(out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    main(args[0] if args else None, short='--short' in sys.argv)

"""Cost of token scores (cr_kv_set_logprobs) for 1, 13 and 64 rows, two ways:

  kernel: one cr_op_logprobs call (the two kernels the prefill / decode launch after the pick, plus the call's own scratch allocation and stream
          synchronise) at vocab 92 553, top_n 1 and 8.  For the kernels' own time run this under rocprofv3 --kernel-trace --stats with --kernel-only:
          logprobs_chunk_kernel + logprobs_merge_kernel against pick_kernel / sample_kernel of the same trace.
  step:   whole decode steps (cr_llm_decode) at full InternVL2-8B dims (random weights, 512-token prompts): scores off, top_n 1, top_n 8, set per
          sequence after a reset; the modes alternate within one process and are timed with device events after warm-up.

`python scripts/logprobs_step.py OUT.json [--kernel-only]`"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from callireader_amd.config import ModelDims
from callireader_amd.engine import op_logprobs

V = 92553
MODES = {'off': 0, 'top1': 1, 'top8': 8}


def step_times(res, steps=16, warm=4, rounds=3, S=512):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, max_tokens=S + 1024, max_pages=64)
    eng, P = m.engine, 64
    kv = eng.kv_alloc(P, S + 1024)
    g = torch.Generator(device='cuda').manual_seed(1)
    prompts = [(torch.randn(S, 4096, device='cuda', generator=g) * 0.02).bfloat16() for _ in range(P)]
    res['step'] = {'prompt_tokens': S, 'steps_per_sample': steps, 'rows': {}}
    for n in (1, 13, 64):
        ms = {md: [] for md in MODES}
        for _ in range(rounds):
            for md, top_n in MODES.items():
                kv.reset()                                           # every mode decodes the same positions of the same prompts
                for s_ in range(n):
                    kv.set_logprobs(s_, top_n)
                for i0 in range(0, n, 16):
                    idx = list(range(i0, min(n, i0 + 16)))
                    eng.prefill_batch(kv, idx, [prompts[i] for i in idx], penalty=1.5)
                for _ in range(warm):
                    eng.decode(kv, list(range(n)), penalty=1.5)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    eng.decode(kv, list(range(n)), penalty=1.5)
                b.record()
                b.synchronize()
                ms[md].append(a.elapsed_time(b) / steps)
        r = {md: round(min(v), 4) for md, v in ms.items()}
        r.update({f'{md}_spread': round(max(v) - min(v), 4) for md, v in ms.items()})
        r.update({f'{md}_vs_off': round(r[md] / r['off'], 4) for md in MODES if md != 'off'})
        res['step']['rows'][n] = r
        print(f'step rows {n}: {r}', flush=True)
    kv.free()
    m.close()


def main(out=None, reps=50, kernel_only=False):
    g = torch.Generator().manual_seed(0)
    res = {'vocab': V, 'reps': reps, 'op_call_us': {}}
    for n in (1, 13, 64):
        lg = (torch.randn(n, V, generator=g) * 2.5).cuda()
        ids = lg.argmax(1)
        res['op_call_us'][n] = {}
        for md, top_n in MODES.items():
            if not top_n:
                continue
            ms = []
            for it in range(reps + 5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                op_logprobs(lg, ids, top_n)
                b.record()
                b.synchronize()
                if it >= 5:
                    ms.append(a.elapsed_time(b))
            res['op_call_us'][n][md] = round(1e3 * sorted(ms)[len(ms) // 2], 1)
    if not kernel_only:
        step_times(res)
    txt = json.dumps(res, indent=1)
    if out:
        with open(out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    main(args[0] if args else None, kernel_only='--kernel-only' in sys.argv)

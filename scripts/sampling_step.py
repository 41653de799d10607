"""Cost of sampled token choice against greedy, two ways, for 1, 13 and 64 rows:

  kernel: one cr_op_sample launch (the kernel the decode step launches) at vocab 92 553 with a 256-id history, penalty 1.5.  The launch copies the
          logits first; that copy is timed on its own (logits_copy_us) and NOT subtracted from the mode columns.
  step:   whole decode steps (cr_llm_decode) at full InternVL2-8B dims (random weights, 512-token prompts): greedy (pick_kernel), top-k 50 sampling
          (the do_sample=True default) and top_k=0, top_p=0.8, set per sequence with cr_kv_set_sampling.

Modes alternate within one process and are timed with device events after warm-up.  `python scripts/sampling_step.py OUT.json [--kernel-only]`
(--kernel-only: the launches alone, e.g. under rocprofv3 --kernel-trace --stats)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from callireader_amd.config import ModelDims
from callireader_amd import _binding as B
from callireader_amd.engine import Engine, _p, _stream

V = 92553
MODES = {'greedy': (0.0, 0, 1.0), 'top_k50': (1.0, 50, 1.0), 'top_p0.8': (1.0, 0, 0.8)}


def step_times(res, steps=16, warm=4, rounds=2, S=512):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, max_tokens=S + 640, max_pages=64)
    eng, P = m.engine, 64
    kv = eng.kv_alloc(P, S + 640)
    kv.reset()
    g = torch.Generator(device='cuda').manual_seed(1)
    for i0 in range(0, P, 16):
        idx = list(range(i0, i0 + 16))
        eng.prefill_batch(kv, idx, [(torch.randn(S, 4096, device='cuda', generator=g) * 0.02).bfloat16() for _ in idx], penalty=1.5)
    res['step'] = {'prompt_tokens': S, 'steps_per_sample': steps, 'rows': {}}
    for n in (1, 13, 64):
        ms = {md: [] for md in MODES}
        for _ in range(rounds):
            for md, (T, k, p) in MODES.items():
                for s_ in range(n):
                    kv.set_sampling(s_, T, k, p, 1000 + s_)
                for _ in range(warm):
                    eng.decode(kv, list(range(n)), penalty=1.5)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    eng.decode(kv, list(range(n)), penalty=1.5)
                b.record()
                b.synchronize()
                ms[md].append(a.elapsed_time(b) / steps)
        r = {md: round(min(v), 3) for md, v in ms.items()}
        r.update({f'{md}_vs_greedy': round(r[md] / r['greedy'], 4) for md in MODES if md != 'greedy'})
        res['step']['rows'][n] = r
        print(f'step rows {n}: {r}', flush=True)
    kv.free()
    m.close()


def main(out=None, reps=50, kernel_only=False):
    eng = Engine(ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1))
    g = torch.Generator().manual_seed(0)
    res = {'vocab': V, 'reps': reps, 'kernel_us': {}}
    for n in (1, 13, 64):
        lg = (torch.randn(n, V, generator=g) * 2.5).cuda()
        hist = torch.randint(0, V, (n, 256), generator=g).cuda()
        hl = torch.full((n,), 256, dtype=torch.int32, device='cuda')
        ids = torch.empty(n, dtype=torch.int64, device='cuda')
        kept = torch.empty(n, dtype=torch.int32, device='cuda')
        seed = torch.arange(n, dtype=torch.int64, device='cuda')
        step = torch.zeros(n, dtype=torch.int32, device='cuda')
        par = {m: (torch.full((n,), T, device='cuda'), torch.full((n,), k, dtype=torch.int32, device='cuda'), torch.full((n,), p, device='cuda'))
               for m, (T, k, p) in MODES.items()}
        ms = {m: [] for m in MODES}
        copy = []
        for it in range(reps + 5):
            for m in MODES:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t_, k_, p_ = par[m]
                B.check(B.lib.cr_op_sample(eng._h, _p(lg), n, V, _p(hist), 256, _p(hl), 1.5, _p(t_), _p(k_), _p(p_), _p(seed), _p(step), _p(ids),
                                           _p(kept), _stream()), 'cr_op_sample')
                b.record()
                b.synchronize()
                if it >= 5:
                    ms[m].append(a.elapsed_time(b))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            scratch = torch.empty_like(lg)
            a.record()
            scratch.copy_(lg)
            b.record()
            b.synchronize()
            if it >= 5:
                copy.append(a.elapsed_time(b))
        med = lambda v: sorted(v)[len(v) // 2]
        res['kernel_us'][n] = {m: round(1e3 * med(v), 1) for m, v in ms.items()}
        res['kernel_us'][n]['logits_copy_us'] = round(1e3 * med(copy), 1)
    eng.close()
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

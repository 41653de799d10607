"""Cost of constrained greedy decoding against unconstrained, two ways, for 1, 13 and 64 rows:

  kernel: one cr_op_constrain call's kernel (the kernel the decode step launches) at vocab 92 553 with a 256-id history.  The call also uploads its
          tables and synchronises, so it is not timed here: take the kernel's dispatch time from `rocprofv3 --kernel-trace --stats` over this part.
  step:   whole decode steps (cr_llm_decode) at full InternVL2-8B dims (random weights, 512-token prompts), penalty 1.5: unconstrained (pick_kernel alone)
          and constrained with no_repeat_ngram_size = 3 plus a 4000-id whitelist (the widest static mask), set per sequence with cr_kv_set_constraints.

Modes alternate within one process and are timed with device events after warm-up.  `python scripts/constrain_step.py OUT.json [--kernel-only |
--unconstrained-only]` (--kernel-only: the launches alone; --unconstrained-only: decode steps of the reduced model without any constraint -- under
rocprofv3 --kernel-trace --stats the first shows constrain_kernel's dispatches, the second that an unconstrained run has none)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from callireader_amd import constraints as K
from callireader_amd.config import ModelDims
from callireader_amd.engine import op_constrain

V = 92553


def wide(vocab=V, eos=None):
    g = torch.Generator().manual_seed(7)
    white = tuple(sorted(set(torch.randperm(vocab, generator=g)[:4000].tolist())))
    return K.Constraints(no_repeat_ngram_size=3, allowed_token_ids=white, eos_token_id=eos)


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
    c = wide()
    res['step'] = {'prompt_tokens': S, 'steps_per_sample': steps, 'rows': {}}
    for n in (1, 13, 64):
        ms = {'unconstrained': [], 'constrained': []}
        for _ in range(rounds):
            for md in ms:
                for s_ in range(n):
                    kv.set_constraints(s_, c if md == 'constrained' else None)
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
        r['constrained_vs_unconstrained'] = round(r['constrained'] / r['unconstrained'], 4)
        res['step']['rows'][n] = r
        print(f'step rows {n}: {r}', flush=True)
    kv.free()
    m.close()


def kernel_launches(reps=20):
    g = torch.Generator().manual_seed(0)
    c = wide()
    for n in (1, 13, 64):
        lg = (torch.randn(n, V, generator=g) * 2.5).cuda()
        hist = torch.randint(0, 50, (n, 256), generator=g)
        for _ in range(reps):
            op_constrain(lg.clone(), c, history=hist)


def unconstrained_steps(steps=32):
    from callireader_amd import synthetic
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=9000)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=3), dims, max_tokens=512, max_pages=16)
    pages = [m.engine.embed_splice(torch.randint(0, 9000, (40,))) for _ in range(13)]
    m.generate_pages(pages, max_new_tokens=steps, eos_token_id=None, repetition_penalty=1.5)
    m.close()


def main(out=None, mode=''):
    res = {'vocab': V, 'constraints': 'no_repeat_ngram_size=3 + 4000-id whitelist'}
    if mode == '--unconstrained-only':
        unconstrained_steps()
        return
    kernel_launches()
    if mode != '--kernel-only':
        step_times(res)
    txt = json.dumps(res, indent=1)
    if out:
        with open(out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    flags = [a for a in sys.argv[1:] if a.startswith('--')]
    main(args[0] if args else None, flags[0] if flags else '')

"""Steps and time of draft-verified decoding for ONE page at full dimensions on random weights: profiles/draft/steps.json.

Three loops over the same prompt and the same 128 ids:
  plain       generation.decode_rows (cr_llm_decode, one id per step);
  exact       generation.decode_rows_drafted with the plain run's own ids as the draft -- the ceiling: about 128 / 8 steps;
  all_wrong   cr_llm_decode_draft with seven wrong ids in EVERY step (the cursor of the host loop would stop offering after the first miss, so this loop
              calls the engine itself) -- the floor: one id per step, so the difference to `plain` per step is what the synchronisation and the seven
              rejected rows cost.
Each loop is run `--repeats` times after a warm-up run; the JSON holds every run's seconds, their median and the spread (max - min) / median, so a
difference is read against the run-to-run spread.  The acceptance rate of draft='align' needs a real checkpoint (random weights transcribe nothing):
    python inference.py --tgt <image> --model <checkpoint dir> --draft
prints the steps and the accepted ids of a page.

    python scripts/measure_draft.py [--new_tokens 128] [--prompt 3158] [--repeats 5] [--out profiles/draft/steps.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--new_tokens', type=int, default=128)
    ap.add_argument('--prompt', type=int, default=3158, help='prompt rows (the example page has 3158)')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--penalty', type=float, default=1.5)
    ap.add_argument('--layers', type=int, default=None, help='LLM layers (default: the full 32; fewer for a dry run)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'draft', 'steps.json'))
    a = ap.parse_args()
    from callireader_amd.config import ModelDims
    from callireader_amd.generation import decode_rows, decode_rows_drafted
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.full() if a.layers is None else ModelDims.reduced(llm_layers=a.layers)
    m = InternVLChatModel.from_synthetic(dims, seed=0, parts=('llm',), max_tokens=a.prompt + a.new_tokens + 128, max_pages=1)
    eng, T, V = m.engine, a.new_tokens, dims.vocab
    g = torch.Generator().manual_seed(1)
    embeds = (torch.randn(a.prompt, dims.llm_hidden, generator=g) * 0.02).to(torch.bfloat16).cuda()
    kv = m.kv(1)

    def run(draft):
        kv.reset()
        eng.prefill(kv, 0, embeds, penalty=a.penalty)
        torch.cuda.synchronize()
        stats = {}
        t0 = time.perf_counter()
        if draft is None:
            ids = decode_rows(eng, kv, [0], T, None, a.penalty)[0]
            stats = dict(steps=T - 1, drafted=0, accepted=0)
        elif draft == 'all_wrong':
            n, stats = 1, dict(steps=0, drafted=0, accepted=0)
            while n < T:
                w = [(t + 1) % V for t in truth[n:n + min(7, T - n - 1)]]
                app = eng.decode_draft(kv, [0], [w], penalty=a.penalty)[0]
                n, stats = n + app, dict(steps=stats['steps'] + 1, drafted=stats['drafted'] + len(w), accepted=stats['accepted'] + app - 1)
            ids = kv.generated(0)
        else:
            ids = decode_rows_drafted(eng, kv, [0], T, None, a.penalty, [draft], stats=stats)[0]
        torch.cuda.synchronize()
        return ids, time.perf_counter() - t0, stats

    truth = None
    ids, _, _ = run(None)                                     # warm-up: workspace, attributes, clocks
    truth = ids
    drafts = dict(plain=None, exact=ids, all_wrong='all_wrong')
    out = dict(new_tokens=T, prompt_rows=a.prompt, penalty=a.penalty, llm_layers=dims.llm_layers, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    for name, d in drafts.items():
        run(d)
        secs, st = [], None
        for _ in range(a.repeats):
            got, s, st = run(d)
            assert got == ids, f'{name}: the ids differ from the plain loop'
            secs.append(s)
        med = statistics.median(secs)
        out[name] = dict(steps=st['steps'], drafted=st['drafted'], accepted=st['accepted'], seconds=[round(s, 5) for s in secs], median_s=round(med, 5),
                         spread=round((max(secs) - min(secs)) / med, 4), ms_per_step=round(1e3 * med / st['steps'], 4))
    out['all_wrong_overhead_ms_per_step'] = round(out['all_wrong']['ms_per_step'] - out['plain']['ms_per_step'], 4)
    out['exact_speedup'] = round(out['plain']['median_s'] / out['exact']['median_s'], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    m.engine.close()


if __name__ == '__main__':
    main()

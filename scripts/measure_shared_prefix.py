#!/usr/bin/env python3
"""What sharing a page's cached prompt between its beams or samples buys in decode, measured in one process against the unshared path of the
same run: the 64-row decode step with cr_kv_set_prefix_sharing off and on at 8 pages x 8 samples, 16 x 4 and 32 x 2, the same for 8 pages x 8 beams, the
attention launch alone through cr_op_decode_attention / cr_op_decode_attention_shared, and the fan-out alone (cr_kv_fanout to 7 siblings).

Full InternVL2-8B dims, seeded random weights, a prompt of the example page's shape (3 164 rows of the embedding table: only the shape matters to a decode
step), device events, the median of three passes after a warm-up.  The sampled configurations are built with cr_kv_fork / cr_kv_fork_shared from one
prefill and fed forced ids (a step's cost does not depend on how its rows pick).  Writes profiles/shared_prefix/step.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT, STEPS, REPEATS, T = 3164, 4, 3, 3328


def device_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, per=1):
    fn()                                                    # warm-up
    return round(statistics.median(device_ms(fn) for _ in range(REPEATS)) / per, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shared_prefix', 'step.json'))
    args = ap.parse_args()
    import torch
    from callireader_amd import engine as E
    from callireader_amd.config import ModelDims
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, max_tokens=T, max_pages=64)
    eng, kv = m.engine, m.kv(64)
    g = torch.Generator().manual_seed(1)
    embeds = eng.embed_splice(torch.randint(0, m.dims.vocab, (PROMPT,), generator=g))
    rec = dict(prompt_rows=PROMPT, steps_per_pass=STEPS, repeats=REPEATS, sampled={}, beams={}, attention_alone={}, fanout_alone={})
    force = torch.arange(64, dtype=torch.long) + 100

    # ---- the 64-row decode step, P pages x n samples
    for P, n in ((8, 8), (16, 4), (32, 2)):
        ms = {}
        for share in (False, True):
            kv.reset()
            kv.set_prefix_sharing(share)
            eng.prefill(kv, 0, embeds, penalty=1.5)
            firsts = [i * n for i in range(P)]
            kv.fork(0, firsts[1:], PROMPT)                   # every page's first sequence holds the prompt itself
            for f in firsts:
                (kv.fork_shared if share else kv.fork)(f, list(range(f + 1, f + n)), PROMPT)
            ms[share] = median_ms(lambda: [eng.decode(kv, list(range(64)), penalty=1.5, force_tokens=force) for _ in range(STEPS)], STEPS)
        rec['sampled'][f'{P}x{n}'] = dict(step_ms_unshared=ms[False], step_ms_shared=ms[True], ratio=round(ms[True] / ms[False], 4))

    # ---- 8 pages x 8 beams
    ms = {}
    for share in (False, True):
        kv.reset()
        kv.set_prefix_sharing(share)
        for i in range(8):
            kv.set_beam(i * 8, 8, 1.0, False, None, 64)
        eng.prefill_batch(kv, [i * 8 for i in range(8)], [embeds] * 8, penalty=1.5)
        ms[share] = median_ms(lambda: [eng.decode(kv, list(range(64)), penalty=1.5) for _ in range(STEPS)], STEPS)
    rec['beams']['8x8'] = dict(step_ms_unshared=ms[False], step_ms_shared=ms[True], ratio=round(ms[True] / ms[False], 4))

    # ---- the fan-out alone: one prefilled, sampling source to 7 siblings
    for share in (False, True):
        kv.reset()
        kv.set_prefix_sharing(share)
        kv.set_sampling(0, 1.0, 50, 1.0, 1)
        row = eng.prefill(kv, 0, embeds, penalty=1.5, want_logits=True)
        one = lambda: kv.fanout(0, list(range(1, 8)), list(range(2, 9)), row)
        one()
        for d in range(1, 8):
            kv.reset(d)
        times = []
        for _ in range(REPEATS):
            times.append(device_ms(one))
            for d in range(1, 8):
                kv.reset(d)
        rec['fanout_alone']['shared' if share else 'unshared'] = round(statistics.median(times), 4)
    kv.reset()
    kv.set_prefix_sharing(False)

    # ---- the attention launch alone (one layer's), 64 rows at PROMPT + 36 keys
    dev = torch.device('cuda', 0)
    kc = torch.randn((64, 8, T, 128), generator=g).to(torch.bfloat16).to(dev)
    vc = torch.randn((64, 8, T, 128), generator=g).to(torch.bfloat16).to(dev)
    q = torch.randn((64, 4096), generator=g).to(torch.bfloat16).to(dev)
    seqs = torch.arange(64, dtype=torch.int32, device=dev)
    keys = PROMPT + 36
    lens = torch.full((64,), keys - 1, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(E.B.lib.cr_op_decode_attention_scratch_floats(64, keys)), device=dev, dtype=torch.float32)
    out = torch.empty(64, 4096, device=dev, dtype=torch.bfloat16)
    plain = median_ms(lambda: [E.op_decode_attention(q, kc, vc, seqs, lens, max_keys=keys, scratch=scratch, out=out) for _ in range(20)], 20)
    rec['attention_alone']['unshared_ms'] = plain
    for P, n in ((8, 8), (16, 4), (32, 2)):
        src = [b - b % n if b % n else -1 for b in range(64)]
        plen = [PROMPT & ~255 if b % n else 0 for b in range(64)]
        # (the entry synchronises and stages its table per call: host time a decode step does not pay, but the events bracket it; 20 launches per pass)
        sh = median_ms(lambda: [E.op_decode_attention_shared(q, kc, vc, seqs, lens, src, plen, max_keys=keys, scratch=scratch, out=out) for _ in range(20)], 20)
        rec['attention_alone'][f'{P}x{n}_shared_ms'] = sh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()

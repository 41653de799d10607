#!/usr/bin/env python3
"""Continuous batching against the batch-granular pipeline, on the same pages (one MI355X).

  python scripts/continuous_bench.py [--pages 256] [--slots 64] [--seed 0] [--out FILE]

Model: seeded random weights of the full InternLM2.5-7B language model (InternVLChatModel.from_synthetic, parts=('llm',)).
Pages: `--pages` prompts of the examples/0.jpg shape (11 page tiles x 256 + 96 characters x 3 pseudo-tokens + 60 text = 3164 tokens), as
random bf16 prompt embeddings: the visual stage is the same work for both paths and is left out; prefill and decode are measured.
Paths, each driven from this thread with its decode on a worker thread and a second stream:
  batch       PagePipeline, 64 pages per batch (two batches in flight: batch i decodes while batch i+1 is prefilled), EOS checks every 16 steps;
  continuous  ContinuousPipeline, `--slots` decode rows (+ as many spare KV sequences), prefill groups of 16.
Workloads: random weights do not emit EOS, so seeded per-page budgets of new tokens stand in for it:
  ragged      97 % of the pages uniform in 20 .. 250 tokens, 3 % run to max_new_tokens = 1024 (a page caught in a repetition loop);
  equal       every page 128 tokens (bench.py's workload).
Both paths carry the real EOS id (92542) as well.  Reported per path and workload: pages/s (wall time from the first prefill to the last page's
ids on the host), decode steps, mean live rows per step, speculative row-steps (rows decoded past their stop), and whether every page's
ids equal between the two paths.  One JSON document on stdout (and in --out).
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchlib.plan import PAGE_TILES, CHAR_TILES, TEXT_TOKENS  # noqa: E402
from callireader_amd.config import ModelDims, EOS_TOKEN_ID  # noqa: E402

MAX_NEW = 1024


def budgets_for(workload, n, seed):
    rng = random.Random(seed)
    if workload == 'equal':
        return [128] * n
    return [MAX_NEW if rng.random() < 0.03 else rng.randint(20, 250) for _ in range(n)]


def run_batch(model, embeds, budgets, batch=64):
    pipe = model.page_pipeline(max_new_tokens=MAX_NEW, eos_token_id=EOS_TOKEN_ID)
    pipe._kv(0, batch)
    pipe._kv(1, batch)                              # both caches allocated before the clock starts
    torch.cuda.synchronize()
    outs = []
    t0 = time.perf_counter()
    for i in range(0, len(embeds), batch):
        prev = pipe.start(embeds[i:i + batch], budgets=budgets[i:i + batch])
        if prev is not None:
            outs += prev
    outs += pipe.finish()
    wall = time.perf_counter() - t0
    steps, row_steps = pipe.host_steps, pipe.row_steps
    pipe.close()
    useful = sum(len(o) - 1 for o in outs)
    return outs, dict(pages_per_s=round(len(embeds) / wall, 3), wall_s=round(wall, 3), decode_steps=steps,
                      mean_live_rows=round(row_steps / max(1, steps), 2), row_steps=row_steps, speculative_row_steps=row_steps - useful)


def run_continuous(model, embeds, budgets, slots):
    from callireader_amd.continuous import ContinuousPipeline
    pipe = ContinuousPipeline(model, slots=slots, max_new_tokens=MAX_NEW, eos_token_id=EOS_TOKEN_ID, admit_group=16)
    torch.cuda.synchronize()
    got = {}
    t0 = time.perf_counter()
    tickets = [pipe.submit(e, max_new_tokens=b) for e, b in zip(embeds, budgets)]
    got.update(pipe.ready())
    got.update(pipe.results())
    wall = time.perf_counter() - t0
    st = dict(pipe.stats)
    pipe.close()
    outs = [got[t] for t in tickets]
    return outs, dict(pages_per_s=round(len(embeds) / wall, 3), wall_s=round(wall, 3), decode_steps=st['decode_steps'],
                      mean_live_rows=round(st['row_steps'] / max(1, st['decode_steps']), 2), row_steps=st['row_steps'],
                      speculative_row_steps=st['speculative_row_steps'], admissions=st['admissions'],
                      decode_host_s=round(st['decode_host_s'], 3), caller_host_s=round(st['caller_host_s'], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pages', type=int, default=256)
    ap.add_argument('--slots', type=int, default=64)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--fp8_kv', action='store_true', help='e4m3 KV caches (kv_cache_dtype="e4m3") for both paths')
    ap.add_argument('--workload', choices=('ragged', 'equal', 'both'), default='both')
    args = ap.parse_args()
    from callireader_amd import build, _binding as B
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    S = PAGE_TILES * 256 + CHAR_TILES * 3 + TEXT_TOKENS
    model = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, parts=('llm',), max_tokens=S + MAX_NEW + 64, max_pages=64,
                                             kv_cache_dtype='e4m3' if args.fp8_kv else 'bf16')
    g = torch.Generator(device=model.device).manual_seed(args.seed)
    embeds = [(torch.randn(S, 4096, generator=g, device=model.device) * 0.02).to(torch.bfloat16) for _ in range(args.pages)]
    # warm-up: both paths once on a few pages (workspaces grow to their steady size, kernels load)
    wb = [40, 9, 25, 70] * 4
    run_batch(model, embeds[:16], wb)
    run_continuous(model, embeds[:16], wb, args.slots)
    res = {}
    for workload in (('ragged', 'equal') if args.workload == 'both' else (args.workload,)):
        budgets = budgets_for(workload, args.pages, args.seed)
        ob, rb = run_batch(model, embeds, budgets)
        oc, rc = run_continuous(model, embeds, budgets, args.slots)
        res[workload] = dict(budgets=dict(mean=round(sum(budgets) / len(budgets), 1), at_max=sum(b == MAX_NEW for b in budgets)),
                             batch=rb, continuous=rc, continuous_over_batch=round(rc['pages_per_s'] / rb['pages_per_s'], 3),
                             ids_equal=ob == oc, ids_match_budgets=all(len(o) == b for o, b in zip(oc, budgets)))
        print(json.dumps({workload: res[workload]}), file=sys.stderr, flush=True)
    argv = sys.argv[1:]
    if '--out' in argv:                                   # the run's arguments, not where its report was saved
        i = argv.index('--out')
        argv = argv[:i] + argv[i + 2:]
    doc = dict(what='continuous batching (ContinuousPipeline) vs batch-granular (PagePipeline) on the same pages; see scripts/continuous_bench.py',
               cmd=' '.join(['python scripts/continuous_bench.py'] + argv), build_id=B.lib.cr_build_id().decode(),
               sources=build.source_hash(), device=torch.cuda.get_device_name(0), pages=args.pages, slots=args.slots, prompt_tokens=S, kv_cache_dtype=model.kv_cache_dtype,
               max_new_tokens=MAX_NEW, results=res)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(txt + '\n')
    model.close()


if __name__ == '__main__':
    main()

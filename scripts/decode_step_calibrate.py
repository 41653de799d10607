#!/usr/bin/env python3
"""CPU only: the figures behind ORACLE_K_STEPS / ORACLE_V_STEPS of tests/test_gpu_decode_step.py.  For the (token, position) pairs its 13- and 64-row
batches feed, the oracle's bf16 layer-0 K / V rows (oracle/internlm2.py) against the float64 closed form (kv_rows_f64), in bf16 steps of the element."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_decode_step as T  # noqa: E402
from callireader_amd.config import ModelDims  # noqa: E402
from callireader_amd import synthetic  # noqa: E402
from callireader_amd.engine import rope_tables  # noqa: E402
from oracle import generate  # noqa: E402

dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=8201)
sd = synthetic.make_state_dict(dims, parts=('llm',), seed=0)
cos, sin = rope_tables(dims, 2048)
ids = {}
with torch.no_grad():
    for S in T.ORACLE_ROWS:
        ids[S] = generate.greedy_generate(sd, 2, T.prompt(S), max_new_tokens=T.STEPS + 1, eos_token_id=-1, repetition_penalty=T.PENALTY)[0].tolist()
        print('oracle ids of the row of', S, 'tokens:', ids[S], flush=True)
worst = [0.0, 0.0]
for rows in (13, 64):
    lens = T.BATCHES[rows]
    tokens = T.forced_tokens(lens, ids).T.reshape(-1)
    positions = torch.tensor([S + t for S in lens for t in range(T.STEPS)])
    dev = T.bf16_steps(T.kv_rows_oracle(sd, tokens, positions), T.kv_rows_f64(sd, cos, sin, tokens, positions))
    for w in (0, 1):
        d = dev[:, w]
        worst[w] = max(worst[w], float(d.max()))
        print(f'{rows} rows, {"KV"[w]}: worst {float(d.max()):.4f} bf16 steps; elements off by > 0: {int((d > 0).sum())}, > 1: {int((d > 1).sum())}, '
              f'> 2: {int((d > 2).sum())} of {d.numel()}', flush=True)
print(f'ORACLE_K_STEPS = {worst[0]:.4f}   ORACLE_V_STEPS = {worst[1]:.4f}')

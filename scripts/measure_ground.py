#!/usr/bin/env python3
"""What grounding costs, measured: cr_llm_ground_batch over all layers and over 8 layers against cr_llm_score_batch on the same rows -- the pass that
grounding rides on, and the yardstick.

Model: seeded random weights at full InternVL2-8B dims (InternVLChatModel.from_synthetic, language model only).  One page-shaped prompt of PROMPT rows is
prefilled once; BOXES character boxes of three pseudo-token rows each sit in it as one run of spans (about a fifth of the keys, as on the example page).
Every measurement forks the prefix (cr_kv_fork, outside the timing) and scores / grounds an answer of 32 / 256 ids behind it.  The three calls alternate in
one process, device events around each, best of REPEATS.

--kernels: one more run of its own, under `rocprofv3 --kernel-trace`, of a single 256-id grounding call over all layers; the two span-mass kernels' times are
read from its trace.  Writes profiles/ground/ground.json (--out).  A step that fails ends the run; the record says which."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT, ANSWERS, REPEATS, PENALTY, TOP_N = 3164, (32, 256), 3, 1.5, 1
BOXES, FIRST_BOX = 220, 2450
SOME_LAYERS = (12, 20)
KERNELS = ('span_mass_kernel', 'span_mass_add_kernel')


def spans():
    return [(FIRST_BOX + 3 * i, FIRST_BOX + 3 * i + 3) for i in range(BOXES)]


def setup():
    import torch
    from callireader_amd.config import ModelDims
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, parts=('llm',), max_tokens=PROMPT + max(ANSWERS) + 64, max_pages=2)
    g = torch.Generator().manual_seed(1)
    prompt = (torch.randn(PROMPT, m.dims.llm_hidden, generator=g) * 0.02).to(torch.bfloat16).cuda()
    kv = m.kv(2)
    kv.reset()
    m.engine.prefill(kv, 0, prompt)
    return m, kv, prompt


def answer(T, vocab, seed=2):
    import torch
    g = torch.Generator().manual_seed(seed)
    pool = torch.randperm(vocab, generator=g)[:T // 2 + 1]
    return pool[torch.randint(0, len(pool), (T,), generator=g)].tolist()


def events(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def rows_of(m, prompt, y):
    import torch
    return torch.cat([prompt[PROMPT - 1:], m.engine.embed_splice(torch.tensor(y[:-1], dtype=torch.long))], dim=0) if len(y) > 1 else prompt[PROMPT - 1:]


def score_once(m, kv, prompt, y):
    kv.fork(0, [1], PROMPT - 1)
    rows = rows_of(m, prompt, y)
    (ts,), ms = events(lambda: m.engine.score_batch(kv, [1], [rows], [list(y)], penalty=PENALTY, top_n=TOP_N))
    return ts.logprobs, ms


def ground_once(m, kv, prompt, y, layers):
    kv.fork(0, [1], PROMPT - 1)
    rows = rows_of(m, prompt, y)
    (tss, ms_), ms = events(lambda: m.engine.ground_batch(kv, [1], [rows], [list(y)], [spans()], layers=layers, penalty=PENALTY, top_n=TOP_N))
    return tss[0].logprobs, ms_[0], ms


def measure(out_path):
    import numpy as np
    m, kv, prompt = setup()
    rec = {'model': 'InternVL2-8B dims, seeded random weights, language model only', 'prompt_rows_cached': PROMPT, 'spans': BOXES, 'span_keys': 3 * BOXES,
           'penalty': PENALTY, 'top_n': TOP_N, 'some_layers': list(SOME_LAYERS),
           'method': f'the three calls alternating in one process, device events, best of {REPEATS}; the fork of the cached prefix is outside the timing',
           'answers': []}
    for T in ANSWERS:
        y = answer(T, m.dims.vocab)
        score_once(m, kv, prompt, y)                       # warm-up: workspace growth, first launches
        ground_once(m, kv, prompt, y, None)
        s_ms, a_ms, p_ms, same = [], [], [], True
        for _ in range(REPEATS):
            lp, ms = score_once(m, kv, prompt, y)
            s_ms.append(ms)
            lp_all, mass, ms = ground_once(m, kv, prompt, y, None)
            a_ms.append(ms)
            lp_some, _, ms = ground_once(m, kv, prompt, y, SOME_LAYERS)
            p_ms.append(ms)
            same = same and bool((lp.view('int32') == lp_all.view('int32')).all()) and bool((lp.view('int32') == lp_some.view('int32')).all())
        rec['answers'].append({'ids': T, 'score_batch_ms': round(min(s_ms), 3), 'ground_all_layers_ms': round(min(a_ms), 3),
                               'ground_8_layers_ms': round(min(p_ms), 3), 'score_batch_ms_all': [round(x, 3) for x in s_ms],
                               'ground_all_layers_ms_all': [round(x, 3) for x in a_ms], 'ground_8_layers_ms_all': [round(x, 3) for x in p_ms],
                               'all_layers_over_score': round(min(a_ms) / min(s_ms), 3), '8_layers_over_score': round(min(p_ms) / min(s_ms), 3),
                               'logprobs_bit_equal_to_score_batch': same, 'mass_on_boxes_mean': round(float(np.asarray(mass).sum(-1).mean()), 4)})
        print(json.dumps(rec['answers'][-1]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(rec, f, indent=1)
    m.close()
    return rec


def traced_child():
    """under rocprofv3: one 256-id grounding call over all layers (after a warm-up call of the same shape)"""
    m, kv, prompt = setup()
    y = answer(max(ANSWERS), m.dims.vocab)
    ground_once(m, kv, prompt, y, None)
    ground_once(m, kv, prompt, y, None)
    m.close()


def kernels(out_path, limit_s):
    """run the traced child in a run of its own and add the two kernels' times (of the LAST call: per kernel, launches and summed microseconds) to the record"""
    rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
    d = tempfile.mkdtemp(prefix='cr_ground_trace_')
    cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__), '--traced-child']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit_s)
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if r.returncode != 0 or not files:
        rec['kernels'] = {'status': f'not measured: rocprofv3 exit {r.returncode}, {len(files)} trace files', 'tail': r.stdout.decode(errors='replace')[-400:]}
    else:
        rows = list(csv.DictReader(open(files[0])))
        out = {}
        for k in KERNELS:
            mine = [x for x in rows if k in x['Kernel_Name']]
            half = mine[len(mine) // 2:]                   # the second of the two calls
            out[k] = {'launches': len(half), 'total_us': round(sum(int(x['End_Timestamp']) - int(x['Start_Timestamp']) for x in half) / 1e3, 1)}
        rec['kernels'] = {'status': f'rocprofv3 --kernel-trace, a run of its own: one {max(ANSWERS)}-id call over all layers', 'per_call': out}
    with open(out_path, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec['kernels']), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ground', 'ground.json'))
    ap.add_argument('--kernels', action='store_true', help='only the rocprofv3 run: adds the kernels\' times to an existing record')
    ap.add_argument('--traced-child', action='store_true')
    ap.add_argument('--limit', type=int, default=400)
    a = ap.parse_args()
    if a.traced_child:
        traced_child()
    elif a.kernels:
        kernels(a.out, a.limit)
    else:
        measure(a.out)

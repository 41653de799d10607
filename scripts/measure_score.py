#!/usr/bin/env python3
"""What scoring a given text costs, measured: cr_llm_score_batch against the only way to get the same numbers without it -- one
cr_llm_decode(force_tokens) step per id, each followed by the repetition penalty and cr_op_logprobs.

Model: seeded random weights at full InternVL2-8B dims (InternVLChatModel.from_synthetic, language model only).  One page-shaped prompt of PROMPT rows is
prefilled once; every measurement forks its prefix (cr_kv_fork, outside the timing) and scores an answer of 32 / 256 / 1024 ids behind it.  Both paths
alternate in one process, device events around each, best of REPEATS; the two paths' log-probabilities are compared as a sanity check (two bf16 kernel paths:
they agree to the noise floor, not bit for bit).

--kernels: one more run of its own, under `rocprofv3 --kernel-trace`, of a single 1024-id scoring call; the three score kernels' times are read from its
trace.  Writes profiles/score/score.json (--out).  A step that fails ends the run; the record says which."""
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

PROMPT, ANSWERS, REPEATS, PENALTY, TOP_N = 3164, (32, 256, 1024), 3, 1.5, 1
KERNELS = ('score_table_kernel', 'score_chunk_kernel', 'score_merge_kernel')


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


def score_once(m, kv, prompt, y):
    import torch
    kv.fork(0, [1], PROMPT - 1)
    rows = torch.cat([prompt[PROMPT - 1:], m.engine.embed_splice(torch.tensor(y[:-1], dtype=torch.long))], dim=0) if len(y) > 1 else prompt[PROMPT - 1:]
    (ts,), ms = events(lambda: m.engine.score_batch(kv, [1], [rows], [list(y)], penalty=PENALTY, top_n=TOP_N))
    return ts.logprobs, ms


def loop_once(m, kv, prompt, y):
    """the parent commit's way: the prompt's last row as a one-row prefill, then one forced decode step per id; every step's raw row is penalised over the
    ids before it (device index ops) and scored by cr_op_logprobs"""
    import torch
    from callireader_amd.engine import op_logprobs
    eng = m.engine
    kv.fork(0, [1], PROMPT - 1)
    dev = prompt.device
    yt = torch.tensor(y, dtype=torch.long, device=dev)

    def run():
        out = []
        lg = eng.prefill(kv, 1, prompt[PROMPT - 1:], penalty=1.0, want_logits=True).reshape(1, -1)
        for j in range(len(y)):
            if j:
                lg = eng.decode(kv, [1], penalty=1.0, force_tokens=yt[j - 1:j], want_logits=True)
                hist = torch.unique(yt[:j])
                s = lg[0, hist]
                lg[0, hist] = torch.where(s < 0, s * PENALTY, s / PENALTY)
            out.append(op_logprobs(lg, yt[j:j + 1], TOP_N)[0])
        return torch.cat(out).cpu().numpy()
    return events(run)


def measure(out_path):
    import numpy as np
    m, kv, prompt = setup()
    rec = {'model': 'InternVL2-8B dims, seeded random weights, language model only', 'prompt_rows_cached': PROMPT, 'penalty': PENALTY, 'top_n': TOP_N,
           'method': f'both paths alternating in one process, device events, best of {REPEATS}; the fork of the cached prefix is outside the timing',
           'answers': []}
    for T in ANSWERS:
        y = answer(T, m.dims.vocab)
        score_once(m, kv, prompt, y)                       # warm-up: workspace growth, first launches
        s_ms, l_ms, diff = [], [], 0.0
        for _ in range(REPEATS):
            a, ms = score_once(m, kv, prompt, y)
            s_ms.append(ms)
            b, ms = loop_once(m, kv, prompt, y)
            l_ms.append(ms)
            diff = max(diff, float(np.abs(a - b).max()))
        rec['answers'].append({'ids': T, 'score_batch_ms': round(min(s_ms), 3), 'decode_loop_ms': round(min(l_ms), 3),
                               'score_batch_ms_all': [round(x, 3) for x in s_ms], 'decode_loop_ms_all': [round(x, 3) for x in l_ms],
                               'speedup': round(min(l_ms) / min(s_ms), 2), 'max_abs_logprob_difference': round(diff, 5)})
        print(json.dumps(rec['answers'][-1]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(rec, f, indent=1)
    m.close()
    return rec


def traced_child():
    """under rocprofv3: one 1024-id scoring call (after a warm-up call of the same shape)"""
    m, kv, prompt = setup()
    y = answer(max(ANSWERS), m.dims.vocab)
    score_once(m, kv, prompt, y)
    score_once(m, kv, prompt, y)
    m.close()


def kernels(out_path, limit_s):
    """run the traced child in a run of its own and add the three kernels' times (of the LAST call: per kernel, launches and summed microseconds) to the record"""
    rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
    d = tempfile.mkdtemp(prefix='cr_score_trace_')
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
        rec['kernels'] = {'status': 'rocprofv3 --kernel-trace, a run of its own: one 1024-id call (4 head tiles of 256 rows)', 'per_call': out}
    with open(out_path, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec['kernels']), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score', 'score.json'))
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

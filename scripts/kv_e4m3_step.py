"""bf16 against e4m3 KV cache (cr_kv_alloc_ex CR_KV_E4M3) at full InternVL2-8B dims, random weights, ~3 164-token prompts:

  attention: the decode attention of one layer alone (cr_op_decode_attention / cr_op_decode_attention_e4m3, split kernel + combine) at 64 rows;
  step:      whole decode steps (cr_llm_decode) at 1, 8 and 64 rows, bf16 weights and e4m3 weights (cr_enable_fp8_decode), the two caches alternating;
  prefill:   16 pages of the prompt length into each cache (the e4m3 cache's prefill adds the bf16 staging and the quantised cache rows).

Modes alternate within one process and are timed with device events after warm-up.  `python scripts/kv_e4m3_step.py OUT.json [--kernels-only]`
(--kernels-only: the 64-row attention launches of both formats alone, for rocprofv3 --kernel-trace --stats)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from callireader_amd.config import ModelDims
from callireader_amd import build, _binding as B
from callireader_amd.engine import op_decode_attention, op_decode_attention_e4m3

S, P = 3164, 64


def ev_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def attention_times(res, reps=50, kernels_only=False):
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    T = S + 64
    lens = torch.full((P,), S - 1, dtype=torch.int32, device=dev)
    seqs = torch.arange(P, dtype=torch.int32, device=dev)
    q = (torch.randn(P, 4096, device=dev, generator=g) * 0.3).bfloat16()
    kb = (torch.randn(P, 8, T, 128, device=dev, generator=g)).bfloat16()
    vb = (torch.randn(P, 8, T, 128, device=dev, generator=g)).bfloat16()
    k8 = torch.randint(0, 0x7e, (P, 8, T, 128), device=dev, generator=g, dtype=torch.uint8)
    v8 = torch.randint(0, 0x7e, (P, 8, T, 128), device=dev, generator=g, dtype=torch.uint8)
    ks = torch.rand(P, 8, T, device=dev, generator=g) + 0.5
    vs = torch.rand(P, 8, T, device=dev, generator=g) + 0.5
    scratch = torch.empty(int(B.lib.cr_op_decode_attention_scratch_floats(P, S)), device=dev)
    out = torch.empty(P, 4096, device=dev, dtype=torch.bfloat16)
    fb = lambda: op_decode_attention(q, kb, vb, seqs, lens, max_keys=S, scratch=scratch, out=out)                   # noqa: E731
    f8 = lambda: op_decode_attention_e4m3(q, k8, v8, ks, vs, seqs, lens, max_keys=S, scratch=scratch, out=out)      # noqa: E731
    for f in (fb, f8):
        ev_ms(f, 5)
    if kernels_only:
        for _ in range(reps):
            fb(); f8()
        torch.cuda.synchronize()
        return
    ms = {'bf16': [], 'e4m3': []}
    for _ in range(3):
        ms['bf16'].append(ev_ms(fb, reps))
        ms['e4m3'].append(ev_ms(f8, reps))
    bytes_b = P * 8 * S * 128 * 2 * 2
    bytes_8 = P * 8 * S * (128 + 4) * 2
    res['attention'] = {'rows': P, 'keys': S, 'us': {k: round(min(v) * 1e3, 1) for k, v in ms.items()},
                        'MB': {'bf16': round(bytes_b / 1e6, 1), 'e4m3': round(bytes_8 / 1e6, 1)},
                        'TB_per_s': {'bf16': round(bytes_b / min(ms['bf16']) / 1e9, 2), 'e4m3': round(bytes_8 / min(ms['e4m3']) / 1e9, 2)}}
    print(json.dumps({'attention': res['attention']}), file=sys.stderr, flush=True)
    del kb, vb, k8, v8


def model_times(res):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    T = S + 256
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, parts=('llm',), max_tokens=T, max_pages=P)
    eng = m.engine
    kvs = {'bf16': eng.kv_alloc(P, T), 'e4m3': eng.kv_alloc(P, T, dtype='e4m3')}
    g = torch.Generator(device='cuda').manual_seed(1)
    pages = [(torch.randn(S, 4096, device='cuda', generator=g) * 0.02).bfloat16() for _ in range(16)]
    pre = {k: [] for k in kvs}
    for i0 in range(0, P, 16):                                # alternate the formats group by group; the first group of each grows the workspace
        for k, kv in kvs.items():
            idx = list(range(i0, i0 + 16))
            pre[k].append(ev_ms(lambda: eng.prefill_batch(kv, idx, pages, penalty=1.0), 1))
    res['prefill_16_pages_ms'] = {k: round(sorted(v[1:])[len(v[1:]) // 2], 1) for k, v in pre.items()}
    res['prefill_16_pages_ms_all'] = {k: [round(x, 1) for x in v] for k, v in pre.items()}
    print(json.dumps({'prefill': res['prefill_16_pages_ms']}), file=sys.stderr, flush=True)
    res['step_ms'] = {}
    steps, warm, rounds = 8, 2, 2
    for fp8 in (False, True):
        eng.enable_fp8_decode(fp8)
        wk = 'e4m3_weights' if fp8 else 'bf16_weights'
        res['step_ms'][wk] = {}
        for n in (1, 8, 64):
            seqs = list(range(n))
            ms = {k: [] for k in kvs}
            for _ in range(rounds):
                for k, kv in kvs.items():
                    ev_ms(lambda: eng.decode(kv, seqs), warm)
                    ms[k].append(ev_ms(lambda: eng.decode(kv, seqs), steps))
            res['step_ms'][wk][n] = {k: round(min(v), 3) for k, v in ms.items()}
            print(json.dumps({wk: {n: res['step_ms'][wk][n]}}), file=sys.stderr, flush=True)
    eng.enable_fp8_decode(False)
    res['cache_len_after'] = kvs['bf16'].length(0)
    for kv in kvs.values():
        kv.free()
    m.close()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('--') else None
    kernels_only = '--kernels-only' in sys.argv
    res = dict(what='bf16 vs e4m3 KV cache; see scripts/kv_e4m3_step.py', build_id=B.lib.cr_build_id().decode(), sources=build.source_hash(),
               device=torch.cuda.get_device_name(0), prompt_tokens=S, cache_bytes_per_token={'bf16': 32 * 8 * 128 * 2 * 2, 'e4m3': 32 * 8 * (128 + 4) * 2})
    attention_times(res, kernels_only=kernels_only)
    if kernels_only:
        return
    model_times(res)
    txt = json.dumps(res, indent=1)
    print(txt)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""fp8 accuracy instrument (round-4 verdict, item 4): full depth, against the reference's own vectors, on checkpoints WITH outlier channels.

tests/golden/full_depth.npz holds what the reference's InternViT (24 L) + extract_feature and InternLM2 (32 L, 92 553-row vocabulary) produce on the seed-0
checkpoint.  `synthetic.outlier_transform` re-scales matched norm-gain / weight-column (and w3-row / w2-column) pairs by 2^shift: the function is unchanged BIT FOR BIT
in bf16 arithmetic, so the same vectors are the golden of every variant, while every row maximum an fp8 quantiser takes is dominated by the outlier channels
(x 32 at shift 5, x 1024 at shift 10).  Three measurements, written to profiles/round5/fp8_schemes.json:
  1. HIP path (needs the GPU): bf16 (must not move by a bit across shifts), cr_enable_fp8_mfma level 1 / level 2 (e4m3 x e4m3 on the matrix cores, ONE fp32 scale
     per activation row and per weight row) -- ViT features and prefill logits, relative L2 against the reference, first greedy pick;
  2. CPU emulation of the same linears (the oracle with fake-quantised operands, fp32 accumulation): per-row fp32 scales (= what the HIP kernels do: the two must
     agree, which validates the emulation) against OCP-MX block scaling (one E8M0 scale per 32 elements along K for both operands: what
     v_mfma_scale_f32_16x16x128_f8f6f4 would multiply) -- the scheme a block-scaled gemm256 instance would have to beat per-row scaling by to be worth building;
  3. the same two schemes with e4m3 replaced by a FIXED-point 8-bit format (int8, symmetric): the control that shows the instrument does see scaling granularity
     (a format without an exponent collapses under per-row scales once the outliers are in; e4m3 carries its own 4-bit exponent per element).
Usage:  python scripts/fp8_schemes.py [--shifts 0,5,10] [--no-gpu] [--layers 32]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from callireader_amd.config import ModelDims  # noqa: E402
from callireader_amd import synthetic  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def bits_to_f32(u16):
    return torch.from_numpy((u16.astype(np.uint32) << 16).view(np.float32).copy())


def subsample(t, step, n):
    return t.reshape(-1)[::step][:n].float()


# ---- fake quantisers (value -> nearest representable value of the format under the scheme's scale) ------------------------------------------------------------
def q_e4m3(x):
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)


def q_int8(x):
    return x.round().clamp(-127.0, 127.0)


def fq_row(x, q, qmax):
    """one fp32 scale per row: max|x| / qmax (1 for an all-zero row) -- weights.hip: quant_fp8_rows_kernel, norm.hip's e4m3 rows"""
    mx = x.abs().amax(-1, keepdim=True)
    sc = torch.where(mx > 0, mx / qmax, torch.ones_like(mx))
    return q(x / sc) * sc


def fq_block32(x, q, emax):
    """OCP MX: one power-of-two (E8M0) scale per 32 elements along the last dimension, 2^(floor(log2 max|block|) - emax), elements saturate"""
    sh = x.shape
    xb = x.reshape(*sh[:-1], sh[-1] // 32, 32)
    mx = xb.abs().amax(-1, keepdim=True)
    e = torch.floor(torch.log2(torch.where(mx > 0, mx, torch.ones_like(mx)))) - emax
    sc = torch.exp2(e)
    return (q(xb / sc) * sc).reshape(sh)


SCHEMES = {
    'e4m3, fp32 scale per row (the HIP kernels)': lambda x: fq_row(x, q_e4m3, 448.0),
    'e4m3, E8M0 scale per 32 along K (OCP MX block scaling)': lambda x: fq_block32(x, q_e4m3, 8),
    'int8 control, fp32 scale per row': lambda x: fq_row(x, q_int8, 127.0),
    'int8 control, E8M0 scale per 32 along K': lambda x: fq_block32(x, q_int8, 6),
}


def emulate_prefill(sd, dims, emb, fq, level, layers):
    """oracle/internlm2.py's forward with the fp8 option's linears (level 1: wqkv, w1, w3; level 2: + wo, w2; never the LM head) taking fake-quantised operands"""
    from oracle import internlm2
    tails = ('attention.wqkv.weight', 'feed_forward.w1.weight', 'feed_forward.w3.weight') + (('attention.wo.weight', 'feed_forward.w2.weight') if level >= 2 else ())
    qset = {id(v) for k, v in sd.items() if k.endswith(tails)}

    def linear(x, w, b=None):
        if id(w) not in qset:
            return F.linear(x, w, b)
        y = fq(x.float()) @ fq(w.float()).t()
        return y.to(x.dtype)
    ns = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith('__')})
    ns.linear = linear
    old = internlm2.F
    internlm2.F = ns
    try:
        with torch.no_grad():
            lg, _ = internlm2.model_forward(sd, layers, inputs_embeds=emb, all_logits=False)
    finally:
        internlm2.F = old
    return lg.float().reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shifts', default='0,5,10')
    ap.add_argument('--no-gpu', action='store_true')
    ap.add_argument('--no-emulation', action='store_true')
    ap.add_argument('--layers', type=int, default=32, help='LLM depth of the CPU emulation (the golden only applies at 32; fewer layers compare against the bf16 oracle at that depth)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'round5', 'fp8_schemes.json'))
    args = ap.parse_args()
    shifts = [int(s) for s in args.shifts.split(',')]
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'full_depth.npz'))
    meta = json.loads(bytes(g['meta']).decode())
    dims = ModelDims.full()
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    S = meta['prompt_tokens']
    emb = (torch.randn(1, S, 4096, generator=torch.Generator().manual_seed(meta['prompt_seed'])) * 0.02).to(torch.bfloat16)
    px = synthetic.make_pixels(2, seed=meta['pixels_seed'])
    ref_logits = bits_to_f32(g['llm32.logits_bf16_bits'])[0]
    ref_feat = torch.from_numpy(g['vit24.feat.sample'])
    rep = {'what': __doc__.split('\n')[0], 'golden': 'tests/golden/full_depth.npz (the reference\'s own modules on the plain seed-0 checkpoint; bit-identical on the outlier variants by construction)',
           'outlier': dict(synthetic.OUTLIER), 'prompt_tokens': S, 'reference_bf16_vs_its_own_fp32_rel_l2': float(g['llm32.ref_bf16_vs_fp32_rel_l2'])}
    t0 = time.time()
    plain = {}
    for parts in (('vit', 'mlp1'), ('llm',)):
        for k, v in synthetic.iter_state_dict(dims, parts=parts, seed=0):
            plain[k] = v
    rep['weights_drawn_s'] = round(time.time() - t0, 1)
    print(f'[{time.time() - t0:.0f}s] weights drawn', flush=True)

    if not args.no_gpu:
        from callireader_amd.engine import Engine
        hip = {}
        base = None
        for sh in shifts:
            eng = Engine(dims, max_pos=4096)
            for k, v in plain.items():
                eng.load_weight(k, synthetic.outlier_transform(k, v, dims, sh))
            eng.load_rope()
            eng.finalize()
            row = {}
            for name, level in (('bf16', 0), ('fp8 level 1', 1), ('fp8 level 2', 2)):
                if level:
                    eng.enable_fp8_mfma(True, level=level)
                feat = eng.extract_feature(px.cuda())
                kv = eng.kv_alloc(1, 512)
                lg = eng.prefill(kv, 0, emb.cuda(), want_logits=True).float().cpu().reshape(-1)
                kv.free()
                torch.cuda.synchronize()
                if level:
                    eng.enable_fp8_mfma(False)
                row[name] = {'extract_feature_rel_l2_vs_reference': rel_l2(subsample(feat.cpu(), int(g['vit24.feat.step']), ref_feat.numel()), ref_feat),
                             'prefill_logits_rel_l2_vs_reference': rel_l2(lg, ref_logits), 'first_pick_equal': bool(int(lg.argmax()) == int(ref_logits.argmax()))}
                if name == 'bf16':
                    if base is None:
                        base = (feat.clone(), lg.clone())
                    row[name]['same_bits_as_the_plain_checkpoint'] = bool(torch.equal(feat, base[0]) and torch.equal(lg, base[1]))
            hip[f'shift {sh}'] = row
            print(f'[{time.time() - t0:.0f}s] HIP, outlier shift {sh}: ' + json.dumps(row), flush=True)
            eng.close()
        rep['hip'] = hip

    if not args.no_emulation:
        emu = {}
        for sh in shifts:
            sd = {k: synthetic.outlier_transform(k, v, dims, sh) for k, v in plain.items() if k.startswith('language_model.')}
            ref = ref_logits
            if args.layers != dims.llm_layers:
                from oracle import internlm2
                with torch.no_grad():
                    ref = internlm2.model_forward(sd, args.layers, inputs_embeds=emb, all_logits=False)[0].float().reshape(-1)
            row = {}
            for name, fq in SCHEMES.items():
                for level in (1, 2):
                    lg = emulate_prefill(sd, dims, emb, fq, level, args.layers)
                    row[f'{name}; level {level}'] = {'prefill_logits_rel_l2_vs_reference': rel_l2(lg, ref), 'first_pick_equal': bool(int(lg.argmax()) == int(ref.argmax()))}
                    print(f'[{time.time() - t0:.0f}s] emulation, shift {sh}, {name}, level {level}: ' + json.dumps(row[f"{name}; level {level}"]), flush=True)
            emu[f'shift {sh}'] = row
            del sd
        rep['cpu_emulation'] = {'layers': args.layers, 'what': 'oracle/internlm2.py forward, the option\'s linears on fake-quantised operands, fp32 accumulation, bf16 result', 'rows': emu}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rep, open(args.out, 'w'), indent=1)
    print('written', args.out)


if __name__ == '__main__':
    main()

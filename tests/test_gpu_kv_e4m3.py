"""The opt-in e4m3 KV cache (cr_kv_alloc_ex CR_KV_E4M3, include/callireader_hip.h) on a real MI355X, 2-layer full-width model:
  - writers: every row the prefill and the decode write is torch's e4m3 quantisation of the row a bf16 cache holds (rope_split_kernel<true>), the
    prefill's logits and first ids are the bf16 cache's bits, and every decode form (fused / folded / separate kernels) writes the same bytes;
  - reader: decode_attn8_kernel against a float64 evaluation of its rule, no worse than the bf16 kernel against its own, deterministic;
  - model level: teacher-forced logits against a CPU decode step built from oracle/internlm2.py with every cached row replaced by its e4m3 round trip;
  - a page's ids do not depend on its batch or on the entry point; the command line; the refusals."""
import os
import subprocess
import sys

import pytest
import torch

from callireader_amd import synthetic
from callireader_amd.config import ModelDims
from test_gpu_boundary import _write_folder, ckpt  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
ATOL = 0.12
RTOL_L2 = 2.5e-2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def quant_rows(x):
    """torch's replica of the cache quantiser: rows of 128 -> (e4m3 bytes as uint8, fp32 scale)."""
    xf = x.float()
    m = xf.abs().amax(-1)
    s = torch.where(m > 0, m / 448.0, torch.ones_like(m))
    q = (xf * (1.0 / s)[..., None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), s


def dequant(q, s):
    return q.view(torch.float8_e4m3fn).float() * s[..., None]


@pytest.fixture(scope='module')
def setup():
    from callireader_amd.engine import Engine
    dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=8201)
    sd = synthetic.make_state_dict(dims, parts=('llm',), seed=0)
    eng = Engine(dims, max_pos=2048)
    eng.load_state_dict(sd)
    eng.load_rope()
    eng.finalize()
    others = {}
    for name, env in (('nofused', 'CR_DECODE_FUSED'), ('nofold', 'CR_DECODE_FOLD_ROPE')):
        os.environ[env] = '0'
        try:
            e = Engine(dims, max_pos=2048)
        finally:
            del os.environ[env]
        e.share_weights_from(eng)
        others[name] = e
    yield dict(eng=eng, dims=dims, sd=sd, **others)
    for e in others.values():
        e.close()


def prompt(S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, S, 4096, generator=g) * 0.02).to(torch.bfloat16)


def check_row(kvb, kv8, layer, seq, pos, what):
    for which in (0, 1):
        q, s = (t.cpu() for t in kv8.read_e4m3(layer, seq, pos, which))
        qr, sr = quant_rows(kvb.read(layer, seq, pos, which).cpu())     # on the CPU: torch's GPU division by a scalar multiplies by its reciprocal
        assert torch.equal(s, sr), (what, layer, seq, pos, which, s, sr)
        assert torch.equal(q, qr), (what, layer, seq, pos, which, int((q != qr).sum()))


def test_prefill_rows_and_logits(setup):
    eng = setup['eng']
    lens = [255, 256, 257, 31]
    embs = [prompt(S, 40 + i) for i, S in enumerate(lens)]
    kvb, kv8 = eng.kv_alloc(4, 600), eng.kv_alloc(4, 600, dtype='e4m3')
    assert (kvb.format, kv8.format) == ('bf16', 'e4m3')
    lb = eng.prefill_batch(kvb, [0, 1, 2, 3], [e.cuda() for e in embs], want_logits=True)
    l8 = eng.prefill_batch(kv8, [0, 1, 2, 3], [e.cuda() for e in embs], want_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(lb, l8)
    assert [kvb.generated(i) for i in range(4)] == [kv8.generated(i) for i in range(4)]
    for i, S in enumerate(lens):
        assert kv8.length(i) == S
        for layer in (0, 1):
            for pos in range(S):
                check_row(kvb, kv8, layer, i, pos, 'prefill')
    kvb.free(); kv8.free()


@pytest.mark.parametrize('rows', [1, 8, 13, 64])
def test_decode_rows_are_the_quantised_bf16_rows(setup, rows):
    """Teacher-forced ids: layer 0's new rows (whose input is the forced token's embedding) are the quantisation of the bf16 run's rows; in every
    layer a written row holds its +-448 byte, and the default, CR_DECODE_FUSED=0 and CR_DECODE_FOLD_ROPE=0 contexts write the same bytes.  Cache
    lengths pass 255 .. 258 and 510 .. 513 (the 256-key splits)."""
    eng = setup['eng']
    base = [252, 507, 20, 33, 9, 130]
    lens = [base[i % len(base)] + (i // len(base)) for i in range(rows)]
    embs = [prompt(S, 900 + i) for i, S in enumerate(lens)]
    steps = 6
    g = torch.Generator().manual_seed(rows)
    forced = torch.randint(0, setup['dims'].vocab, (steps, rows), generator=g)
    kvb = eng.kv_alloc(rows, 540)
    kv8 = {n: setup[n].kv_alloc(rows, 540, dtype='e4m3') if n != 'eng' else eng.kv_alloc(rows, 540, dtype='e4m3') for n in ('eng', 'nofused', 'nofold')}
    seqs = list(range(rows))
    for i0 in range(0, rows, 16):
        idx = seqs[i0:i0 + 16]
        eng.prefill_batch(kvb, idx, [embs[i].cuda() for i in idx])
        for n, kv in kv8.items():
            (eng if n == 'eng' else setup[n]).prefill_batch(kv, idx, [embs[i].cuda() for i in idx])
    order = seqs[::-1]
    for t in range(steps):
        ft = forced[t][order]
        eng.decode(kvb, order, force_tokens=ft)
        for n, kv in kv8.items():
            (eng if n == 'eng' else setup[n]).decode(kv, order, force_tokens=ft)
    torch.cuda.synchronize()
    for i, S in enumerate(lens):
        for t in range(steps):
            pos = S + t
            check_row(kvb, kv8['eng'], 0, i, pos, f'decode rows={rows} step={t}')
            for layer in (0, 1):
                for which in (0, 1):
                    q, s = kv8['eng'].read_e4m3(layer, i, pos, which)
                    for n in ('nofused', 'nofold'):
                        q2, s2 = kv8[n].read_e4m3(layer, i, pos, which)
                        assert torch.equal(q, q2) and torch.equal(s, s2), (n, rows, i, t, layer, which)
                    qc = q.cpu()
                    has = ((qc & 0x7f) == 0x7e).any(-1)
                    nonzero = (qc & 0x7f).any(-1)
                    assert bool((has | ~nonzero).all()), (rows, i, t, layer, which)
    kvb.free()
    for kv in kv8.values():
        kv.free()


def _reader_case(rows, key_counts, seed):
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(seed)
    lens = torch.tensor([key_counts[i % len(key_counts)] - 1 for i in range(rows)], dtype=torch.int32, device=dev)
    T = max(key_counts) + 8
    x = torch.randn(rows, 8, T, 128, device=dev, generator=g) * torch.exp(torch.randn(rows, 8, T, 1, device=dev, generator=g))
    k8, ks = quant_rows(x)
    x = torch.randn(rows, 8, T, 128, device=dev, generator=g) * torch.exp(torch.randn(rows, 8, T, 1, device=dev, generator=g))
    v8, vs = quant_rows(x)
    q = (torch.randn(rows, 4096, device=dev, generator=g) * 0.3).to(torch.bfloat16)
    seqs = torch.arange(rows, dtype=torch.int32, device=dev)
    return q, k8.contiguous(), v8.contiguous(), ks.contiguous(), vs.contiguous(), seqs, lens


def _attn64(q, K, V, lens):
    """float64 decode attention: q (B, 4096), K / V (B, 8, T, 128) float64 values, lens + 1 keys per row -> (B, 4096)"""
    B = q.shape[0]
    out = torch.empty(B, 32, 128, dtype=torch.float64, device=q.device)
    qh = q.double().view(B, 8, 4, 128)
    for b in range(B):
        n = int(lens[b]) + 1
        s = torch.einsum('hqd,hkd->hqk', qh[b], K[b, :, :n]) / 128 ** 0.5
        p = torch.softmax(s, -1)
        out[b] = torch.einsum('hqk,hkd->hqd', p, V[b, :, :n]).reshape(32, 128)
    return out.reshape(B, 4096)


@pytest.mark.parametrize('rows', [1, 13, 64])
def test_reader_against_float64(rows):
    """Error = rel-L2 over every output of the launches against the float64 result rounded to bf16 (both readers write bf16; a max |diff| is set
    by the largest outputs' last bit).  One row: each key count in turn, the errors summed over the five launches."""
    from callireader_amd.engine import op_decode_attention, op_decode_attention_e4m3
    key_counts = [1, 255, 256, 257, 3164]
    acc = {'e4m3': [0.0, 0.0], 'bf16': [0.0, 0.0]}

    def add(k, o, r):
        acc[k][0] += float(((o.double() - r.double()) ** 2).sum())
        acc[k][1] += float((r.double() ** 2).sum())
    for kc in ([[k] for k in key_counts] if rows == 1 else [key_counts]):
        q, k8, v8, ks, vs, seqs, lens = _reader_case(rows, kc, 5 + rows + kc[0])
        Kd, Vd = dequant(k8, ks).double(), dequant(v8, vs).double()
        max_keys = max(kc)
        o8 = op_decode_attention_e4m3(q, k8, v8, ks, vs, seqs, lens, max_keys=max_keys)
        o8b = op_decode_attention_e4m3(q, k8, v8, ks, vs, seqs, lens, max_keys=max_keys)
        torch.cuda.synchronize()
        assert torch.equal(o8, o8b)                               # the partials' merge is deterministic
        add('e4m3', o8, _attn64(q, Kd, Vd, lens).to(torch.bfloat16))
        Kb, Vb = Kd.to(torch.bfloat16), Vd.to(torch.bfloat16)
        del Kd, Vd
        ob = op_decode_attention(q, Kb.contiguous(), Vb.contiguous(), seqs, lens, max_keys=max_keys)
        add('bf16', ob, _attn64(q, Kb.double(), Vb.double(), lens).to(torch.bfloat16))
        # a row's result depends on its own key count only: row 0 alone gives the same bits
        o1 = op_decode_attention_e4m3(q[:1].contiguous(), k8, v8, ks, vs, seqs[:1].contiguous(), lens[:1].contiguous(), max_keys=max_keys)
        torch.cuda.synchronize()
        assert torch.equal(o1[0], o8[0])
    err8, errb = ((a / b) ** 0.5 for a, b in (acc['e4m3'], acc['bf16']))
    print(f'rows {rows}: rel-L2 error e4m3 reader {err8:.3e}, bf16 reader {errb:.3e} (ratio {err8 / errb:.2f})')
    assert err8 <= 1.5 * errb, (err8, errb)


def _emulated_attention(orig):
    """oracle/internlm2.attention with every cached K / V row, the current one included, replaced by its e4m3 round trip in a decode step
    (q_len == 1); the prefill attends over bf16, as the engine's does.  The returned cache stays bf16 (what the quantiser reads)."""
    import math
    import torch.nn.functional as F
    from oracle import internlm2 as I

    def rt(x):
        q, s = quant_rows(x)
        return dequant(q, s)                      # fp32: exact

    def attention(sd, p, x, position_ids, past_kv, cos_t, sin_t, n_heads=32, n_kv=8):
        B, q_len, D = x.shape
        if q_len != 1:
            return orig(sd, p, x, position_ids, past_kv, cos_t, sin_t, n_heads, n_kv)
        hd = D // n_heads
        groups = n_heads // n_kv
        qkv = F.linear(x, sd[p + 'attention.wqkv.weight']).view(B, q_len, n_kv, groups + 2, hd)
        q = qkv[..., :groups, :].reshape(B, q_len, n_heads, hd).transpose(1, 2)
        k = qkv[..., -2, :].transpose(1, 2)
        v = qkv[..., -1, :].transpose(1, 2)
        kv_len = q_len + past_kv[0].shape[-2]
        q, k = I.apply_rope(q, k, cos_t[:kv_len].to(x.dtype), sin_t[:kv_len].to(x.dtype), position_ids)
        k = torch.cat([past_kv[0], k], dim=2)
        v = torch.cat([past_kv[1], v], dim=2)
        kq, vq = rt(k), rt(v)
        kr = kq[:, :, None].expand(B, n_kv, groups, kv_len, hd).reshape(B, n_heads, kv_len, hd)
        vr = vq[:, :, None].expand(B, n_kv, groups, kv_len, hd).reshape(B, n_heads, kv_len, hd)
        # the reference's rounding points on the dequantised rows, the products in fp32 (rule 3: bf16 scores, / sqrt(128) in bf16, bf16 probabilities)
        w = torch.matmul(q.float(), kr.transpose(2, 3)).to(q.dtype) / math.sqrt(hd)
        w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        o = torch.matmul(w.float(), vr).to(q.dtype).transpose(1, 2).contiguous().reshape(B, q_len, D)
        return F.linear(o, sd[p + 'attention.wo.weight']), (k, v)
    return attention


@pytest.mark.parametrize('penalty', [1.0, 1.5])
def test_model_level_against_an_emulated_oracle(setup, penalty, monkeypatch):
    from oracle import internlm2 as I, generate
    from test_gpu_llm import check_stream
    eng, sd = setup['eng'], setup['sd']
    monkeypatch.setattr(I, 'attention', _emulated_attention(I.attention))
    drift, agree, total = [], 0, 0
    for j, S in enumerate((300, 77, 129)):
        emb = prompt(S, 300 + j)
        with torch.no_grad():
            ids, logits = generate.greedy_generate(sd, 2, emb, max_new_tokens=13, eos_token_id=-1, repetition_penalty=penalty, return_logits=True)
        ref_ids = ids[0].tolist()
        kv8 = eng.kv_alloc(1, 512, dtype='e4m3')
        div = check_stream(eng, kv8, 0, emb, ref_ids, logits, penalty=penalty)
        if div:
            print(f'S={S} penalty {penalty}: picks differed from the emulated oracle at measured near-ties, steps {div}')
        # drift against the bf16 cache along the same forced ids
        kvb = eng.kv_alloc(1, 512)
        kv8.reset()
        lb = eng.prefill(kvb, 0, emb.cuda(), penalty=penalty, want_logits=True)
        l8 = eng.prefill(kv8, 0, emb.cuda(), penalty=penalty, want_logits=True)
        for t in range(len(ref_ids)):
            torch.cuda.synchronize()
            drift.append(rel_l2(l8.float().cpu().reshape(-1), lb.float().cpu().reshape(-1)))
            agree += int(torch.argmax(l8) == torch.argmax(lb))
            total += 1
            if t + 1 < len(ref_ids):
                ft = torch.tensor([ref_ids[t]])
                lb = eng.decode(kvb, [0], penalty=penalty, force_tokens=ft, want_logits=True)
                l8 = eng.decode(kv8, [0], penalty=penalty, force_tokens=ft, want_logits=True)
        kvb.free(); kv8.free()
    print(f'penalty {penalty}: e4m3 vs bf16 cache: logit rel-L2 max {max(drift):.4f} mean {sum(drift) / len(drift):.4f}, '
          f'greedy agreement {agree}/{total}')
    assert max(drift) <= 0.15
    assert agree >= 0.6 * total


@pytest.fixture(scope='module')
def chat(setup):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = setup['dims']
    m = InternVLChatModel(dims, max_tokens=640, max_pages=1, kv_cache_dtype='e4m3')
    for k, v in setup['sd'].items():
        m.engine.load_weight(k, v if v.dtype == torch.bfloat16 or not v.is_floating_point() else v.to(torch.bfloat16))
    m._finish()
    m.img_context_token_id = 92546 % dims.vocab
    yield m
    m.close()


def test_a_pages_ids_do_not_depend_on_its_batch_or_entry_point(chat):
    from callireader_amd.continuous import ContinuousPipeline
    from callireader_amd.sampling import SamplingParams, page_seeds
    m = chat
    assert m.kv_cache_dtype == 'e4m3'
    V = m.dims.vocab
    lens = [40 + (i * 37) % 300 for i in range(64)]
    g = torch.Generator().manual_seed(3)
    ids = [torch.randint(0, V, (S,), generator=g) for S in lens]
    embs = [m.engine.embed_splice(x) for x in ids]
    N, eos, pen = 10, None, 1.3
    for fp8 in (False, True):
        m.engine.enable_fp8_decode(fp8)
        for sp in (None, SamplingParams(temperature=0.8, top_k=20, top_p=0.9)):
            seeds = page_seeds(64, base=17)
            kw = dict(sampling=sp, seeds=seeds) if sp is not None else {}
            full = m.generate_pages(embs, N, eos, pen, **kw)
            assert m._kv.format == 'e4m3'
            for P in (1, 13):
                kwp = dict(sampling=sp, seeds=seeds[:P]) if sp is not None else {}
                assert m.generate_pages(embs[:P], N, eos, pen, **kwp) == full[:P], (fp8, sp, P)
            pipe = m.page_pipeline(max_new_tokens=N, eos_token_id=eos, repetition_penalty=pen)
            try:
                assert pipe.start(embs[:13], sampling=sp, seeds=seeds[:13] if sp is not None else None) is None
                assert pipe.finish() == full[:13], (fp8, sp, 'PagePipeline')
                assert {kv.format for kv in pipe.kvs if kv is not None} == {'e4m3'}
                with pytest.raises(RuntimeError):
                    m.kv_cache_dtype = 'bf16'                     # refused while a pipeline made from the model is open
            finally:
                pipe.close()
            cp = ContinuousPipeline(m, slots=2, spare=1, max_new_tokens=N, eos_token_id=-1, repetition_penalty=pen, admit_group=1)
            try:
                assert cp.kv.format == 'e4m3'
                tickets = [cp.submit(embs[i], sampling=sp, seed=seeds[i] if sp is not None else None) for i in range(5)]
                got = dict(cp.ready())
                for t, x in cp.results():
                    got[t] = x
                assert [got[t] for t in tickets] == full[:5], (fp8, sp, 'ContinuousPipeline')
            finally:
                cp.close()
            gk = dict(max_new_tokens=N, eos_token_id=None, do_sample=sp is not None)
            if sp is not None:
                gk.update(temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p)
                torch.manual_seed(11)
                seed0 = page_seeds(1)[0]
                torch.manual_seed(11)
                want = m.generate_pages(embs[:1], N, eos, pen, sampling=sp, seeds=[seed0])[0]
                torch.manual_seed(11)
            else:
                want = full[0]
            out = m.generate_ocr(input_ids=ids[0][None], repetition_penalty=pen, **gk)
            assert out[0].tolist() == want, (fp8, sp, 'generate_ocr')
    m.engine.enable_fp8_decode(False)
    # the format follows the model: switching back gives the bf16 cache
    m.kv_cache_dtype = 'bf16'
    assert m._kv is None and m.kv(1).format == 'bf16'
    m.kv_cache_dtype = 'e4m3'


def test_refusals_leave_the_context_working(setup):
    from callireader_amd._binding import CalliReaderError
    eng = setup['eng']
    kv8 = eng.kv_alloc(2, 300, dtype='e4m3')
    emb = prompt(50, 1).cuda()
    eng.prefill(kv8, 0, emb)
    with pytest.raises(CalliReaderError, match='e4m3'):
        kv8.read(0, 0, 0)
    with pytest.raises(CalliReaderError, match='already holds'):
        eng.prefill(kv8, 0, emb)
    kvb = eng.kv_alloc(1, 300)
    with pytest.raises(CalliReaderError, match='bf16'):
        kvb.read_e4m3(0, 0, 0)
    eng.prefill(kvb, 0, emb)
    for _ in range(3):
        eng.decode(kv8, [0])
        eng.decode(kvb, [0])
    assert kv8.length(0) == 53 and len(kv8.generated(0)) == 4
    kv8.reset(0)
    eng.prefill(kv8, 0, emb)                                     # after a reset the sequence takes a prefill again
    assert kv8.length(0) == 50
    kv8.free(); kvb.free()


def test_matrix_core_decode_refuses_an_e4m3_cache():
    """CR_DECODE_ATTN=0 (read once per process) selects the matrix-core split kernel, which reads bf16 only: an e4m3 cache is refused, a bf16
    cache still decodes."""
    code = r'''
import torch
from callireader_amd import synthetic
from callireader_amd.config import ModelDims
from callireader_amd.engine import Engine, op_decode_attention_e4m3
from callireader_amd._binding import CalliReaderError
dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=8201)
eng = Engine(dims, max_pos=512)
eng.load_state_dict(synthetic.make_state_dict(dims, parts=('llm',), seed=0))
eng.load_rope(); eng.finalize()
emb = (torch.randn(1, 20, 4096) * 0.02).to(torch.bfloat16).cuda()
kv8, kvb = eng.kv_alloc(1, 64, dtype='e4m3'), eng.kv_alloc(1, 64)
eng.prefill(kv8, 0, emb); eng.prefill(kvb, 0, emb)
try:
    eng.decode(kv8, [0]); print('NOT REFUSED')
except CalliReaderError as e:
    print('refused:', 'CR_DECODE_ATTN' in str(e))
eng.decode(kvb, [0]); torch.cuda.synchronize()
print('bf16 ok', len(kvb.generated(0)), kv8.length(0))
'''
    env = dict(os.environ, CR_DECODE_ATTN='0')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    assert 'refused: True' in out and 'bf16 ok 2 20' in out, out[-2000:]


def test_cli_fp8_kv(ckpt, tmp_path, monkeypatch):
    """inference.py --fp8_kv on a folder: image order and the per-image ERROR! pattern kept, each response equals the page's own (serial, per-page
    chat_ocr) run with an e4m3 cache, and without the switch the JSON is byte for byte the default run's."""
    import json
    from PIL import Image
    from callireader_amd import inference as inf
    d = str(tmp_path / 'pages')
    paths, bad = _write_folder(None, d, n_good=4)
    raw = [[300, 310, 380, 480], [10, 20, 110, 140], [200, 50, 420, 300]]
    for p in paths:
        if p == bad:
            continue
        w, h = Image.open(p).size
        shapes = [{'points': [[b[0] / w * 0.5, b[1] / h * 0.5], [b[2] / w * 0.5, b[3] / h * 0.5]]} for b in raw]
        json.dump({'imageHeight': h, 'imageWidth': w, 'shapes': shapes}, open(os.path.splitext(p)[0] + '.json', 'w'))
    monkeypatch.chdir(tmp_path)
    common = ['--tgt', d, '--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '8']

    def run(name, *extra):
        inf.main(common + ['--save_name', name] + list(extra))
        return open(tmp_path / 'results' / name, 'rb').read()
    default = run('default.json', '--batch_pages', '3')
    fp8 = run('kv8.json', '--batch_pages', '3', '--fp8_kv')
    serial = run('kv8_serial.json', '--batch_pages', '1', '--fp8_kv')
    assert run('default_again.json', '--batch_pages', '3') == default
    a, s, g = (json.loads(x.decode('utf-8')) for x in (fp8, serial, default))
    assert [r['imagePath'] for r in a] == [r['imagePath'] for r in g] == paths
    assert [r['response'] == 'ERROR!' for r in a] == [p == bad for p in paths]
    assert [r['response'] for r in a] == [r['response'] for r in s]
    print('e4m3 cache responses equal to the bf16 ones on', sum(x['response'] == y['response'] for x, y in zip(a, g)), 'of', len(a), 'pages')

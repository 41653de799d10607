"""Sampled generation on the device (csrc/sample.hip, ABI v12 cr_kv_set_sampling / cr_op_sample).

  - the kept set of cr_op_sample against the installed transformers' own RepetitionPenalty / Temperature / TopK / TopP processors;
  - every draw against the host replica (the same warpers, Gumbel noise from the numpy Philox in float64, argmax);
  - the draw distribution against HF's filtered softmax (chi-square, seeded: deterministic);
  - greedy rows beside sampled rows keep their bits, top_k = 1 and temperature 0 are greedy;
  - a sampled page's ids do not depend on its batch, its slot or the pipeline that decodes it; each step's id is the host replica's;
  - the public surface: torch.manual_seed makes chat reproducible."""
import numpy as np
import pytest
import torch

from callireader_amd import sampling as S
from callireader_amd import synthetic
from callireader_amd.config import ModelDims

pytestmark = pytest.mark.gpu

V_FULL, V_RAGGED = 92553, 9001


def hf_filter(logits, hist, penalty, T, k, p):
    """transformers' processors in _get_logits_processor's order on one fp32 row (CPU): the processed scores, -inf where removed."""
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    x = torch.as_tensor(logits, dtype=torch.float32).reshape(1, -1).clone()
    ids = torch.as_tensor(hist, dtype=torch.long).reshape(1, -1)
    if penalty != 1.0 and ids.numel():
        x = RepetitionPenaltyLogitsProcessor(penalty)(ids, x)
    if T != 1.0:
        x = TemperatureLogitsWarper(T)(ids, x)
    if k != 0:
        x = TopKLogitsWarper(k)(ids, x)
    if p < 1.0:
        x = TopPLogitsWarper(p)(ids, x)
    return x[0]


def boundary_case(z, z_all, p, kept):
    """Why the device's kept count may differ from HF's, or None: 'tie' when it equals HF's set extended by the ids tied with HF's smallest kept
    score (the documented tie rule: an exact tie AT the boundary value), 'near' when the softmax cumsum of the top-k survivors (z_all) passes
    within 1e-6 of 1 - top_p."""
    if kept == int(torch.isfinite(tie_extended(z, z_all)).sum()):
        return 'tie'
    if p < 1.0:
        srt = torch.sort(z_all[torch.isfinite(z_all)]).values
        cum = torch.softmax(srt, 0).cumsum(0)
        if torch.any((cum - (1 - p)).abs() < 1e-6):
            return 'near'
    return None


def tie_extended(z, z_all):
    """The device's kept set from HF's: every id tied with the smallest kept score is kept too (these logits come out of bf16 products and
    hold exact ties; HF's torch.sort order keeps only some of them at the top-p boundary)."""
    thr = z[torch.isfinite(z)].min()
    return torch.where(z_all >= thr, z_all, torch.full_like(z_all, -float('inf')))


def replica_draw(z, seed, step):
    """argmax over kept ids of z + g (float64); also the gap between the two best perturbed scores."""
    kept = torch.nonzero(torch.isfinite(z)).reshape(-1).numpy()
    sc = z.numpy()[kept].astype(np.float64) + S.gumbel(seed, step, kept)
    o = np.argsort(-sc, kind='stable')
    gap = sc[o[0]] - sc[o[1]] if len(o) > 1 else np.inf
    return int(kept[o[0]]), gap


@pytest.fixture(scope='module')
def eng():
    from callireader_amd.engine import Engine
    e = Engine(ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1))
    yield e
    e.close()


@pytest.mark.parametrize('V', [V_FULL, V_RAGGED])
def test_kept_set_and_draws_match_hf(eng, V):
    from callireader_amd.engine import op_sample
    g = torch.Generator().manual_seed(V)
    n = 6
    logits = torch.randn(n, V, generator=g) * 2.5
    hist = torch.randint(0, V, (n, 40), generator=g)
    hist_len = [0, 5, 17, 40, 40, 33]
    draws = near = kept_exc = rows = 0
    for T in (0.7, 1.0, 1.3):
        for k in (0, 1, 50, 1000, V):
            for p in (1.0, 0.95, 0.8, 0.0):
                seeds = [S.splitmix64(1000 * T + 10 * k + 100 * p + r) for r in range(n)]
                steps = [r * 37 + k % 5 for r in range(n)]
                ids, kept = op_sample(eng, logits, T, k, p, seeds, steps, history=hist, hist_len=hist_len, penalty=1.5)
                ids, kept = ids.cpu().tolist(), kept.cpu().tolist()
                for r in range(n):
                    rows += 1
                    z = hf_filter(logits[r], hist[r, :hist_len[r]], 1.5, T, k, p)
                    want = int(torch.isfinite(z).sum())
                    if kept[r] != want:
                        why = boundary_case(z, hf_filter(logits[r], hist[r, :hist_len[r]], 1.5, T, k, 1.0), p, kept[r])
                        assert why, f'T={T} k={k} p={p} row {r}: kept {kept[r]} vs HF {want}'
                        kept_exc += 1
                        continue
                    wid, gap = replica_draw(z, seeds[r], steps[r])
                    draws += 1
                    if gap < 1e-4:
                        near += 1
                        continue
                    assert ids[r] == wid, f'T={T} k={k} p={p} row {r}: id {ids[r]} vs replica {wid} (gap {gap})'
    print(f'V={V}: {rows} rows, {kept_exc} kept-set boundary exceptions, {draws} draws, {near} near-ties')
    assert draws >= 256 and near <= 0.005 * draws and kept_exc <= 0.02 * rows


def test_greedy_rows_and_temperature_zero(eng):
    from callireader_amd.engine import op_sample
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(8, V_FULL, generator=g)
    ids, kept = op_sample(eng, logits, 0.0, 50, 0.9, 1, 0)
    assert ids.cpu().tolist() == logits.argmax(1).tolist() and kept.cpu().tolist() == [0] * 8
    ids1, kept1 = op_sample(eng, logits, 1.0, 1, 1.0, list(range(8)), 3)
    assert ids1.cpu().tolist() == logits.argmax(1).tolist() and kept1.cpu().tolist() == [1] * 8


def test_distribution_chi_square(eng):
    from scipy.stats import chisquare
    from callireader_amd.engine import op_sample
    V, N, k = 1000, 1 << 15, 20
    g = torch.Generator().manual_seed(11)
    row = torch.randn(V, generator=g) * 1.5
    z = hf_filter(row, [], 1.0, 1.0, k, 1.0)
    probs = torch.softmax(z.double(), 0).numpy()
    counts = np.zeros(V)
    seed = 0xC0FFEE
    for s0 in range(0, N, 4096):
        ids, kept = op_sample(eng, row.expand(4096, V), 1.0, k, 1.0, seed, torch.arange(s0, s0 + 4096))
        assert set(kept.cpu().tolist()) == {k}
        np.add.at(counts, ids.cpu().numpy(), 1)
    keep = probs > 0
    assert counts[~keep].sum() == 0
    p = chisquare(counts[keep], probs[keep] * N).pvalue
    print(f'chi-square p = {p:.4g}')
    assert p > 1e-4


@pytest.fixture(scope='module')
def llm():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=9000)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=3), dims, max_tokens=512, max_pages=64)
    g = torch.Generator().manual_seed(1)
    ids = [torch.randint(0, 9000, (int(n),), generator=g) for n in torch.randint(20, 90, (64,), generator=g)]
    pages = [m.engine.embed_splice(i) for i in ids]
    yield m, pages, ids
    m.close()


GEN = dict(max_new_tokens=24, eos_token_id=None, repetition_penalty=1.3)


def test_greedy_pages_untouched_beside_sampled(llm):
    m, pages, _ = llm
    greedy = m.generate_pages(pages[:13], **GEN)
    sp = S.SamplingParams(1.0, 50, 0.9)
    mix = [sp if i % 2 else None for i in range(13)]                       # 6 sampled, 7 greedy
    out = m.generate_pages(pages[:13], **GEN, sampling=mix, seeds=list(range(100, 113)))
    for i in range(0, 13, 2):
        assert out[i] == greedy[i]
    assert sum(out[i] != greedy[i] for i in range(1, 13, 2)) >= 3
    top1 = m.generate_pages(pages[:13], **GEN, sampling=S.SamplingParams(1.0, 1, 1.0), seeds=list(range(13)))
    for i in range(13):
        if top1[i] != greedy[i]:                           # only where the greedy stream meets an exact tie of the top score (both ids kept)
            assert greedy_meets_tie(m, pages[i], greedy[i]), i


def greedy_meets_tie(m, page, ids):
    """Whether the penalised scores of the page's greedy stream hold an exact tie for the maximum at some step."""
    kv = m.kv()
    kv.reset()
    pen = GEN['repetition_penalty']
    lgs = [m.engine.prefill(kv, 0, page, penalty=pen, want_logits=True).cpu()]
    for _ in range(len(ids) - 1):
        lgs.append(m.engine.decode(kv, [0], penalty=pen, want_logits=True)[0].cpu())
    assert kv.generated(0) == ids
    for step, lg in enumerate(lgs):
        z = hf_filter(lg, ids[:step], pen, 1.0, 0, 1.0)
        if int((z == z.max()).sum()) > 1:
            return True
    return False


def test_batch_invariance(llm):
    m, pages, ids = llm
    sp = S.SamplingParams(1.2, 0, 0.95)
    torch.manual_seed(42)
    seed = S.page_seeds(1)[0]                                  # what a one-page public call draws after torch.manual_seed(42)
    m.img_context_token_id = 8990
    try:
        for fp8 in (False, True):
            m.engine.enable_fp8_decode(fp8)
            _batch_invariance(m, pages, ids, sp, seed, fp8)
    finally:
        m.engine.enable_fp8_decode(False)


def _batch_invariance(m, pages, ids, sp, seed, fp8):
    from callireader_amd.continuous import ContinuousPipeline
    torch.manual_seed(42)
    alone = m.generate_ocr(input_ids=ids[7][None], repetition_penalty=GEN['repetition_penalty'], max_new_tokens=GEN['max_new_tokens'],
                           eos_token_id=None, do_sample=True, temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p)[0].tolist()
    assert alone == m.generate_pages([pages[7]], **GEN, sampling=sp, seeds=[seed])[0]
    for P, at in ((13, 5), (64, 40)):
        order = [i for i in range(P) if i != 7]
        order.insert(at, 7)
        mix = [sp if (j % 3 == 0 or j == at) else None for j in range(P)]
        seeds = [seed if j == at else S.splitmix64(j) for j in range(P)]
        out = m.generate_pages([pages[i] for i in order], **GEN, sampling=mix, seeds=seeds)
        assert out[at] == alone, (fp8, P)
    pipe = m.page_pipeline(max_new_tokens=GEN['max_new_tokens'], eos_token_id=None, repetition_penalty=GEN['repetition_penalty'])
    try:
        pipe.start([pages[1], pages[7], pages[2]], sampling=[None, sp, sp], seeds=[1, seed, 2])
        assert pipe.finish()[1] == alone
    finally:
        pipe.close()
    cp = ContinuousPipeline(m, slots=2, max_new_tokens=GEN['max_new_tokens'], eos_token_id=None, repetition_penalty=GEN['repetition_penalty'],
                            admit_group=1)
    try:
        tickets = [cp.submit(pages[i], sampling=sp if i == 7 else None, seed=seed if i == 7 else None) for i in (3, 4, 5, 6, 7)]
        got = dict(cp.results())
        assert got[tickets[-1]] == alone
    finally:
        cp.close()
    other = m.generate_pages([pages[7]], **GEN, sampling=sp, seeds=[seed + 1])[0]
    assert other != alone


def test_stream_replays_on_host(llm):
    """Each id of a sampled stream is the host replica's draw from that step's raw logits (penalty over the ids sampled before it)."""
    m, pages, _ = llm
    kv = m.kv()
    kv.reset()
    sp, seed, pen = S.SamplingParams(0.9, 200, 0.9), 77, 1.5
    kv.set_sampling(0, sp.temperature, sp.top_k, sp.top_p, seed)
    lgs = [m.engine.prefill(kv, 0, pages[0], penalty=pen, want_logits=True).cpu()]
    for _ in range(63):
        lgs.append(m.engine.decode(kv, [0], penalty=pen, want_logits=True)[0].cpu())
    ids = kv.generated(0)
    assert len(ids) == 64
    near = 0
    for step, lg in enumerate(lgs):
        z = tie_extended(hf_filter(lg, ids[:step], pen, sp.temperature, sp.top_k, sp.top_p),
                         hf_filter(lg, ids[:step], pen, sp.temperature, 0, 1.0))
        wid, gap = replica_draw(z, seed, step)
        if gap < 1e-4:
            near += 1
            continue
        assert ids[step] == wid, step
    assert near <= 1


def test_chat_reproducible_with_manual_seed():
    from chat_helpers import FakeTokenizer
    from callireader_amd import preprocess
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    from PIL import Image
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=9000)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=0), dims, max_tokens=4096)
    try:
        tok = FakeTokenizer()
        img = Image.fromarray(np.random.default_rng(0).integers(0, 255, (448, 448, 3), dtype=np.uint8))
        px = preprocess.load_image(img).to(torch.bfloat16).cuda()
        gen = dict(do_sample=True, max_new_tokens=16)
        torch.manual_seed(0)
        a = m.chat(tok, px, 'hello', gen)
        torch.manual_seed(0)
        b = m.chat(tok, px, 'hello', gen)
        torch.manual_seed(1)
        c = m.chat(tok, px, 'hello', gen)
        assert a == b and a != c
        greedy = m.chat(tok, px, 'hello', dict(max_new_tokens=16))
        assert greedy == m.chat(tok, px, 'hello', dict(max_new_tokens=16, do_sample=False, top_k=5))
    finally:
        m.close()

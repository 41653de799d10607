"""Continuous batching (callireader_amd/continuous.py, ABI v11 cr_kv_set_stop / cr_kv_poll_finished): a finished page's decode row is refilled
at once, and every page keeps the ids of its own generate_pages call.

  - the margin-controlled long streams of tests/golden/peaked_long.npz (built as test_gpu_peaked_long.py builds them: repetition penalty 1.5,
    1024 new tokens), through 2 decode rows: fixture ids with sequences reused, the decode step count of a refilling schedule, a per-page budget;
  - random weights at reduced dimensions: pages of different lengths with mixed budgets and a frequent EOS id against single-page
    generate_pages; at the ABI, a step without stop criteria computes the same bits as before and the finished queue holds each sequence once."""
import json
import os

import numpy as np
import pytest
import torch

from callireader_amd import synthetic
from callireader_amd.config import ModelDims

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'peaked_long.npz')


@pytest.fixture(scope='module')
def peaked():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    g = np.load(GOLD)
    meta = json.loads(bytes(g['meta']).decode())
    P = synthetic.PEAKED_LONG
    dims = ModelDims.reduced(llm_layers=P['llm_layers'])
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    m = InternVLChatModel(dims, max_tokens=1408, max_pages=3)
    for k, v in synthetic.iter_peaked_llm(dims, P['start_a'], seed=meta['seed'], cfg=P):
        m.engine.load_weight(k, v)
    m._finish()
    e = {t: m.engine.embed_splice(torch.from_numpy(g[f'{t}.prompt'].astype(np.int64))) for t in ('LA', 'LB', 'LC')}
    w = {t: g[f'{t}.ids'].tolist() for t in ('LA', 'LB', 'LC')}
    yield m, e, w, meta
    m.engine.close()


def run(m, pages, budgets=None, **kw):
    from callireader_amd.continuous import ContinuousPipeline
    pipe = ContinuousPipeline(m, **kw)
    try:
        tickets = [pipe.submit(p, max_new_tokens=None if budgets is None else budgets[i]) for i, p in enumerate(pages)]
        got = dict(pipe.ready())
        for t, ids in pipe.results():
            assert t not in got, f'ticket {t} returned twice'
            got[t] = ids
        assert sorted(got) == sorted(tickets)
        return [got[t] for t in tickets], dict(pipe.stats)
    finally:
        pipe.close()


def test_fixture_ids_through_two_rows_with_sequences_reused(peaked):
    m, e, w, meta = peaked
    tags = ['LA', 'LB', 'LC', 'LB', 'LC', 'LB']
    outs, stats = run(m, [e[t] for t in tags], slots=2, spare=2, admit_group=1, max_new_tokens=meta['max_new_tokens'],
                      eos_token_id=synthetic.PEAKED_LONG['eos'], repetition_penalty=meta['penalty'])
    for t, o in zip(tags, outs):
        assert o == w[t], (t, len(o), len(w[t]), next((i for i, (a, b) in enumerate(zip(o, w[t])) if a != b), None))
    assert stats['pages_admitted'] == 6 and stats['row_steps'] <= 2 * stats['decode_steps']


def test_refilled_row_keeps_the_step_count_of_the_longest_page(peaked):
    """LA holds one row for 1023 steps while four LBs (84 steps each) cycle through the other: a refilling schedule needs about 1023 decode steps
    (+ a few speculative ones after each EOS), a batch-granular one at least 1023 + 84 + 84."""
    m, e, w, meta = peaked
    tags = ['LA', 'LB', 'LB', 'LB', 'LB']
    outs, stats = run(m, [e[t] for t in tags], slots=2, spare=2, admit_group=1, max_new_tokens=meta['max_new_tokens'],
                      eos_token_id=synthetic.PEAKED_LONG['eos'], repetition_penalty=meta['penalty'])
    assert outs == [w[t] for t in tags]
    assert stats['decode_steps'] <= 1023 + 64, stats
    assert stats['row_steps'] == 1023 + 4 * 84 + stats['speculative_row_steps'], stats


def test_per_page_budget(peaked):
    m, e, w, meta = peaked
    outs, stats = run(m, [e['LA'], e['LB']], budgets=[300, None], slots=2, max_new_tokens=meta['max_new_tokens'],
                      eos_token_id=synthetic.PEAKED_LONG['eos'], repetition_penalty=meta['penalty'])
    assert outs == [w['LA'][:300], w['LB']]
    assert stats['decode_steps'] <= 299 + 8


@pytest.fixture(scope='module')
def small():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=8201)
    sd = synthetic.make_state_dict(dims, parts=('llm',), seed=0)
    m = InternVLChatModel.from_state_dict(sd, dims, max_tokens=768, max_pages=1)
    yield m
    m.engine.close()


def prompts(n, seed=21):
    g = torch.Generator().manual_seed(seed)
    sizes = [40, 170, 33, 64, 90, 20, 300, 51, 77, 128, 5, 211][:n]
    return [(torch.randn(S, 4096, generator=g) * 0.02).to(torch.bfloat16).cuda() for S in sizes]


def test_mixed_budgets_and_frequent_eos_equal_single_page_generate(small):
    pages = prompts(12)
    plain = [small.generate_pages([p], max_new_tokens=40, eos_token_id=None)[0] for p in pages]
    flat = [t for ids in plain for t in ids[2:]]
    eos = max(set(flat), key=flat.count)                        # an id several pages emit: their rows stop at different steps
    budgets = [40, 7, 25, 1, 40, 13, 33, 40, 2, 19, 40, 30]
    want = [small.generate_pages([p], max_new_tokens=b, eos_token_id=eos, repetition_penalty=1.3)[0] for p, b in zip(pages, budgets)]
    assert any(ids[-1] == eos and len(ids) < b for ids, b in zip(want, budgets))
    outs, stats = run(small, pages, budgets=budgets, slots=4, admit_group=3, max_new_tokens=40, eos_token_id=eos, repetition_penalty=1.3)
    assert outs == want
    assert stats['pages_admitted'] == 12 and max(len(o) for o in outs) <= 40


def test_abi_stop_criteria_leave_the_step_unchanged_and_queue_each_sequence_once(small):
    eng = small.engine
    V = eng.dims.vocab
    pages = prompts(4, seed=5)
    plain = eng.kv_alloc(4, 512)
    crit = eng.kv_alloc(4, 512)
    for kv in (plain, crit):
        kv.reset()
    # criteria on `crit` only: EOS for two sequences (one of them chosen so that it fires), a budget for another, none on the last
    eng.prefill_batch(plain, [0, 1, 2, 3], pages, penalty=1.2)
    logits_plain = [eng.decode(plain, [0, 1, 2, 3], penalty=1.2, want_logits=True) for _ in range(6)]
    ids_plain = [plain.generated(s) for s in range(4)]
    eos_hit = ids_plain[0][3]
    first = ids_plain[0].index(eos_hit) + 1
    eng.prefill_batch(crit, [0, 1, 2, 3], pages, penalty=1.2)
    crit.set_stop(0, eos_hit, 0)
    crit.set_stop(1, V - 1 if V - 1 not in ids_plain[1] else V - 2, 0)         # never emitted: never stops
    crit.set_stop(2, None, 4)
    logits_crit = [eng.decode(crit, [0, 1, 2, 3], penalty=1.2, want_logits=True) for _ in range(6)]
    ids_crit = [crit.generated(s) for s in range(4)]
    torch.cuda.synchronize()
    assert ids_crit == ids_plain and all(len(i) == 7 for i in ids_crit)
    for a, b in zip(logits_plain, logits_crit):
        assert torch.equal(a, b)
    for layer in (0, 1):
        for s in range(4):
            for pos in (0, 17, plain.length(s) - 1):
                for which in (0, 1):
                    assert torch.equal(plain.read(layer, s, pos, which), crit.read(layer, s, pos, which))
    buf = torch.zeros(1 + 2 * 4, dtype=torch.int32).pin_memory()
    crit.poll_finished(buf)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    ev.synchronize()
    h = buf.tolist()
    queued = [h[1 + k % 4] for k in range(h[0])]
    assert sorted(queued) == [0, 2], h
    assert h[1 + 4 + 0] == first and h[1 + 4 + 2] == 4 and h[1 + 4 + 1] == 0 and h[1 + 4 + 3] == 0, h
    # a reset sequence can be stopped again: it is queued once more; budgets past the cache or the id capacity are refused
    crit.reset(2)
    eng.prefill(crit, 2, pages[2], penalty=1.2)
    crit.set_stop(2, None, 1)                     # already reached by the prefill's id: recorded at once
    crit.poll_finished(buf)
    torch.cuda.synchronize()
    h = buf.tolist()
    assert h[0] == 3 and h[1 + 2 % 4] == 2 and h[1 + 4 + 2] == 1, h
    from callireader_amd._binding import CalliReaderError
    with pytest.raises(CalliReaderError, match='budget'):
        crit.set_stop(3, None, 512 - crit.length(3) + 1)
    with pytest.raises(CalliReaderError, match='budget'):
        crit.set_stop(3, None, 5000)
    for kv in (plain, crit):
        kv.free()

"""Shared prompts through the stage (cr_kv_fork_shared, cr_kv_set_prefix_sharing) on a real MI355X, at reduced dims (2 layers, vocabulary 9 000).

Every comparison is an equality.  A sequence that shares reads the first pfx_len = n & ~255 cached positions of its source; what it computes must be, bit for
bit, what it computes from a copy:
  - fork_shared copies positions [n & ~255, n) only: below them a destination still holds what it held (a sentinel prompt), behind them too;
  - a fan-out on a cache in sharing mode gives the ids, the raw logits and the log-probabilities of 16 further decode steps that the same calls give on a second
    cache without it -- prompts 255 (nothing shared), 256, 300, 513, and 500 (the steps cross the 512-key boundary: a split goes from partial to full beside
    the shared ones); 1, 7 and 63 destinations -- and the sentinel survives the steps;
  - beam groups (2 pages x 4 beams, a greedy and a sampled neighbour, prompt 300) give the ids and sequences_scores of the unshared run and of
    tests/beam_replica.py;
  - generate_pages(num_return_sequences=4, share_prompt=True) and chat_ocr(num_beams=4, share_prompt=True) equal the calls without the keyword;
  - every lifetime rule refuses with CR_ERR_STATE and leaves every sequence as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from beam_replica import beam_search
from callireader_amd import sampling as S
from callireader_amd import synthetic
from callireader_amd.config import ModelDims

pytestmark = pytest.mark.gpu

V, PEN, LAYERS, STEPS, T = 9000, 1.5, 2, 16, 640
SENTINEL = 3
SP = S.SamplingParams(0.7, 5, 0.8)
ARG, STATE = -1, -3


@pytest.fixture(scope='module')
def llm():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=LAYERS, rs_depth=1, vocab=V)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=3), dims, max_tokens=T, max_pages=64)
    g = torch.Generator().manual_seed(7)
    prompt = m.engine.embed_splice(torch.randint(0, V, (520,), generator=g))
    other = m.engine.embed_splice(torch.randint(0, V, (520 + SENTINEL,), generator=g))
    second = m._kv_alloc(64, T)
    yield m, prompt, other, second
    second.free()
    m.close()


def poll(kv):
    out = torch.zeros(1 + 2 * kv.n_seqs, dtype=torch.int32).pin_memory()
    kv.poll_finished(out)
    torch.cuda.synchronize()
    return out.tolist()


def rows_of(kv, seq, lo, hi, step=1):
    """cache rows lo, lo + step, .. < hi of a sequence's OWN slot: [layer, K|V, position, 8, 128] bf16"""
    return torch.stack([torch.stack([torch.stack([kv.read(l, seq, p, w) for p in range(lo, hi, step)]) for w in (0, 1)]) for l in range(LAYERS)])


def state_of(kv, seqs):
    p, N = poll(kv), kv.n_seqs
    return [(kv.length(s), kv.generated(s), p[1 + N + s]) for s in seqs], p[0]


def prefill_src(m, kv, emb, seed, lpn=0, budget=0, seq=0):
    kv.reset(seq)
    kv.set_sampling(seq, SP.temperature, SP.top_k, SP.top_p, seed)
    if lpn:
        kv.set_logprobs(seq, lpn)
    if budget:
        kv.set_stop(seq, None, budget)
    return m.engine.prefill(kv, seq, emb, penalty=PEN, want_logits=True)


def fresh(kv, share):
    kv.reset()
    kv.set_prefix_sharing(share)


@pytest.mark.parametrize('n', [255, 256, 300, 513])
def test_fork_shared_copies_the_tail_only(llm, n):
    m, prompt, other, second = llm
    kv, dsts, P = m.kv(64), [1, 5], n & ~255
    got = {}
    for cache, shared in ((kv, True), (second, False)):
        cache.reset()
        m.engine.prefill_batch(cache, dsts, [other[:n + SENTINEL]] * 2, penalty=PEN)
        m.engine.prefill(cache, 0, prompt[:n], penalty=PEN)
        before = {s: rows_of(cache, s, 0, n + SENTINEL) for s in [0] + dsts}
        src_state = state_of(cache, [0])
        (cache.fork_shared if shared else cache.fork)(0, dsts, n)
        after = {s: rows_of(cache, s, 0, n + SENTINEL) for s in [0] + dsts}
        got[shared] = (before, after, src_state, state_of(cache, [0]), state_of(cache, dsts))
    before, after, s0, s1, sd = got[True]
    for d in dsts:
        assert torch.equal(after[d][:, :, :P], before[d][:, :, :P]), d               # the shared range was never written: still the sentinel prompt
        assert torch.equal(after[d][:, :, P:n], before[0][:, :, P:n]), d             # the tail is the source's
        assert torch.equal(after[d][:, :, n:], before[d][:, :, n:]), d               # positions >= n untouched
    if P:
        assert not torch.equal(before[1][:, :, :P], before[0][:, :, :P])             # (the sentinel differs from the source: the check above means something)
    assert torch.equal(after[0], before[0]) and s0 == s1                             # the source is unchanged
    assert sd == got[False][4] and sd[0] == [(n, [], 0)] * 2                         # the destinations' state is cr_kv_fork's
    assert torch.equal(got[False][1][1][:, :, :n], before[0][:, :, :n])              # (and cr_kv_fork did copy everything)
    kv.reset()


FAN = [(s, d) for s in (255, 256, 300, 513) for d in (1, 7, 63)] + [(500, 7)]


@pytest.mark.parametrize('S_len,n_dst', FAN)
def test_fanout_with_sharing_equals_fanout_without(llm, S_len, n_dst):
    m, prompt, other, second = llm
    kv = m.kv(64)
    dsts, batch, P = list(range(1, n_dst + 1)), list(range(n_dst + 1)), S_len & ~255
    seeds = [S.splitmix64(1000 + j) for j in range(n_dst)]
    marked = sorted({dsts[0], dsts[-1]})
    res = {}
    for cache, share in ((kv, True), (second, False)):
        fresh(cache, share)
        m.engine.prefill_batch(cache, marked, [other[:S_len + SENTINEL]] * len(marked), penalty=PEN)      # the sentinel
        sent = {d: rows_of(cache, d, 0, max(P, 1), 17) for d in marked}
        row = prefill_src(m, cache, prompt[:S_len], S.splitmix64(5), lpn=3, budget=10)
        cache.fanout(0, dsts, seeds, row)
        lg = [m.engine.decode(cache, batch, penalty=PEN, want_logits=True).clone() for _ in range(STEPS)]
        res[share] = (row.clone(), lg, state_of(cache, batch), [cache.logprobs(s) for s in batch], sent,
                      {d: rows_of(cache, d, 0, max(P, 1), 17) for d in marked})
    a, b = res[True], res[False]
    assert torch.equal(a[0], b[0])
    for t in range(STEPS):
        assert torch.equal(a[1][t], b[1][t]), t                                      # raw logits of every row of every step
        assert not torch.isnan(a[1][t]).any()
    assert a[2] == b[2]                                                              # lengths, all 17 ids, stop counts (the budget of 10), finished count
    assert all(st[0] == S_len + STEPS and len(st[1]) == STEPS + 1 for st in a[2][0])
    for x, y in zip(a[3], b[3]):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))                       # log-probabilities and alternatives
    if P:
        for d in marked:
            assert torch.equal(a[5][d], a[4][d]), d                                  # shared: the destinations' shared range still holds the sentinel
            assert not torch.equal(b[5][d], b[4][d]), d                              # copied: it was overwritten
    fresh(kv, False)
    second.reset()


def beam_run(m, kv, prompt, other, share, n_new=12):
    eng = m.engine
    kv.reset()
    eng.prefill_batch(kv, [1, 2, 3], [other[:300]] * 3, penalty=PEN)                 # what the first group's other sequences hold beforehand
    fresh(kv, share)
    kv.set_beam(0, 4, 1.0, False, None, n_new)
    kv.set_beam(4, 4, 0.0, True, None, n_new)
    kv.set_sampling(9, 0.9, 40, 0.95, 1234)
    eng.prefill_batch(kv, [0, 4, 8, 9], [prompt[:300], prompt[10:310], prompt[20:320], prompt[30:330]], penalty=PEN)
    rows = list(range(10))
    for _ in range(n_new - 1):
        eng.decode(kv, rows, penalty=PEN)
    return kv.beam_result(0), kv.beam_result(4), kv.generated(8), kv.generated(9)


def test_beam_groups_with_sharing_equal_unshared_and_the_replica(llm):
    m, prompt, other, second = llm
    kv = m.kv(64)
    a = beam_run(m, kv, prompt, other, True)
    # the group's other sequences never received rows [0, 256): they still hold the other prompt's
    held = rows_of(kv, 1, 0, 256, 51)
    assert not torch.equal(held, rows_of(kv, 0, 0, 256, 51))
    b = beam_run(m, second, prompt, other, False)
    assert torch.equal(rows_of(second, 1, 0, 256, 51), rows_of(second, 0, 0, 256, 51)) and not torch.equal(rows_of(second, 1, 0, 256, 51), held)      # (copied there)
    assert a == b and a[0][2] and a[1][2] and len(a[2]) == 12 and len(a[3]) == 12     # ids, sequences_scores, done flags; the neighbours' ids
    one = m.engine.kv_alloc(1, T)
    try:
        for res, page, lp, es in ((a[0], prompt[:300], 1.0, False), (a[1], prompt[10:310], 0.0, True)):
            def fn(seqs):
                out = []
                for ids in seqs:
                    one.reset(0)
                    lg = m.engine.prefill(one, 0, page, want_logits=True)
                    for t in ids:
                        lg = m.engine.decode(one, [0], force_tokens=torch.tensor([t]), want_logits=True)[0]
                    out.append(lg.float().cpu())
                return torch.stack(out)
            bm = beam_search(fn, 4, 12, eos_token_id=None, length_penalty=lp, early_stopping=es, repetition_penalty=PEN)
            want_ids, want_sc = bm.result()
            if res[0] != want_ids or abs(res[1] - want_sc) > 1e-5:
                assert bm.min_gap <= 1e-5, (res, want_ids, want_sc, bm.min_gap)          # the replica's own excuse: a float64 tie among its candidates
    finally:
        one.free()
    # dissolving a group releases its shares: resetting its first sequence is accepted (sequences 1..3 read it) and leaves no share behind
    assert kv.length(1) == 300 + 11
    kv.reset(0)
    assert [kv.length(s) for s in range(4)] == [0, 0, 0, 0] and kv.length(4) == 311
    kv.reset(6)                                                                      # ... and so does resetting any other member
    assert [kv.length(s) for s in range(4, 8)] == [0, 0, 0, 0]
    fresh(kv, False)
    second.reset()


def test_through_the_surface(llm):
    m, prompt, other, second = llm
    pages = [prompt[:300], prompt[100:370]]
    kw = dict(max_new_tokens=10, eos_token_id=None, repetition_penalty=PEN, sampling=SP, seeds=list(range(8)), logprobs=2, num_return_sequences=4)
    ids0, sc0 = m.generate_pages(pages, **kw)
    ids1, sc1 = m.generate_pages(pages, share_prompt=True, **kw)
    assert ids1 == ids0
    for p0, p1 in zip(sc0, sc1):
        for x, y in zip(p0, p1):
            assert np.array_equal(x.logprobs, y.logprobs) and np.array_equal(x.top_ids, y.top_ids) and np.array_equal(x.top_logprobs, y.top_logprobs)
    assert not m.kv(8).prefix_sharing and [m.kv(8).length(s) for s in range(8)] == [0] * 8      # the call left the cache without shares, in the copying mode
    bw = dict(max_new_tokens=10, eos_token_id=None, repetition_penalty=PEN, num_beams=4)
    assert m.generate_pages(pages, share_prompt=True, **bw) == m.generate_pages(pages, **bw)
    assert m.generate_pages(pages[:1], max_new_tokens=6, eos_token_id=None, share_prompt=True) == m.generate_pages(pages[:1], max_new_tokens=6, eos_token_id=None)
    with pytest.raises(NotImplementedError, match='drafts'):
        m.generate_pages(pages[:1], max_new_tokens=6, eos_token_id=None, share_prompt=True, drafts=[[1, 2]])


def test_chat_ocr_with_beams_and_share_prompt(llm):
    from chat_helpers import FakeTokenizer, SPECIALS
    m, prompt, other, second = llm
    tok = FakeTokenizer()
    m.img_context_token_id = SPECIALS['<IMG_CONTEXT>']
    m.aligned_token_id = SPECIALS['[UNUSED_TOKEN_140]']
    from PIL import Image
    page = Image.fromarray(np.random.default_rng(0).integers(0, 255, (448, 448, 3), dtype=np.uint8))      # one tile: a prompt of about 300 tokens
    boxes = [(10, 20, 110, 140), (200, 50, 420, 300), (300, 310, 380, 440)]
    gc = dict(max_new_tokens=8, num_beams=4, do_sample=False)
    want = m.chat_ocr(tok, None, page, 'what?', dict(gc), use_p=True, repetition_penalty=1.5, boxes=boxes)
    got = m.chat_ocr(tok, None, page, 'what?', dict(gc, share_prompt=True), use_p=True, repetition_penalty=1.5, boxes=boxes)
    assert got == want and isinstance(got, str)


def test_lifetime_rules_refuse_and_change_nothing(llm):
    from callireader_amd import _binding as B
    m, prompt, other, second = llm
    kv, eng = m.kv(64), m.engine
    fresh(kv, False)
    eng.prefill(kv, 0, prompt[:300], penalty=PEN)                                    # the source
    eng.prefill(kv, 7, other[:40], penalty=PEN)                                      # a bystander
    kv.fork_shared(0, [1, 2], 300)                                                   # 1 and 2 read rows [0, 256) of 0
    watch = [0, 1, 2, 3, 7]

    def snapshot():
        return state_of(kv, watch), rows_of(kv, 0, 250, 300, 7), rows_of(kv, 1, 250, 300, 7), rows_of(kv, 3, 0, 8)

    def refused(code, fn, *a, **k):
        before = snapshot()
        with pytest.raises(B.CalliReaderError, match=f'error {code}:'):
            fn(*a, **k)
        after = snapshot()
        assert before[0] == after[0] and all(torch.equal(x, y) for x, y in zip(before[1:], after[1:]))
    refused(STATE, kv.reset, 0)                                                      # the source, while it has sharers
    refused(STATE, kv.truncate, 0, 255)                                              # ... cut below the share
    refused(STATE, kv.truncate, 0, 0)
    refused(STATE, kv.truncate, 1, 255)                                              # a sharer below its share
    refused(STATE, kv.fork, 1, [3], 100)                                             # forks and a fan-out FROM a sharer
    refused(STATE, kv.fork_shared, 1, [3], 300)
    refused(STATE, kv.fork, 7, [0], 10)                                              # ... and INTO a source
    refused(STATE, kv.fork_shared, 7, [0], 10)
    refused(STATE, eng.prefill, kv, 1, other[:4], penalty=PEN)                       # a continued prefill of a sharer
    refused(STATE, eng.score_batch, kv, [1], [other[:4]], [[5, 6, 7, 8]])
    refused(STATE, eng.ground_batch, kv, [1], [other[:4]], [[5, 6, 7, 8]], [[(0, 4)]])
    refused(STATE, kv.beam_reorder, 1, [1, 0], 100)                                  # a re-order (of the two sharers) that would move shared rows
    refused(STATE, kv.set_prefix_sharing, True)                                      # the mode, while sequences hold tokens
    eng.decode(kv, [0, 1, 2], force_tokens=torch.tensor([5, 6, 7]), penalty=PEN)     # (an id to feed: the draft step needs one)
    refused(STATE, eng.decode_draft, kv, [1], [[3, 4]], penalty=PEN)
    kv.set_sampling(1, 0.7, 5, 0.8, 3)
    kv.truncate(2, 290)                                                              # a sharer cut above its share keeps it ...
    assert kv.length(2) == 290
    refused(STATE, kv.reset, 0)                                                      # ... so the source still cannot go
    kv.truncate(0, 256)                                                              # the source may be cut down to the share
    # reset order: the source is refused, the sharers go, then the source is accepted
    kv.reset(1)
    refused(STATE, kv.reset, 0)
    kv.reset(2)
    kv.reset(0)
    assert [kv.length(s) for s in (0, 1, 2)] == [0, 0, 0] and kv.length(7) == 40
    # fan-out from a sharer
    row = prefill_src(m, kv, prompt[:300], 9)
    kv.fork_shared(0, [4], 300)
    refused(STATE, kv.fanout, 4, [5], [7], row)
    kv.reset()                                                                       # everything at once always goes
    e4 = eng.kv_alloc(2, 320, dtype='e4m3')
    try:
        with pytest.raises(B.CalliReaderError, match=f'error {ARG}:'):
            e4.set_prefix_sharing(True)
        eng.prefill(e4, 0, prompt[:300], penalty=PEN)
        with pytest.raises(B.CalliReaderError, match=f'error {ARG}:'):
            e4.fork_shared(0, [1], 300)
    finally:
        e4.free()
    kv.set_prefix_sharing(True)                                                      # an empty cache takes the mode
    kv.set_prefix_sharing(False)

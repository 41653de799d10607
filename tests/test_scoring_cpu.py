"""Scoring a given text, host side (callireader_amd/scoring.py and the entry points' argument checks): no GPU."""
import math

import numpy as np
import pytest
import torch

from callireader_amd import scores as SC
from callireader_amd import scoring as S

from engine_stubs import EOS, make_model, make_session, ids_of, RoundTripTokenizer


def test_rows_and_targets_from_prompt_and_answer():
    p = S.plan(5, [11, 12, 13], eos_id=99)
    assert p.ids == [11, 12, 13, 99] and p.feed == [11, 12, 13] and p.targets == [-1, -1, -1, -1, 11, 12, 13, 99]
    assert len(p.targets) == 5 + len(p.feed)                                  # one target per row of prompt ++ embed(feed)
    q = S.plan(5, [11, 12, 13], eos_id=99, score_eos=False)
    assert q.ids == [11, 12, 13] and q.feed == [11, 12] and q.targets == [-1, -1, -1, -1, 11, 12, 13]
    assert S.plan(5, [11], eos_id=None).ids == [11]                           # no EOS id: nothing to append
    one = S.plan(1, [], eos_id=7)                                             # an empty answer still scores the stop
    assert one.ids == [7] and one.feed == [] and one.targets == [7]
    assert S.plan(3, torch.tensor([4, 5]), eos_id=np.int64(6)).targets == [-1, -1, 4, 5, 6]


def test_validation_errors():
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            S.plan(bad, [1], eos_id=2)
    with pytest.raises(ValueError):
        S.plan(3, [], eos_id=None)
    with pytest.raises(ValueError):
        S.plan(3, [], eos_id=5, score_eos=False)
    with pytest.raises(ValueError):
        S.plan(3, [-2], eos_id=5)
    with pytest.raises(ValueError):
        S.plan(3, [100], eos_id=5, vocab=100)
    assert S.plan(3, [99], eos_id=5, vocab=100).ids == [99, 5]
    for bad in (0, -1.5, float('inf'), float('nan'), True, '1.5'):
        with pytest.raises(ValueError):
            S.check_penalty(bad)
    assert S.check_penalty(1) == 1.0 and S.check_penalty(np.float32(1.5)) == 1.5
    with pytest.raises(ValueError):
        S.check_fits(10, 7, 16)
    S.check_fits(9, 7, 16)
    for bad in (-1, 9, 1.0, True):
        with pytest.raises(ValueError):
            S.top_n_of(bad)
    assert S.top_n_of(0) == 0 and S.top_n_of(8) == 8


def test_generation_keywords_are_refused():
    assert S.refuse_generation(None) == {} and S.refuse_generation(dict(max_new_tokens=5, num_beams=1, do_sample=False))['max_new_tokens'] == 5
    for gc in (dict(do_sample=True), dict(num_beams=4), dict(no_repeat_ngram_size=3), dict(bad_words_ids=[[5]]), dict(suppress_tokens=[1]),
               dict(min_new_tokens=2), dict(allowed_token_ids=[1, 2]), dict(draft_ids=[1])):
        with pytest.raises(ValueError):
            S.refuse_generation(gc)
    with pytest.raises(ValueError):
        S.refuse_generation({}, draft='align')


class Tok:
    all_special_ids = [92542]

    def convert_ids_to_tokens(self, ids):
        return ['<|im_end|>' if i == 92542 else f't{i}' for i in ids]

    def __call__(self, text, add_special_tokens=True):
        return {'input_ids': [int(c) for c in text.split()]}


def test_response_scores_with_total_logprob():
    ids = [11, 27, 13, 92542]
    lp = np.array([-0.5, -2.0, -0.25, -0.125], dtype=np.float32)
    ts = SC.TokenScores(lp, np.array([[i, i + 1] for i in ids]), np.stack([lp, lp - 1], 1))
    rs = S.response_scores(Tok(), ids, ts)
    assert rs.kept == [0, 1, 2] and rs.total_logprob == pytest.approx(-2.75) and rs.mean_logprob == pytest.approx(-2.75 / 3)
    assert rs.min_logprob == -2.0 and rs.min_index == 1 and rs.confidence == math.exp(rs.mean_logprob)
    assert rs.tokens[3].piece == '<|im_end|>' and rs.tokens[3].logprob == -0.125          # the stop is scored, outside the aggregates
    j = rs.to_json(total=True)
    assert j['total_logprob'] == rs.total_logprob and 'total_logprob' not in rs.to_json() and {k: v for k, v in j.items() if k != 'total_logprob'} == rs.to_json()
    none = S.response_scores(Tok(), [92542], SC.TokenScores(lp[:1], np.zeros((1, 0)), np.zeros((1, 0))))      # top_logprobs=0: no alternatives
    assert none.kept == [] and math.isnan(none.total_logprob) and none.tokens[0].top == []
    assert S.answer_to_ids(Tok(), '5 6 7') == [5, 6, 7] and S.answer_to_ids(Tok(), (5, np.int64(6))) == [5, 6]


def test_entry_points_refuse_what_steers_a_generation():
    """model.score_ocr / score_pages and PageSession.score on the stubs: every refusal comes before any engine call"""
    m = make_model()
    tok = RoundTripTokenizer()
    for kw in (dict(generation_config=dict(do_sample=True)), dict(generation_config=dict(num_beams=2)), dict(generation_config=dict(no_repeat_ngram_size=2)),
               dict(draft='align'), dict(draft=[1, 2]), dict(top_logprobs=9), dict(repetition_penalty=0)):
        with pytest.raises(ValueError):
            m.score_ocr(tok, None, None, 'q', 'abc', **kw)
    assert m.engine.log == []
    emb = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        m.score_pages([emb], [[1], [2]])
    with pytest.raises(ValueError):
        m.score_pages([emb], [[1]], logprobs=9)
    with pytest.raises(ValueError):
        m.score_pages([emb], [[1]], repetition_penalty=-1)
    m8 = make_model(kv_cache_dtype='e4m3')
    with pytest.raises(NotImplementedError):
        m8.score_pages([emb], [[1]])
    assert m.engine.log == [] and m8.engine.log == []

    sess, eng = make_session(max_branches=2)
    for kw in (dict(generation_config=dict(do_sample=True)), dict(generation_config=dict(num_beams=3)), dict(generation_config=dict(min_new_tokens=1)),
               dict(draft='previous'), dict(top_logprobs=-1), dict(repetition_penalty=float('nan'))):
        with pytest.raises(ValueError):
            sess.score('q', ['ab'], **kw)
    with pytest.raises(ValueError):
        sess.score('q', ['a', 'b', 'c'])                                       # more candidates than branches
    with pytest.raises(ValueError):
        sess.score('q', [])
    assert eng.log == [] and sess.cached_ids == []


def test_session_score_forks_and_leaves_the_trunk():
    """PageSession.score on the stubs: one fork for all candidates at the prefix the prompt shares with the trunk, one score_batch with the tail rows, the
    answer's rows and targets that score the answer and the stop; the trunk's ids and length stay"""
    sess, eng = make_session(max_branches=2)
    calls = []

    def score_batch(kv, seqs, rows, targets, penalty=1.0, top_n=0):
        calls.append((list(seqs), [r[:, 0].long().tolist() for r in rows], [list(t) for t in targets], penalty, top_n))
        return [SC.TokenScores(np.full(sum(1 for x in t if x >= 0), -1.0, np.float32), np.zeros((sum(1 for x in t if x >= 0), 0)),
                               np.zeros((sum(1 for x in t if x >= 0), 0))) for t in targets]
    eng.score_batch = score_batch
    sess.tokenizer.all_special_ids = [EOS]
    sess.tokenizer.convert_ids_to_tokens = lambda ids: [str(i) for i in ids]
    eng.script[0] = ids_of('ok') + [EOS]
    sess.chat_ocr('what?', dict(max_new_tokens=8))                              # a first turn fills the trunk
    cached, length = list(sess.cached_ids), sess.kv.length(0)
    eng.log.clear()
    out = sess.score('what?', ['ok', 'no!'], repetition_penalty=1.5, top_logprobs=0)
    assert sess.cached_ids == cached and sess.kv.length(0) == length
    forks = [e for e in eng.log if e[0] == 'fork']
    assert len(forks) == 1 and forks[0][1] == 0 and forks[0][2] == [1, 2]
    p = forks[0][3]
    (seqs, rows, targets, penalty, top_n), = calls
    assert seqs == [1, 2] and penalty == 1.5 and top_n == 0
    for r, t, text in zip(rows, targets, ('ok', 'no!')):
        y = ids_of(text) + [EOS]
        assert len(r) == len(t) and r[len(r) - len(y) + 1:] == y[:-1] and t[-len(y):] == y and all(x == -1 for x in t[:-len(y)])
        assert len(r) - len(y) + 1 == 1 and r[0] == cached[p]                          # the trunk holds the whole prompt: rolled back one row, fed again
    assert [len(o.tokens) for o in out] == [3, 4] and out[0].total_logprob == pytest.approx(-2.0) and out[1].total_logprob == pytest.approx(-3.0)

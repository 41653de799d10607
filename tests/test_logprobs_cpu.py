"""Token scores on the host (callireader_amd/scores.py and what passes them through): keyword validation, cutting and aggregation, ContinuousPipeline
handing `logprobs` to the cache and the scores back with the ids (a fake engine, as tests/test_continuous_cpu.py), the sharded entry's refusal, the CLI flag."""
import math

import numpy as np
import pytest

import test_continuous_cpu as T
from callireader_amd import scores as SC
from callireader_amd.continuous import ContinuousPipeline


def test_parse_keywords():
    assert SC.parse({}) == 0 and SC.parse({'output_scores': True}) == 0 and SC.parse({'top_logprobs': 3}) == 0
    assert SC.parse({'return_dict_in_generate': True}) == 0
    assert SC.parse({'return_dict_in_generate': True, 'output_scores': True}) == 1
    assert SC.parse({'return_dict_in_generate': True, 'output_scores': True, 'top_logprobs': 8}) == 8
    for bad in (0, 9, -1, 2.5, True, '3'):
        with pytest.raises(ValueError):
            SC.parse({'return_dict_in_generate': True, 'output_scores': True, 'top_logprobs': bad})
    for k in ('output_logits', 'output_attentions', 'output_hidden_states'):
        with pytest.raises(NotImplementedError):
            SC.parse({'return_dict_in_generate': True, 'output_scores': True, k: True})
        assert SC.parse({k: True}) == 0                                   # ignored without return_dict_in_generate, as before


def test_per_page():
    assert SC.per_page(0, 3) == [0, 0, 0] and SC.per_page(5, 2) == [5, 5] and SC.per_page([0, 8, 1], 3) == [0, 8, 1] and SC.per_page(None, 1) == [0]
    for bad in (9, -1, [1, 2], [0, 9, 0]):
        with pytest.raises(ValueError):
            SC.per_page(bad, 3)


def scores_of(ids, n=3):
    """Deterministic scores for a list of ids: logprob -(id % 10) / 10 - 0.05, alternatives id, id + 1, ..."""
    lp = np.array([-(i % 10) / 10 - 0.05 for i in ids], dtype=np.float32)
    ti = np.array([[i + k for k in range(n)] for i in ids], dtype=np.int32).reshape(len(ids), n)
    tl = np.array([[l - k for k in range(n)] for l in lp], dtype=np.float32).reshape(len(ids), n)
    return lp, ti, tl


def test_token_scores_cut():
    ts = SC.TokenScores(*scores_of(list(range(20, 30))))
    c = ts.cut(4)
    assert len(c) == 4 and c.top_ids.shape == (4, 3) and c.top_logprobs.shape == (4, 3) and np.array_equal(c.logprobs, ts.logprobs[:4])
    with pytest.raises(ValueError):
        ts.cut(11)

    class KV:
        def logprobs(self, seq, max_tokens=4096):
            return scores_of(list(range(12)))
    assert len(SC.TokenScores.read(KV(), 0, 7)) == 7


class Tok:
    all_special_ids = [92542]

    def convert_ids_to_tokens(self, ids):
        return ['<|im_end|>' if i == 92542 else f't{i}' for i in ids]


def test_response_scores_aggregate_over_kept_tokens():
    ids = [11, 27, 13, 92542, 99]                                         # EOS kept in tokens, outside the aggregates; the caller has cut the ids
    full = ids + [5, 6]                                                   # speculative steps past the stop are dropped by the cut
    rs = SC.ResponseScores.build(Tok(), ids, SC.TokenScores(*scores_of(full)))
    assert [t.piece for t in rs.tokens] == ['t11', 't27', 't13', '<|im_end|>', 't99'] and rs.kept == [0, 1, 2, 4] and rs.pieces() == ['t11', 't27', 't13', 't99']
    lps = [rs.tokens[t].logprob for t in rs.kept]
    assert rs.mean_logprob == pytest.approx(sum(lps) / 4) and rs.confidence == math.exp(rs.mean_logprob)
    assert rs.min_logprob == min(lps) and rs.min_index == 4 and rs.tokens[4].id == 99
    assert rs.tokens[1].top == [(27, 't27', pytest.approx(-0.75)), (28, 't28', pytest.approx(-1.75)), (29, 't29', pytest.approx(-2.75))]
    j = rs.to_json()
    assert j['tokens'][3] == '<|im_end|>' and len(j['alternatives'][0]) == 3 and j['confidence'] == rs.confidence
    assert rs.summary_line().startswith('confidence ') and rs.summary_line().endswith('at token 4 (t99)')
    empty = SC.ResponseScores.build(Tok(), [92542], SC.TokenScores(*scores_of([92542])))
    assert empty.kept == [] and math.isnan(empty.confidence) and empty.min_index == -1


class ScoredKV(T.FakeKV):
    """FakeKV with the device semantics of cr_kv_set_logprobs: off after a reset, scores for every generated id while on."""

    def reset(self, seq=-1):
        super().reset(seq)
        if seq < 0:
            self.lpn = {}
        for s in (range(self.n_seqs) if seq < 0 else [seq]):
            self.lpn[s] = 0

    def set_logprobs(self, seq, top_n):
        assert not self.ids[seq], 'scores are switched on after the reset and before the prefill'
        self.lpn[seq] = top_n

    def logprobs(self, seq, max_tokens=4096):
        assert self.lpn[seq] > 0, 'CR_ERR_STATE: scores are off'
        with self.lock:
            return scores_of(self.ids[seq][:max_tokens], self.lpn[seq])


def test_continuous_pipeline_passes_logprobs_through():
    m = T.FakeModel(max_rows=2)
    m.engine.kv_alloc = lambda n, mt: m.engine.kvs.append(ScoredKV(n, mt)) or m.engine.kvs[-1]
    pipe = ContinuousPipeline(m, slots=2, max_new_tokens=12, eos_token_id=7, admit_group=1, spare=1, ops=T.FakeOps())
    try:
        pages = [T.Page(s) for s in range(9)]
        lpn = [0, 3, 0, 8, 1, 0, 2, 0, 5]                                 # nine pages through three sequences: every slot is reused
        tickets = [pipe.submit(p, logprobs=n) for p, n in zip(pages, lpn)]
        got = dict(pipe.results())
        for t, p, n in zip(tickets, pages, lpn):
            want = T.reference(p, 12, 7)
            if n == 0:
                assert got[t] == want                                     # exactly what it was
            else:
                ids, ts = got[t]
                assert ids == want and isinstance(ts, SC.TokenScores) and len(ts) == len(ids) and ts.top_ids.shape == (len(ids), n)
                assert ts.top_ids[:, 0].tolist() == ids
        with pytest.raises(ValueError):
            pipe.submit(pages[0], logprobs=9)
    finally:
        pipe.close()


def test_sharded_entry_refuses_scores():
    from callireader_amd.parallel import chat_ocr_pages_sharded
    with pytest.raises(NotImplementedError, match='token scores'):
        chat_ocr_pages_sharded(None, None, None, [], 'q', dict(max_new_tokens=4), return_scores=True)


def test_cli_flag():
    from callireader_amd import inference as I
    p = I.build_parser()
    assert p.parse_args(['--tgt', 'x']).scores == 0 and p.parse_args(['--tgt', 'x', '--scores']).scores == 1
    assert p.parse_args(['--tgt', 'x', '--scores', '8']).scores == 8
    with pytest.raises(SystemExit):
        p.parse_args(['--tgt', 'x', '--scores', '9'])
    assert I.scores_name('results/recognition.json') == 'results/recognition.scores.json'
    assert I.scores_name('results/run_result.json') == 'results/run_result.scores.json'

"""Scoring at the chat and command-line level: model.score_ocr on the synthetic page of tests/chat_helpers.py against the scores chat_ocr recorded for the
ids it generated, PageSession.score on the same page, and `inference.py --score_answer` on a checkpoint from disk.

Bound of the comparison with chat_ocr(return_scores=True): two bf16 paths -- the decode steps that recorded the scores and the prefill-shaped pass that
scores the same ids -- are each within 2 * max(penalty, 1) * ATOL of the oracle's log-probability (tests/test_gpu_score.py), hence within
4 * max(penalty, 1) * ATOL of each other."""
import json
import math
import os

import numpy as np
import pytest
from PIL import Image

from callireader_amd.config import ModelDims
from callireader_amd import synthetic

from chat_helpers import SPECIALS, FakeTokenizer
from decode_checks import ATOL
from test_gpu_boundary import ckpt  # noqa: F401  (module fixture: a checkpoint on disk)

pytestmark = pytest.mark.gpu

PENALTY = 1.5


class Tok(FakeTokenizer):
    all_special_ids = sorted(SPECIALS.values())

    def convert_ids_to_tokens(self, ids):
        return [('<|im_end|>' if int(t) == 8992 else str(int(t))) for t in ids]

    def batch_decode(self, out, skip_special_tokens=True):
        return [' '.join(self.convert_ids_to_tokens([t])[0] for t in row if not (skip_special_tokens and int(t) in self.all_special_ids)) for row in out]


@pytest.fixture(scope='module')
def setup():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=9000)
    model = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=0), dims, max_tokens=4096)
    model.aligned_token_id = SPECIALS['[UNUSED_TOKEN_140]']
    img = Image.fromarray(np.random.default_rng(0).integers(0, 255, (500, 640, 3), dtype=np.uint8))
    boxes = [(10, 20, 110, 140), (200, 50, 420, 300), (300, 310, 380, 480)]
    yield dict(model=model, img=img, boxes=boxes, tok=Tok())
    model.close()


def close_to(got, want, what):
    bound = 4 * max(PENALTY, 1.0) * ATOL
    assert [t.id for t in got.tokens] == [t.id for t in want.tokens] and got.kept == want.kept and got.pieces() == want.pieces(), what
    d = max(abs(a.logprob - b.logprob) for a, b in zip(got.tokens, want.tokens))
    print(f'{what}: {len(got.tokens)} tokens, max |logprob difference| {d:.4f} (bound {bound:.2f})')
    assert d <= bound, (what, d)


def test_score_ocr_agrees_with_the_scores_chat_ocr_recorded(setup):
    m, tok = setup['model'], setup['tok']
    gen = dict(num_beams=1, max_new_tokens=12, do_sample=False)
    resp, rec = m.chat_ocr(tok, None, setup['img'], 'what?', gen, use_p=True, repetition_penalty=PENALTY, boxes=setup['boxes'], return_scores=3)
    ids = [t.id for t in rec.tokens]
    got = m.score_ocr(tok, None, setup['img'], 'what?', ids, gen, repetition_penalty=PENALTY, top_logprobs=3, boxes=setup['boxes'], score_eos=False)
    close_to(got, rec, 'score_ocr')
    assert all(len(t.top) == 3 for t in got.tokens)
    lps = [got.tokens[t].logprob for t in got.kept]
    assert got.total_logprob == pytest.approx(sum(lps)) and got.confidence == math.exp(got.mean_logprob)
    # the stop is scored by default: one more token, the aggregates unchanged
    if ids[-1] != SPECIALS['<|im_end|>']:
        more = m.score_ocr(tok, None, setup['img'], 'what?', ids, None, repetition_penalty=PENALTY, top_logprobs=0, boxes=setup['boxes'])
        assert [t.id for t in more.tokens] == ids + [SPECIALS['<|im_end|>']] and more.kept == got.kept
        # (one more row in the pass: the earlier rows keep their values up to the attention's wave-wide rescale vote, i.e. inside the same bound)
        assert max(abs(a.logprob - b.logprob) for a, b in zip(more.tokens, got.tokens)) <= 4 * max(PENALTY, 1.0) * ATOL and more.tokens[-1].top == []
    with pytest.raises(ValueError):
        m.score_ocr(tok, None, setup['img'], 'what?', ids, dict(do_sample=True), boxes=setup['boxes'])


def test_session_score_leaves_the_trunk(setup):
    m, tok = setup['model'], setup['tok']
    gen = dict(num_beams=1, max_new_tokens=8, do_sample=False)
    with m.open_page(tok, None, setup['img'], boxes=setup['boxes'], max_branches=3) as s:
        resp, rec = s.chat_ocr('what?', gen, repetition_penalty=PENALTY, return_scores=True)
        ids = [t.id for t in rec.tokens]
        cached, length, gen_ids = list(s.cached_ids), s.kv.length(0), s.kv.generated(0)
        other = [i + 1 for i in ids]
        a, b, c = s.score('what?', [ids, other, ids[:3]], repetition_penalty=PENALTY, score_eos=False)
        assert s.cached_ids == cached and s.kv.length(0) == length and s.kv.generated(0) == gen_ids
        close_to(a, rec, 'session.score')
        assert [t.id for t in b.tokens] == other and len(c.tokens) == 3
        assert a.total_logprob > b.total_logprob                                           # what the model said outranks what it did not
        again = s.score('what?', [other], repetition_penalty=PENALTY, score_eos=False)[0]    # alone, in another branch
        assert [t.logprob for t in again.tokens] == [t.logprob for t in b.tokens]


def test_cli_score_answer(ckpt, tmp_path, monkeypatch, capsys):
    from callireader_amd import inference as inf
    img = Image.fromarray(np.random.default_rng(3).integers(0, 255, (500, 640, 3), dtype=np.uint8))
    path = str(tmp_path / 'page.jpg')
    img.save(path, quality=92)
    raw = [[300, 310, 380, 480], [10, 20, 110, 140], [200, 50, 420, 300]]
    shapes = [{'points': [[b[0] / 640 * 0.5, b[1] / 500 * 0.5], [b[2] / 640 * 0.5, b[3] / 500 * 0.5]]} for b in raw]
    json.dump({'imageHeight': 500, 'imageWidth': 640, 'shapes': shapes}, open(str(tmp_path / 'page.json'), 'w'))
    monkeypatch.chdir(tmp_path)
    common = ['--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '4', '--tgt', path, '--repetition_penalty', '1.2']
    inf.main(common)
    before = capsys.readouterr().out
    inf.main(common + ['--score_answer', 'abc def', '--scores', '2'])
    after = capsys.readouterr().out
    # the existing output is unchanged up to the --scores line; the scoring lines follow it
    assert after.startswith(before) and before.strip()
    extra = after[len(before):].strip().splitlines()
    assert extra[0].startswith('confidence ') and extra[1] == 'Scored: abc def' and extra[2].startswith('confidence ') and extra[3].startswith('total logprob ')
    doc = json.load(open(tmp_path / 'results' / 'recognition.answer_scores.json', encoding='utf-8'))
    sc = doc['scores']
    assert doc['imagePath'] == path and doc['answer'] == 'abc def' and len(sc['ids']) == len(sc['logprobs']) >= 2
    assert all(len(a) == 2 for a in sc['alternatives']) and all(lp <= 0 for lp in sc['logprobs'])
    kept = [sc['logprobs'][t] for t in sc['kept']]
    assert sc['total_logprob'] == pytest.approx(sum(kept)) and sc['mean_logprob'] == pytest.approx(sum(kept) / len(kept))
    with pytest.raises(ValueError):
        inf.main(common + ['--score_answer', 'abc', '--do_sample'])

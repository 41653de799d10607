"""num_return_sequences at the chat and command-line level: chat_ocr with n = 3 on the synthetic page of tests/test_gpu_score_chat.py -- three responses
and three ResponseScores from one call, each the response of a lone chat_ocr call made with that sample's seed -- and `inference.py
--num_return_sequences 2` on a checkpoint from disk."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from callireader_amd import sampling as S
from callireader_amd.config import ModelDims
from callireader_amd import synthetic

from chat_helpers import SPECIALS
from test_gpu_boundary import _write_folder, ckpt  # noqa: F401  (module fixture: a checkpoint on disk)
from test_gpu_score_chat import Tok

pytestmark = pytest.mark.gpu


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


def test_chat_ocr_returns_n_responses(setup, monkeypatch):
    import callireader_amd.modeling_internvl_chat as M
    m, tok = setup['model'], setup['tok']
    gen = dict(num_beams=1, max_new_tokens=12, do_sample=True, temperature=0.9, top_k=40)
    kw = dict(use_p=True, repetition_penalty=1.5, boxes=setup['boxes'])
    torch.manual_seed(21)
    resp, hist, scs = m.chat_ocr(tok, None, setup['img'], 'what?', dict(gen, num_return_sequences=3), return_history=True, return_scores=True, **kw)
    assert isinstance(resp, list) and len(resp) == 3 and all(isinstance(r, str) for r in resp) and len(scs) == 3
    assert hist[-1][1] == resp[0]                                                   # the history holds sample 0's answer
    for sc in scs:
        lps = [sc.tokens[t].logprob for t in sc.kept]
        assert sc.total_logprob == pytest.approx(sum(lps)) and len(sc.tokens) <= 12 and all(len(t.top) == 1 for t in sc.tokens)
    assert max(range(3), key=lambda j: scs[j].total_logprob) in (0, 1, 2)          # best-of-n is one max()
    # the three responses are those of three lone chat_ocr calls made with the three seeds
    torch.manual_seed(21)
    seeds = S.page_seeds(3)
    for j in range(3):
        monkeypatch.setattr(M, 'page_seeds', lambda n, base=None, sd=seeds[j]: [sd] * n)
        r, sc = m.chat_ocr(tok, None, setup['img'], 'what?', gen, return_scores=True, **kw)
        assert r == resp[j] and sc.to_json() == scs[j].to_json() and sc.total_logprob == scs[j].total_logprob, j
    monkeypatch.undo()
    plain = m.chat_ocr(tok, None, setup['img'], 'what?', dict(gen, num_return_sequences=3), **kw)
    assert isinstance(plain, list) and len(plain) == 3
    with pytest.raises(ValueError, match='Greedy methods without beam search'):
        m.chat_ocr(tok, None, setup['img'], 'what?', dict(num_beams=1, max_new_tokens=4, do_sample=False, num_return_sequences=3), **kw)
    with m.open_page(tok, None, setup['img'], boxes=setup['boxes']) as s:
        with pytest.raises(NotImplementedError, match='num_return_sequences'):
            s.chat_ocr('what?', dict(gen, num_return_sequences=2))


def test_cli_num_return_sequences(ckpt, tmp_path, monkeypatch, capsys):
    from callireader_amd import inference as inf
    d = str(tmp_path / 'pages')
    paths, bad = _write_folder(None, d, n_good=3)
    raw = [[300, 310, 380, 480], [10, 20, 110, 140], [200, 50, 420, 300]]
    for p in paths:
        if p == bad:
            continue
        w, h = Image.open(p).size
        shapes = [{'points': [[b[0] / w * 0.5, b[1] / h * 0.5], [b[2] / w * 0.5, b[3] / h * 0.5]]} for b in raw]
        json.dump({'imageHeight': h, 'imageWidth': w, 'shapes': shapes}, open(os.path.splitext(p)[0] + '.json', 'w'))
    monkeypatch.chdir(tmp_path)
    common = ['--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '6', '--do_sample', '--seed', '3']
    inf.main(common + ['--tgt', d, '--batch_pages', '8', '--save_name', 'two.json', '--num_return_sequences', '2', '--scores'])
    res = json.load(open(tmp_path / 'results' / 'two.json', encoding='utf-8'))
    assert [e['imagePath'] for e in res] == paths
    for e in res:
        if e['imagePath'] == bad:
            assert e['response'] == 'ERROR!'
        else:
            assert isinstance(e['response'], list) and len(e['response']) == 2 and all(isinstance(r, str) for r in e['response'])
    doc = json.load(open(tmp_path / 'results' / 'two.scores.json', encoding='utf-8'))
    assert all((e['scores'] is None) if e['imagePath'] == bad else (len(e['scores']) == 2 and 'total_logprob' in e['scores'][0]) for e in doc)
    inf.main(common + ['--tgt', d, '--batch_pages', '8', '--save_name', 'one.json'])
    one = json.load(open(tmp_path / 'results' / 'one.json', encoding='utf-8'))
    assert all(isinstance(e['response'], str) for e in one)                         # the JSON gains a list only when N > 1
    good = next(p for p in paths if p != bad)
    capsys.readouterr()
    inf.main(common + ['--tgt', good, '--num_return_sequences', '2', '--scores'])
    lines = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith('Assistant[') for ln in lines) == 2 and sum(ln.strip().startswith('total logprob ') for ln in lines) == 2

"""Grounding at the chat and command-line level: model.ground_ocr / ground_pages and PageSession.ground on the synthetic page of tests/chat_helpers.py (the
small chat set-up of tests/test_gpu_score_chat.py), and `inference.py --ground` on a checkpoint from disk."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from callireader_amd.config import ModelDims
from callireader_amd import grounding as G
from callireader_amd import synthetic

from chat_helpers import SPECIALS
from test_gpu_boundary import ckpt  # noqa: F401  (module fixture: a checkpoint on disk)
from test_gpu_score_chat import Tok

pytestmark = pytest.mark.gpu

PENALTY = 1.5
GEN = dict(num_beams=1, max_new_tokens=12, do_sample=False)


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


def test_ground_ocr_grounds_what_chat_ocr_answers(setup):
    m, tok, img, boxes = setup['model'], setup['tok'], setup['img'], setup['boxes']
    want = m.chat_ocr(tok, None, img, 'what?', dict(GEN), use_p=True, repetition_penalty=PENALTY, boxes=boxes)
    resp, g = m.ground_ocr(tok, None, img, 'what?', None, dict(GEN), repetition_penalty=PENALTY, boxes=boxes)
    assert resp == want
    ids = [t.id for t in g.tokens]
    assert 1 <= len(ids) <= 12 and g.boxes == [list(b) for b in boxes] and g.mass.shape == (len(ids), 3) and g.layers == (0, 1)
    assert all(0 <= t.box < 3 and 0 < t.box_mass <= 1 and 0 <= t.elsewhere < 1 for t in g.tokens)
    assert all(b in g.boxes for _, b, _ in g.pairs()) and [p for p, _, _ in g.pairs()] == [t.piece for t in g.tokens if t.id not in tok.all_special_ids]
    # the same prompt, ids and spans through ground_pages: one pass over prompt ++ answer instead of a continued prefill over the cached prompt
    page, px = m._open_page(img)
    out_tokens, _ = m.calli_align(page, None, boxes=boxes)
    _, _, _, inputs, gc = m._ocr_prompt(tok, 'what?', None, len(px), out_tokens, True, None, {}, False)
    pids = inputs['input_ids'].reshape(-1)
    spans = G.spans_of(pids, m.aligned_token_id)
    assert spans == g.spans and len(spans) == 3 and all(e - s == 3 for s, e in spans)
    prompt = m.engine.embed_splice(pids, m.extract_feature(px), out_tokens, img_id=m.img_context_token_id, ref_id=m.aligned_token_id)
    toks, ms, ts = m.ground_pages([prompt], [ids], [spans], repetition_penalty=PENALTY, score_eos=False)
    assert toks[0] == ids and ts[0] is None and torch.equal(ms[0], torch.from_numpy(g.mass))
    # and the answer brought back by the caller: the same bits, with the scores of the same pass when asked for
    resp2, g2 = m.ground_ocr(tok, None, img, 'what?', ids, None, repetition_penalty=PENALTY, boxes=boxes, score_eos=False, top_logprobs=2)
    assert resp2 == want and np.array_equal(g2.mass, g.mass) and [t.box for t in g2.tokens] == [t.box for t in g.tokens]
    assert [t.id for t in g2.scores.tokens] == ids and all(len(t.top) == 2 for t in g2.scores.tokens)
    with pytest.raises(ValueError):
        m.ground_ocr(tok, None, img, 'what?', None, dict(do_sample=True), boxes=boxes)


def test_session_ground_leaves_the_trunk(setup):
    m, tok, img, boxes = setup['model'], setup['tok'], setup['img'], setup['boxes']
    gen = dict(GEN, max_new_tokens=8)

    def turns(ground):
        with m.open_page(tok, None, img, boxes=boxes, max_branches=1) as s:
            r1, hist = s.chat_ocr('what?', dict(gen), repetition_penalty=PENALTY, return_history=True)
            got = None
            if ground:
                cached, length, gen_ids = list(s.cached_ids), s.kv.length(0), s.kv.generated(0)
                got = s.ground('what?', repetition_penalty=PENALTY, generation_config=dict(gen)), s.ground('what?', s.answer_ids, score_eos=False)
                assert s.cached_ids == cached and s.kv.length(0) == length and s.kv.generated(0) == gen_ids
            r2 = s.chat_ocr('and the second line?', dict(gen), history=hist, repetition_penalty=PENALTY)
            return r1, r2, list(s.answer_ids), got
    a1, a2, ids_a, _ = turns(False)
    b1, b2, ids_b, ((resp, g), (_, g_given)) = turns(True)
    assert (a1, a2, ids_a) == (b1, b2, ids_b)
    assert g.boxes == [list(b) for b in boxes] and len(g.tokens) >= 1 and all(0 <= t.box < 3 for t in g.tokens) and isinstance(resp, str)
    assert g_given.mass.shape[1] == 3 and len(g_given.tokens) >= 1


def test_cli_ground(ckpt, tmp_path, monkeypatch, capsys):
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
    inf.main(common + ['--ground'])
    after = capsys.readouterr().out
    assert after.startswith(before) and before.strip()              # the recognition is printed as without the flag; the grounding lines follow it
    lines = after[len(before):].strip().splitlines()
    doc = json.load(open(tmp_path / 'results' / 'recognition.grounding.json', encoding='utf-8'))
    page_boxes = [[int(v) for v in b[:4]] for b in inf.boxes_for(path)]
    gr = doc['grounding']
    assert doc['imagePath'] == path and before.rstrip('\n').endswith('Assistant: ' + doc['response'])
    assert len(gr) == len(lines) and all(set(e) == {'piece', 'box', 'mass'} for e in gr)      # one entry per decoded piece
    assert all(e['box'] in page_boxes and 0 < e['mass'] <= 1 for e in gr)
    inf.main(common + ['--ground_answer', 'abc def'])
    out = capsys.readouterr().out
    doc = json.load(open(tmp_path / 'results' / 'recognition.grounding.json', encoding='utf-8'))
    assert 'Grounded: abc def' in out and doc['response'] == 'abc def' and len(doc['grounding']) >= 2 and all(e['box'] in page_boxes for e in doc['grounding'])
    with pytest.raises(ValueError):
        inf.main(common + ['--ground', '--do_sample'])

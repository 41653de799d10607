"""Token scores at the chat and command-line level, on a checkpoint from disk (test_gpu_boundary.py's checkpoint, trained sentencepiece tokenizer, detector
object and page folder): chat_ocr(..., return_scores=) with the real tokenizer, and `inference.py --scores` in single-image and folder mode -- the results
JSON byte-equal to a run without the flag, the scores JSON beside it and consistent."""
import json
import math
import os

import pytest
from PIL import Image

from test_gpu_boundary import YoloLike, _write_folder, ckpt, setup  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu


def test_chat_ocr_returns_response_scores(setup):
    m, tok, img = setup['model'], setup['tok'], setup['img']
    det = YoloLike(setup['raw'])
    gen = dict(num_beams=1, max_new_tokens=12, do_sample=False)
    q = '这幅书法作品内容是什么？'
    plain = m.chat_ocr(tok, det, img, q, gen, repetition_penalty=1.2)
    resp, sc = m.chat_ocr(tok, det, img, q, gen, repetition_penalty=1.2, return_scores=5)
    assert resp == plain
    kept_ids = [sc.tokens[t].id for t in sc.kept]
    assert tok.convert_tokens_to_ids(sc.pieces()) == kept_ids                      # the pieces are the response's tokens ...
    assert tok.decode(kept_ids, skip_special_tokens=True).split('<|im_end|>')[0].strip() == resp      # ... and joined they reproduce it
    assert len(sc.tokens) <= 12 and all(len(tk.top) == 5 and tk.top[0][0] == tk.id and tk.top[0][2] == tk.logprob for tk in sc.tokens)
    lps = [sc.tokens[t].logprob for t in sc.kept]
    assert sc.mean_logprob == pytest.approx(sum(lps) / len(lps)) and sc.confidence == math.exp(sc.mean_logprob)
    assert sc.min_logprob == min(lps) and all(lp <= 0 for lp in lps)
    r2, hist, sc2 = m.chat_ocr(tok, det, img, q, gen, repetition_penalty=1.2, return_history=True, return_scores=True)
    assert r2 == plain and hist[-1][1] == plain and [tk.id for tk in sc2.tokens] == [tk.id for tk in sc.tokens] and len(sc2.tokens[0].top) == 1
    # the page-list form: one ResponseScores per page, the same numbers as the page's own call
    both, scs = m.chat_ocr_pages(tok, det, [img, img], q, gen, repetition_penalty=1.2, return_scores=5)
    assert both == [plain, plain] and all(s.to_json() == sc.to_json() for s in scs)


def test_cli_scores(ckpt, tmp_path, monkeypatch, capsys):
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
    common = ['--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '8']

    def run(name, *extra):
        inf.main(common + ['--tgt', d, '--batch_pages', '3', '--save_name', name] + list(extra))
        return open(tmp_path / 'results' / name, 'rb').read()
    plain = run('plain.json')
    assert not os.path.exists(tmp_path / 'results' / 'plain.scores.json')
    for name, extra in (('scored.json', ['--scores', '3']), ('cont.json', ['--scores', '3', '--continuous']), ('serial.json', ['--scores', '3', '--batch_pages', '1'])):
        assert run(name, *extra) == plain, name               # the results JSON does not change, byte for byte
    res = json.loads(plain.decode('utf-8'))
    docs = [json.load(open(tmp_path / 'results' / (n + '.scores.json'), encoding='utf-8')) for n in ('scored', 'cont', 'serial')]
    assert docs[0] == docs[1] == docs[2]                                            # a page's scores do not depend on the path it took
    assert [e['imagePath'] for e in docs[0]] == paths
    for e, r in zip(docs[0], res):
        s = e['scores']
        if r['response'] == 'ERROR!':
            assert s is None and e['imagePath'] == bad
            continue
        T = len(s['tokens'])
        assert 1 <= T <= 8 and len(s['ids']) == len(s['logprobs']) == len(s['alternatives']) == T
        assert all(len(a) == 3 and a[0]['id'] == i and a[0]['logprob'] == lp for a, i, lp in zip(s['alternatives'], s['ids'], s['logprobs']))
        kept = [s['logprobs'][t] for t in s['kept']]
        assert s['mean_logprob'] == pytest.approx(sum(kept) / len(kept)) and s['confidence'] == pytest.approx(math.exp(s['mean_logprob']))
        assert s['min_logprob'] == min(kept) and s['kept'][kept.index(min(kept))] == s['min_index']
    # single image: the response as always, then one line
    good = next(p for p in paths if p != bad)
    capsys.readouterr()
    inf.main(common + ['--tgt', good])
    before = capsys.readouterr().out
    inf.main(common + ['--tgt', good, '--scores'])
    after = capsys.readouterr().out
    assert after.startswith(before) and before.strip()
    extra = after[len(before):].strip().splitlines()
    assert len(extra) == 1 and extra[0].startswith('confidence ') and ' min ' in extra[0] and ' at token ' in extra[0]

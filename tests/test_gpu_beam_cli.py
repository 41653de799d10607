"""Beam search at the public surface, on a checkpoint from disk (test_gpu_boundary.py's checkpoint, tokenizer and page folder): chat_ocr(num_beams=3)
gives a page the response chat_ocr_pages gives it inside a batch, `inference.py --num_beams 3` writes the same JSON twice, and without the flag the JSON is
the greedy one byte for byte."""
import json
import os

import pytest
from PIL import Image

from test_gpu_boundary import YoloLike, _write_folder, ckpt, setup  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu


def test_chat_ocr_with_beams_equals_chat_ocr_pages(setup, tmp_path):
    m, tok = setup['model'], setup['tok']
    paths, bad = _write_folder(setup, str(tmp_path))
    good = [p for p in paths if p != bad][:3]
    det = YoloLike(setup['raw'][:3])
    gen = dict(num_beams=3, max_new_tokens=7, do_sample=False, length_penalty=1.0, early_stopping=False)
    q = '读出图中所有文字。'
    want = [m.chat_ocr(tok, det, p, q, gen, repetition_penalty=1.1) for p in good]
    assert m.chat_ocr_pages(tok, det, good, q, gen, repetition_penalty=1.1) == want
    assert gen == dict(num_beams=3, max_new_tokens=7, do_sample=False, length_penalty=1.0, early_stopping=False)      # the caller's dict is not mutated
    with pytest.raises(NotImplementedError):
        m.chat_ocr(tok, det, good[0], q, gen, repetition_penalty=1.1, return_scores=True)


def test_inference_cli_with_and_without_beams(ckpt, tmp_path, monkeypatch, capsys):
    from callireader_amd import inference as inf
    d = str(tmp_path / 'pages')
    paths, bad = _write_folder(None, d, n_good=4)
    raw = [[300, 310, 380, 480], [10, 20, 110, 140], [200, 50, 420, 300]]
    for k, p in enumerate(paths):
        if p == bad:
            continue
        w, h = Image.open(p).size
        shapes = [{'points': [[b[0] / w * 0.5, b[1] / h * 0.5], [b[2] / w * 0.5, b[3] / h * 0.5]]} for b in raw[:2 + k % 2]]
        json.dump({'imageHeight': h, 'imageWidth': w, 'shapes': shapes}, open(os.path.splitext(p)[0] + '.json', 'w'))
    monkeypatch.chdir(tmp_path)
    common = ['--tgt', d, '--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '8', '--batch_pages', '6']
    read = lambda n: open(tmp_path / 'results' / n, 'rb').read()      # noqa: E731
    inf.main(common + ['--save_name', 'greedy.json'])
    inf.main(common + ['--save_name', 'one.json', '--num_beams', '1', '--length_penalty', '2.0'])          # num_beams=1: the beam knobs are ignored
    inf.main(common + ['--save_name', 'b1.json', '--num_beams', '3'])
    inf.main(common + ['--save_name', 'b2.json', '--num_beams', '3', '--early_stopping', 'false', '--length_penalty', '1.0'])
    capsys.readouterr()
    assert read('one.json') == read('greedy.json')
    assert read('b1.json') == read('b2.json')
    res = json.loads(read('b1.json'))
    assert [r['imagePath'] for r in res] == paths and [r['response'] == 'ERROR!' for r in res] == [p == bad for p in paths]

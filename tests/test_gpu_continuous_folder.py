"""Continuous batching at the public surface: chat_ocr_continuous gives every page its own chat_ocr response (a bad page fails alone with
errors='return'), and `inference.py --tgt <folder> --continuous` on a checkpoint from disk writes the default folder mode's JSON and console lines.
The checkpoint, tokenizer and page folder are test_gpu_boundary.py's."""
import json
import os

import pytest
from PIL import Image

from test_gpu_boundary import YoloLike, _write_folder, ckpt, setup  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu


def test_chat_ocr_continuous_equals_chat_ocr_per_page(setup, tmp_path):
    m, tok = setup['model'], setup['tok']
    paths, bad = _write_folder(setup, str(tmp_path))
    det = YoloLike(setup['raw'][:3])
    gen = dict(num_beams=1, max_new_tokens=7, do_sample=False)
    q = '读出图中所有文字。'
    want = {}
    for p in paths:
        try:
            want[p] = m.chat_ocr(tok, det, p, q, gen, repetition_penalty=1.1)
        except Exception as e:
            want[p] = type(e)
    stats = {}
    got = list(m.chat_ocr_continuous(tok, det, paths, q, gen, repetition_penalty=1.1, slots=2, admit_group=2, visual_group=2, errors='return',
                                     stats=stats))
    assert sorted(i for i, _ in got) == list(range(len(paths)))
    for i, r in got:
        w = want[paths[i]]
        assert (r == w) if isinstance(w, str) else isinstance(r, w), paths[i]
    assert stats['pages_admitted'] == len(paths) - 1 and stats['decode_steps'] > 0
    with pytest.raises(FileNotFoundError):                  # errors='raise' (the default): chat_ocr's exception
        list(m.chat_ocr_continuous(tok, det, paths, q, gen, repetition_penalty=1.1, slots=2))


def test_inference_cli_continuous_folder_mode_writes_the_default_modes_json(ckpt, tmp_path, monkeypatch, capsys):
    from callireader_amd import inference as inf
    d = str(tmp_path / 'pages')
    paths, bad = _write_folder(None, d, n_good=5)
    raw = [[300, 310, 380, 480], [10, 20, 110, 140], [200, 50, 420, 300]]
    for k, p in enumerate(paths):
        if p == bad:
            continue
        w, h = Image.open(p).size
        shapes = [{'points': [[b[0] / w * 0.5, b[1] / h * 0.5], [b[2] / w * 0.5, b[3] / h * 0.5]]} for b in raw[:2 + k % 2]]
        json.dump({'imageHeight': h, 'imageWidth': w, 'shapes': shapes}, open(os.path.splitext(p)[0] + '.json', 'w'))
    monkeypatch.chdir(tmp_path)
    common = ['--tgt', d, '--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '9', '--batch_pages', '2']
    capsys.readouterr()
    inf.main(common + ['--save_name', 'default.json'])
    out_default = capsys.readouterr().out
    inf.main(common + ['--save_name', 'continuous.json', '--continuous'])
    out_cont = capsys.readouterr().out
    a = json.load(open(tmp_path / 'results' / 'continuous.json', encoding='utf-8'))
    b = json.load(open(tmp_path / 'results' / 'default.json', encoding='utf-8'))
    assert a == b and [r['imagePath'] for r in a] == paths
    assert [r['response'] == 'ERROR!' for r in a] == [p == bad for p in paths]
    lines = lambda out: [ln for ln in out.splitlines() if ln.startswith(('User:', 'Assistant:', 'An error has occured'))]
    assert lines(out_cont) == lines(out_default) and len(lines(out_cont)) >= 2 * len(paths)

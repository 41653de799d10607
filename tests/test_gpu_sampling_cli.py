"""`inference.py --do_sample` on a folder, end to end on a checkpoint from disk (test_gpu_boundary.py's checkpoint, tokenizer and page folder):
with --seed the results JSON is the same twice, another seed changes it, and without --do_sample the sampling flags change nothing (the default,
greedy output stays byte for byte what it was)."""
import json
import os

import pytest
from PIL import Image

from test_gpu_boundary import _write_folder, ckpt  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


def test_cli_folder_mode_sampling_is_reproducible_and_greedy_unchanged(ckpt, tmp_path, monkeypatch, capsys):
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
    common = ['--tgt', d, '--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '8', '--batch_pages', '3']

    def run(name, *extra):
        inf.main(common + ['--save_name', name] + list(extra))
        return open(tmp_path / 'results' / name, 'rb').read()
    greedy = run('greedy.json')
    assert run('greedy_knobs.json', '--temperature', '0.5', '--top_k', '3', '--top_p', '0.5', '--seed', '3') == greedy
    s1 = run('s1.json', '--do_sample', '--seed', '1')
    assert run('s1b.json', '--do_sample', '--seed', '1') == s1
    s2 = run('s2.json', '--do_sample', '--seed', '2')
    a, b, g = (json.loads(x.decode('utf-8')) for x in (s1, s2, greedy))
    assert [r['imagePath'] for r in a] == [r['imagePath'] for r in g] == paths
    assert [r['response'] == 'ERROR!' for r in a] == [p == bad for p in paths]
    assert a != b and a != g

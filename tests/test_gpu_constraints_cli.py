"""`inference.py --no_repeat_ngram_size / --min_new_tokens` on a folder, end to end on a checkpoint from disk (test_gpu_boundary.py's checkpoint,
tokenizer and page folder): --no_repeat_ngram_size 1 changes the results JSON and no response repeats an id any more; without the flags -- also
with them at 0, the defaults -- the JSON stays byte for byte what it is today."""
import json
import os

import pytest
from PIL import Image

from test_gpu_boundary import _write_folder, ckpt  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


def test_cli_folder_mode_constraints_change_the_json_and_defaults_do_not(ckpt, tmp_path, monkeypatch, capsys):
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
    common = ['--tgt', d, '--model', ckpt['dir'], '--params', ckpt['params'], '--max_new_tokens', '24', '--batch_pages', '3']

    def run(name, *extra):
        inf.main(common + ['--save_name', name] + list(extra))
        return open(tmp_path / 'results' / name, 'rb').read()
    greedy = run('greedy.json')
    assert run('zeros.json', '--no_repeat_ngram_size', '0', '--min_new_tokens', '0') == greedy
    assert inf.constraint_config(inf.argparse.Namespace(no_repeat_ngram_size=0, min_new_tokens=0)) == {}      # the generation_config of a run without the flags is today's
    n1 = run('n1.json', '--no_repeat_ngram_size', '1')
    assert run('n1b.json', '--no_repeat_ngram_size', '1') == n1
    a, g = (json.loads(x.decode('utf-8')) for x in (n1, greedy))
    assert [r['imagePath'] for r in a] == [r['imagePath'] for r in g] == paths
    assert [r['response'] == 'ERROR!' for r in a] == [p == bad for p in paths]
    assert a != g

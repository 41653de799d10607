"""bench.py's host-side pieces (no GPU): the script's flags, the benchlib modules, and the stand-in tokenizer directory of the api_level block."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_every_block_switch_and_benchlib_imports():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    for flag in ('--gpus', '--steps', '--warmup', '--pages', '--no-api', '--api-batches', '--no-ragged', '--two-steps-one-decode', '--no-strong-share', '--no-traffic',
                 '--no-cpu-baseline', '--no-vit-extra', '--no-pipeline', '--scaling', '--total-pages', '--dump-outputs', '--full'):
        assert flag in out, flag
    sys.path.insert(0, ROOT)
    import bench
    from benchlib import plan, measure, extras, api, kernels                      # noqa: F401  (every piece imports without a GPU)
    assert bench.plan_workload is plan.plan_workload and bench.CHAR_TILES == plan.CHAR_TILES == 96 and bench.PAGE_TILES == 11
    assert measure.PEAK_BF16_TFLOPS == 2500.0 and measure.PEAK_HBM_GBS == 8000.0
    for fn in ('strong_share_block', 'strong_scaling_block', 'single_gpu_extras', 'ragged_balanced', 'measure_balanced'):
        assert callable(getattr(extras, fn))


def test_a_plain_run_has_no_untimed_block_and_full_has_every_one():
    """Without --full the run does only what its headline needs; --full runs every untimed block of the world size, less what its --no-* switches drop."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.untimed_blocks(bench.parse_args([]), 1, 0) == set()
    assert bench.untimed_blocks(bench.parse_args(['--gpus', '2', '--steps', '3', '--warmup', '0', '--no-pipeline']), 2, 1) == set()
    one = {'one_batch_at_a_time', 'vit_prefill', 'strong_share', 'api_level', 'single_gpu_extras', 'traffic', 'cpu_baseline'}
    assert bench.untimed_blocks(bench.parse_args(['--full']), 1, 0) == one
    assert bench.untimed_blocks(bench.parse_args(['--full', '--cpu-baseline', 'full', '--fp8-extras']), 1, 0) == one
    for rank in (0, 1):
        assert bench.untimed_blocks(bench.parse_args(['--gpus', '2', '--full']), 2, rank) == {'one_batch_at_a_time', 'vit_prefill', 'all_gather', 'strong_scaling'}
    assert bench.untimed_blocks(bench.parse_args(['--gpus', '2', '--full', '--no-strong-block']), 2, 0) == {'one_batch_at_a_time', 'vit_prefill', 'all_gather'}
    drops = {'--no-api': 'api_level', '--no-vit-extra': 'single_gpu_extras', '--no-traffic': 'traffic', '--no-cpu-baseline': 'cpu_baseline', '--no-strong-share': 'strong_share'}
    for flag, block in drops.items():
        assert bench.untimed_blocks(bench.parse_args(['--full', flag]), 1, 0) == one - {block}, flag
    assert 'traffic' not in bench.untimed_blocks(bench.parse_args(['--full', '--pages', '8']), 1, 0)
    assert 'strong_share' not in bench.untimed_blocks(bench.parse_args(['--full', '--pages', '12']), 1, 0)     # not a multiple of --share-world


def test_options_of_full_blocks_are_refused_without_full():
    """An option that only shapes a block of --full would change nothing in a plain run: the script says so instead of printing a line without it."""
    sys.path.insert(0, ROOT)
    import bench
    for argv in (['--cpu-baseline', 'full'], ['--fp8-extras'], ['--two-steps-one-decode'], ['--balanced-owners', '4'], ['--api-batches', '2'],
                 ['--share-world', '4'], ['--share-steps', '1'], ['--strong-steps', '1']):
        with pytest.raises(SystemExit) as e:
            bench.parse_args(argv)
        assert e.value.code == 2, argv
        assert bench.parse_args(argv + ['--full']).full
    assert not bench.parse_args(['--cpu-baseline', 'sample', '--no-api', '--no-traffic']).full      # defaults and --no-* switches are fine either way
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--fp8-extras'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 2 and b'--full' in r.stdout, r.stdout[-2000:]


def test_dump_outputs_writes_ids_and_fixed_samples(tmp_path):
    """bench.dump_outputs (--dump-outputs): the ids whole, a small tensor whole, a large one as the same seeded sample on every call; float32 only."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    ids = [[5, 92542, 7], [1, 2, 3]]
    small = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    big = torch.randn(bench.DUMP_SAMPLE + 1000, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    names = bench.dump_outputs(str(tmp_path / 'a'), ids, {'small': small, 'big': big, 'absent': None}, suffix='_rank1')
    assert names == ['big', 'small', 'token_ids']
    assert sorted(os.listdir(tmp_path / 'a')) == ['big_rank1.npy', 'small_rank1.npy', 'token_ids_rank1.npy']
    got = {n: np.load(tmp_path / 'a' / f'{n}_rank1.npy') for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got['token_ids'], np.array(ids, dtype=np.float32)) and np.array_equal(got['small'], small.float().numpy().reshape(-1))
    assert got['big'].shape == (bench.DUMP_SAMPLE,) and np.isin(got['big'], big.float().numpy()).all()
    bench.dump_outputs(str(tmp_path / 'b'), ids, {'big': big.clone()})
    assert np.array_equal(np.load(tmp_path / 'b' / 'big.npy'), got['big'])


def test_dump_outputs_of_all_ranks_stay_within_the_cap(tmp_path):
    """Every rank writes its own files: at 8 ranks of the default step's shapes (64 pages x 128 ids, two tensors far larger than a sample)
    all files together stay within bench.DUMP_BYTES, each rank's samples are as large as its share allows, and the positions are fixed."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    ids = [[p] * 128 for p in range(64)]
    big = torch.randn(3 * bench.DUMP_SAMPLE, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    world = 8
    for r in range(world):
        bench.dump_outputs(str(tmp_path / 'all'), ids, {'a': big, 'b': big[1:]}, suffix=f'_rank{r}', world=world)
    files = os.listdir(tmp_path / 'all')
    assert len(files) == 3 * world
    assert sum(os.path.getsize(tmp_path / 'all' / f) for f in files) <= bench.DUMP_BYTES
    a0 = np.load(tmp_path / 'all' / 'a_rank0.npy')
    assert 4 * 2 * a0.size > bench.DUMP_BYTES // world - 4 * bench.NPY_HEADER - 64 * 128 * 4 - 8 and a0.size < bench.DUMP_SAMPLE
    assert np.array_equal(a0, np.load(tmp_path / 'all' / f'a_rank{world - 1}.npy'))
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / 'none'), [[0] * (1 << 20)] * 64, {'a': big}, world=world)


def test_api_level_tokenizer_dir_has_the_references_structure(tmp_path):
    """The stand-in for the reference's tokenizer files (benchlib/api.py): 92 544 sentencepiece pieces with [UNUSED_TOKEN_140] = 92 537 as a user-defined piece, the reference's
    added-token ids, every id of the 92 553-row vocabulary decodable (random-init weights pick any of them), and a page prompt with the reference's token counts."""
    pytest.importorskip('sentencepiece')
    sys.path.insert(0, ROOT)
    from benchlib.api import make_tokenizer_dir, make_pages, PROMPT, ADDED, VOCAB_SP
    from callireader_amd.tokenization_internlm2 import InternLM2Tokenizer
    from callireader_amd.conversation import get_conv_template
    from callireader_amd.config import IMG_CONTEXT_TOKEN_ID, ALIGNED_TOKEN_ID, EOS_TOKEN_ID
    d = str(tmp_path / 'InternVL')
    os.makedirs(d)
    make_tokenizer_dir(d)
    tok = InternLM2Tokenizer.from_pretrained(d)
    assert tok.vocab_size == VOCAB_SP == 92544
    assert tok.convert_tokens_to_ids('[UNUSED_TOKEN_140]') == ALIGNED_TOKEN_ID == 92537
    assert tok.convert_tokens_to_ids('<IMG_CONTEXT>') == IMG_CONTEXT_TOKEN_ID == ADDED['<IMG_CONTEXT>'] and tok.convert_tokens_to_ids('<|im_end|>') == EOS_TOKEN_ID
    t = get_conv_template('internlm2-chat')
    t.append_message(t.roles[0], '<image>\n' + PROMPT + '[UNUSED_TOKEN_140]' * 288)
    t.append_message(t.roles[1], None)
    ids = tok(t.get_prompt().replace('<image>', '<img>' + '<IMG_CONTEXT>' * 256 * 11 + '</img>', 1), return_tensors='pt')['input_ids'].reshape(-1)
    assert int((ids == IMG_CONTEXT_TOKEN_ID).sum()) == 2816 and int((ids == ALIGNED_TOKEN_ID).sum()) == 288 and 3150 <= ids.numel() <= 3292     # the bench's KV cache has room for 3164 + 128
    text = tok.batch_decode(torch.arange(0, 92553).reshape(1, -1), skip_special_tokens=True)[0]
    assert isinstance(text, str) and len(text) > 92553
    assert tok.batch_decode(torch.tensor([[5, EOS_TOKEN_ID, 7]]), skip_special_tokens=False)[0].count('<|im_end|>') == 1
    # the page folder: the example page and its boxes JSON n times (what inference.py reads without a detector)
    paths, boxes = make_pages(str(tmp_path), 3, ROOT)
    assert len(paths) == 3 and len(boxes) == 96 and all(os.path.exists(os.path.splitext(p)[0] + '.json') for p in paths)
    from callireader_amd.inference import get_image_paths, boxes_for
    assert get_image_paths(str(tmp_path)) == sorted(paths) and boxes_for(paths[0]) == boxes
    assert json.load(open(os.path.splitext(paths[0])[0] + '.json'))['imageWidth'] == 788

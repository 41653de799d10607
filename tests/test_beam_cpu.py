"""Beam search, host side.  (1) tests/beam_replica.py -- the seven steps the device implements -- against the installed transformers' deterministic
beam search on a tiny seeded LlamaForCausalLM driven with inputs_embeds only, over num_beams x length_penalty x early_stopping x repetition_penalty x
{EOS early, EOS late, no EOS}: identical ids, sequences_scores within 1e-5.  (2) the generation-config parsing and validation (sampling.parse_beams).
(3) the group layout of the host loop and what the ABI refuses without a device."""
import itertools
import warnings

import pytest
import torch

from beam_replica import beam_search
from callireader_amd import sampling as S

MAX_NEW, PROMPT = 7, 5
EOS, EOS_LIFT = 7, {'early': 3.0, 'late': 1.5}
SWEEP = list(itertools.product((2, 3, 4, 8), (0.0, 1.0, 2.0), (False, True, 'never'), (1.0, 1.5), ('early', 'late', None)))


@pytest.fixture(scope='module')
def runs():
    """Every case of the sweep, run once through transformers and through the replica (the same model is the replica's logits callback)."""
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=200, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      max_position_embeddings=64)
    m = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(5.0)                # flat enough that several hypotheses compete, peaked enough that beams and greedy part ways
    bias = torch.zeros(200)                       # added to the LM head's output: the EOS id's logit is lifted so that hypotheses finish
    m.lm_head.register_forward_hook(lambda mod, inp, out: out + bias)
    emb = torch.randn(1, PROMPT, 32)

    def logits_fn(seqs):
        with torch.no_grad():
            ids = torch.tensor(seqs, dtype=torch.long)
            e = emb.expand(len(seqs), -1, -1)
            if ids.numel():
                e = torch.cat([e, m.get_input_embeddings()(ids)], dim=1)
            return m(inputs_embeds=e).logits[:, -1].float()

    def hf(**kw):
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter('ignore')
            return m.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=MAX_NEW, pad_token_id=0, return_dict_in_generate=True, output_scores=True, **kw)

    def set_mode(mode):
        """EOS reached early (a lift that makes it the likely next id within a step or two), late (a smaller lift), or no EOS id at all."""
        bias.zero_()
        if mode is not None:
            bias[EOS] = EOS_LIFT[mode]
        return EOS if mode is not None else None

    greedy, out = {}, []
    for pen in (1.0, 1.5):
        for mode in ('early', 'late', None):
            eos = set_mode(mode)
            greedy[pen, mode] = hf(num_beams=1, repetition_penalty=pen, eos_token_id=eos).sequences[0].tolist()
    for B, lp, es, pen, mode in SWEEP:
        eos = set_mode(mode)
        o = hf(num_beams=B, length_penalty=lp, early_stopping=es, repetition_penalty=pen, eos_token_id=eos)
        bm = beam_search(logits_fn, B, MAX_NEW, eos_token_id=eos, length_penalty=lp, early_stopping=es, repetition_penalty=pen)
        out.append(dict(case=(B, lp, es, pen, mode), eos=eos, hf_ids=o.sequences[0].tolist(), hf_score=float(o.sequences_scores[0]), bm=bm,
                        greedy=greedy[pen, mode]))
    return out


def test_replica_matches_transformers(runs):
    skipped = 0
    for r in runs:
        ids, score = r['bm'].result()
        if ids != r['hf_ids'] or abs(score - r['hf_score']) > 1e-5:
            # only an exact tie among a step's top K candidates excuses a case (torch.topk leaves its order open)
            assert r['bm'].min_gap == 0.0, (r['case'], ids, r['hf_ids'], score, r['hf_score'], r['bm'].min_gap)
            skipped += 1
    assert skipped <= 0.05 * len(runs), skipped


def test_the_sweep_is_not_degenerate(runs):
    n = len(runs)
    differs = sum(r['bm'].result()[0] != r['greedy'] for r in runs)
    by_eos = sum(r['eos'] is not None and r['bm'].result()[0][-1] == r['eos'] and len(r['bm'].result()[0]) < MAX_NEW for r in runs)
    heur_alive = sum(r['bm'].stopped_by == 'heuristic' and r['bm'].alive_at_stop for r in runs)
    assert differs >= n / 2, (differs, n)
    assert by_eos >= n / 3, (by_eos, n)
    assert heur_alive >= 1


# ---- parsing and validation -------------------------------------------------------------------------------------------------------
def test_parse_beams_defaults_and_values():
    assert S.parse_beams({}) is None and S.parse_beams(dict(num_beams=1, length_penalty=2.0, early_stopping=True)) is None
    assert S.parse_beams(dict(num_beams=None)) is None
    bp = S.parse_beams(dict(num_beams=3))
    assert (bp.num_beams, bp.length_penalty, bp.early_stopping, bp.early_code) == (3, 1.0, False, 0)
    bp = S.parse_beams(dict(num_beams=8, length_penalty=0, early_stopping='never', do_sample=False))
    assert (bp.num_beams, bp.length_penalty, bp.early_code) == (8, 0, 2)
    assert S.parse_beams(dict(num_beams=2, early_stopping=True)).early_code == 1
    assert S.parse(dict(num_beams=4)) is None                                       # beam search is not sampling


@pytest.mark.parametrize('kw', [dict(num_beams=0), dict(num_beams=-2), dict(num_beams=2.5), dict(num_beams=True), dict(num_beams=2, early_stopping='always'),
                                dict(num_beams=2, early_stopping=1), dict(num_beams=2, length_penalty=float('nan')), dict(num_beams=2, length_penalty='x')])
def test_invalid_beam_values_raise_value_error(kw):
    with pytest.raises(ValueError):
        S.parse_beams(kw)


@pytest.mark.parametrize('kw', [dict(num_beams=9), dict(num_beams=2, do_sample=True), dict(num_beams=2, num_return_sequences=2), dict(num_beams=4, num_beam_groups=2),
                                dict(num_beams=2, diversity_penalty=0.5), dict(num_beams=2, constraints=[object()]), dict(num_beams=2, force_words_ids=[[1]]),
                                dict(num_beams=2, output_scores=True, return_dict_in_generate=True), dict(num_beams=2, return_scores=True)])
def test_unsupported_beam_knobs_raise(kw):
    with pytest.raises(NotImplementedError):
        S.parse_beams(kw)
    with pytest.raises(NotImplementedError):
        S.parse(kw)


def test_gen_args_takes_beams_only_where_a_beam_path_exists():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    assert InternVLChatModel._gen_args(dict(num_beams=4, max_new_tokens=9), allow_beams=True)[::2] == (9, None)
    with pytest.raises(NotImplementedError, match='num_beams=4'):
        InternVLChatModel._gen_args(dict(num_beams=4, max_new_tokens=9))            # the one-row-per-page callers
    with pytest.raises(ValueError):
        InternVLChatModel._gen_args(dict(num_beams=0), allow_beams=True)


# ---- group layout and the ABI's refusals ------------------------------------------------------------------------------------------------
def test_group_layout():
    from callireader_amd.modeling_internvl_chat import beam_slots
    for B in (2, 3, 8):
        rows = [s for i in range(5) for s in beam_slots(i, B)]
        assert rows == list(range(5 * B))                                           # pages tile the cache: page i owns B consecutive sequences
        assert beam_slots(3, B)[0] == 3 * B and len(beam_slots(3, B)) == B


def test_abi_refuses_bad_beam_state_without_a_gpu():
    from callireader_amd import _binding as B
    for nb in (1, 9, 0, -1):
        assert B.lib.cr_kv_set_beam(None, 0, nb, 1.0, 0, 2, 16, None) == -1
        assert b'num_beams' in B.lib.cr_last_error()
    assert B.lib.cr_kv_set_beam(None, 0, 2, 1.0, 3, 2, 16, None) == -1 and b'early_stopping' in B.lib.cr_last_error()
    assert B.lib.cr_kv_set_beam(None, 0, 2, float('inf'), 0, 2, 16, None) == -1 and b'length_penalty' in B.lib.cr_last_error()
    assert B.lib.cr_kv_set_beam(None, 0, 2, 1.0, 0, 2, 16, None) == -1 and b'sequences' in B.lib.cr_last_error()      # good values: the missing cache
    assert B.lib.cr_op_beam_step(None, 1, 100, None, 8, None, 1.0, None, None, None, None) == -1 and b'cr_op_beam_step' in B.lib.cr_last_error()
    assert B.lib.cr_kv_beam_result(None, 0, None, 0, None, None, None, None) == -1
    assert B.lib.cr_kv_beam_reorder(None, 0, 2, None, 0, None) == -1 and B.lib.cr_kv_beam_reorder(None, 0, 9, None, 0, None) == -1


def test_pipelines_and_sharded_entry_points_refuse_beams():
    from callireader_amd import parallel
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    with pytest.raises(NotImplementedError, match='beam'):
        parallel.chat_ocr_pages_sharded(None, None, None, [], 'q', dict(num_beams=2))
    with pytest.raises(NotImplementedError, match='beam'):
        parallel.sharded_generate(None, [], [], [], img_id=0, ref_id=0, max_new_tokens=4, num_beams=2)
    with pytest.raises(NotImplementedError, match='PagePipeline'):
        next(InternVLChatModel.chat_ocr_stream(None, None, None, [], 'q', dict(num_beams=2)))
    with pytest.raises(NotImplementedError, match='ContinuousPipeline'):
        next(InternVLChatModel.chat_ocr_continuous(None, None, None, [], 'q', dict(num_beams=2)))

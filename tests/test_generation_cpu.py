"""The host side of generation without a GPU, over the stub engine and cache of engine_stubs.py: which sequences every decode call runs, when ids
are read back, the order of an admission (reset -> sampling -> logprobs -> prefill) and where ids are cut.  The first part drives public surface
only (generate_pages, generate_ocr, session.chat_ocr, session.ask_many); the second part holds callireader_amd/generation.py's functions and
InternVLChatModel.kv(n) to the same traces."""
import pytest
import torch

from engine_stubs import EOS, HID, ids_of, make_model, make_session


def decodes(eng):
    return [e[1] for e in eng.log if e[0] == 'decode']


def before_first(eng, kind):
    """The log up to the first entry of `kind` (all of it when there is none)."""
    i = next((k for k, e in enumerate(eng.log) if e[0] == kind), len(eng.log))
    return eng.log[:i]


def embeds_of(*rows):
    return [torch.zeros(r, HID) for r in rows]


# ---- public surface: these pass unchanged before and after the loops were made one -------------------------------------------------
@pytest.mark.parametrize('scored', [False, True])
def test_generate_pages_two_rows_one_stops_early(scored):
    from callireader_amd.sampling import SamplingParams
    m = make_model()
    eng = m.engine
    eng.script[0] = [11, 12, EOS, 13, 14, 15, 16]
    kw = dict(sampling=[None, SamplingParams(temperature=0.7, top_k=5, top_p=0.9)], seeds=[1, 2], logprobs=[2, 0]) if scored else {}
    out = m.generate_pages(embeds_of(5, 7), max_new_tokens=10, eos_token_id=EOS, check_every=4, **kw)
    ids, sc = out if scored else (out, None)
    assert ids == [[11, 12, EOS], [77] * 10]
    assert decodes(eng) == [[0, 1]] * 4 + [[1]] * 5
    state = [('set_sampling', 1), ('set_logprobs', 0, 2)] if scored else []
    assert before_first(eng, 'decode') == [('reset', -1)] + state + [('prefill_batch', [0, 1], [5, 7])]      # and nothing read back before the first step
    if scored:
        assert len(sc[0]) == 3 and sc[1] is None


def test_generate_pages_prefills_in_groups_and_regrows_its_cache():
    m = make_model()
    eng = m.engine
    assert m.generate_pages(embeds_of(3, 4, 5), max_new_tokens=2, eos_token_id=EOS, prefill_batch=2) == [[77, 77]] * 3
    assert [e for e in eng.log if e[0] == 'prefill_batch'] == [('prefill_batch', [0, 1], [3, 4]), ('prefill_batch', [2], [5])]
    assert decodes(eng) == [[0, 1, 2]]
    assert m._kv.n_seqs == 3 and m.max_pages == 3
    m.generate_pages(embeds_of(3, 4, 5, 6), max_new_tokens=2, eos_token_id=None)
    assert eng.kvs[0].freed and m._kv is eng.kvs[1] and m._kv.n_seqs == 4 and m.max_pages == 4


def generate_ocr(m, n_prompt=4, **kw):
    m.img_context_token_id = 0
    return m.generate_ocr(input_ids=torch.arange(20, 20 + n_prompt).reshape(1, -1), repetition_penalty=1.0, eos_token_id=EOS, **kw)


def test_one_sequence_decodes_max_new_minus_one_steps():
    m = make_model()
    out = generate_ocr(m, max_new_tokens=6)
    assert out.tolist() == [[77] * 6]
    assert decodes(m.engine) == [[0]] * 5 and m._kv.length(0) == 4 + 5
    assert m._kv.n_seqs == 1


def test_one_sequence_looks_before_its_first_chunk():
    m = make_model()
    m.engine.script[0] = [EOS, 11, 12]
    assert generate_ocr(m, max_new_tokens=6).tolist() == [[EOS]]
    assert decodes(m.engine) == []                                   # the prefill's own pick was EOS: no decode step
    m = make_model()
    m.engine.script[0] = [11, 12, EOS]
    assert generate_ocr(m, max_new_tokens=40).tolist() == [[11, 12, EOS]]
    assert decodes(m.engine) == [[0]] * 16                           # looked at n = 1 and n = 17: one chunk of check_every steps


def test_one_sequence_admission_order_and_scores():
    m = make_model()
    m.engine.script[0] = [11, EOS]
    out = generate_ocr(m, max_new_tokens=6, do_sample=True, top_k=5, return_dict_in_generate=True, output_scores=True, top_logprobs=2)
    assert out.sequences.tolist() == [[11, EOS]] and tuple(out.token_logprobs.shape) == (1, 2)
    kinds = [e[0] for e in m.engine.log if e[0] != 'embed']
    assert kinds[:4] == ['reset', 'set_sampling', 'set_logprobs', 'prefill']


def test_one_sequence_prompt_check():
    m = make_model()
    with pytest.raises(ValueError, match=r'prompt of 4 tokens \+ 509 new exceeds max_tokens=512'):
        generate_ocr(m, max_new_tokens=509)
    assert not [e for e in m.engine.log if e[0] in ('prefill', 'decode')]


def test_session_turn_runs_the_one_sequence_loop_on_the_trunk():
    s, eng = make_session()
    eng.script[0] = ids_of('abc') + [EOS] + ids_of('xy')
    assert s.chat_ocr('what?', dict(num_beams=1, max_new_tokens=40, do_sample=False)) == 'abc'
    assert decodes(eng) == [[0]] * 16
    assert not [e for e in eng.log if e[0] == 'reset']               # the trunk is rolled back, never reset
    s, eng = make_session()
    eng.script[0] = [EOS]
    assert s.chat_ocr('what?', dict(num_beams=1, max_new_tokens=40, do_sample=False)) == ''
    assert decodes(eng) == []


def test_ask_many_decodes_its_branches_as_one_batch():
    s, eng = make_session(max_branches=3)
    eng.script[1], eng.script[2] = ids_of('r1') + [EOS], ids_of('r2') + [EOS]
    out = s.ask_many(['who?', 'when?', 'why?'], dict(num_beams=1, max_new_tokens=20, do_sample=False))
    assert out == ['r1', 'r2', 'C' * 20]
    assert decodes(eng) == [[1, 2, 3]] * 16 + [[3]] * 3
    after_prefill = eng.log[[e[0] for e in eng.log].index('prefill_batch'):]
    assert not [e for e in before_first_of(after_prefill, 'decode') if e[0] == 'generated']      # no look before the first chunk


def before_first_of(log, kind):
    i = next((k for k, e in enumerate(log) if e[0] == kind), len(log))
    return log[:i]


# ---- callireader_amd/generation.py ------------------------------------------------------------------------------------------------------
def prefilled(script, rows=(3, 3)):
    """A stub engine and a cache whose sequences 0 .. len(rows) - 1 are prefilled (each holds its first id)."""
    m = make_model()
    eng = m.engine
    eng.script.update(script)
    kv = eng.kv_alloc(len(rows), 512)
    eng.prefill_batch(kv, list(range(len(rows))), embeds_of(*rows))
    eng.log.clear()
    return eng, kv


def test_cut_ids():
    from callireader_amd.generation import cut_ids
    ids = [5, 6, EOS, 7, EOS, 8]
    assert cut_ids(ids, EOS, 6) == [5, 6, EOS]                       # EOS inside the budget
    assert cut_ids(ids, EOS, 3) == [5, 6, EOS]                       # EOS at the budget
    assert cut_ids(ids, EOS, 2) == [5, 6]                            # EOS beyond the budget
    assert cut_ids([5, 6, 7], EOS, 2) == [5, 6] and cut_ids([5, 6, 7], EOS, 9) == [5, 6, 7]      # EOS absent
    assert cut_ids(ids, None, 4) == [5, 6, EOS, 7]                   # eos=None: the budget alone
    assert ids == [5, 6, EOS, 7, EOS, 8]


def test_decode_rows_with_budgets_and_no_eos():
    from callireader_amd.generation import decode_rows
    eng, kv = prefilled({0: list(range(100, 120)), 1: list(range(200, 220))})
    chunks = []
    outs = decode_rows(eng, kv, [0, 1], 10, None, 1.0, check_every=4, budgets=[3, 10], on_chunk=lambda steps, rows, s: chunks.append((steps, rows)))
    assert outs == [[100, 101, 102], list(range(200, 210))]
    assert decodes(eng) == [[0, 1]] * 4 + [[1]] * 5
    assert chunks == [(4, 2), (4, 1), (1, 1)]
    # eos=None: a row is read back only at or past its budget -- once each
    assert [e for e in eng.log if e[0] == 'generated'] == [('generated', 0), ('generated', 1)]


def test_decode_rows_without_look_first_issues_its_first_chunk():
    from callireader_amd.generation import decode_rows
    eng, kv = prefilled({0: [EOS, 11, 12]}, rows=(3,))
    assert decode_rows(eng, kv, [0], 10, EOS, 1.0, check_every=4) == [[EOS]]
    assert decodes(eng) == [[0]] * 4 and eng.log[0] == ('decode', [0])
    eng, kv = prefilled({0: [EOS, 11, 12]}, rows=(3,))
    assert decode_rows(eng, kv, [0], 10, EOS, 1.0, check_every=4, look_first=True) == [[EOS]]
    assert decodes(eng) == []


def test_decode_rows_keeps_input_order_and_a_budget_of_one():
    from callireader_amd.generation import decode_rows
    eng, kv = prefilled({2: [21, EOS], 0: [1, 2, 3, 4]}, rows=(3, 3, 3))
    assert decode_rows(eng, kv, [2, 0], 3, EOS, 1.0, check_every=16) == [[21, EOS], [1, 2, 3]]
    assert decodes(eng) == [[2, 0]] * 2
    eng, kv = prefilled({}, rows=(3,))
    assert decode_rows(eng, kv, [0], 1, EOS, 1.0) == [[77]] and decodes(eng) == []


def test_admit_orders_reset_sampling_logprobs_prefill():
    from callireader_amd.generation import admit
    from callireader_amd.sampling import SamplingParams
    m = make_model()
    eng = m.engine
    kv = eng.kv_alloc(8, 512)
    sp = SamplingParams(temperature=0.7, top_k=5, top_p=0.9)
    admit(eng, kv, [5, 2, 7], embeds_of(3, 4, 5), 1.0, per_page=[None, (sp, 9), None], lpn=[0, 0, 3], prefill_batch=2, reset_each=True)
    assert eng.log == [('reset', 5), ('reset', 2), ('reset', 7), ('set_sampling', 2), ('set_logprobs', 7, 3),
                       ('prefill_batch', [5, 2], [3, 4]), ('prefill_batch', [7], [5])]


def test_check_fits():
    from callireader_amd.generation import check_fits
    check_fits(500, 12, 512)
    with pytest.raises(ValueError, match=r'prompt of 500 tokens \+ 13 new exceeds max_tokens=512'):
        check_fits(500, 13, 512)


def test_kv_grows_never_shrinks_and_frees_the_old_cache():
    m = make_model()
    eng = m.engine
    m.max_pages = 2
    a = m.kv(1)
    assert a.n_seqs == 1 and m.kv() is a and m.kv(1) is a and m.max_pages == 2       # kv() / kv(1): whatever exists
    b = m.kv(2)
    assert a.freed and b is not a and b.n_seqs == 2 and m.max_pages == 2            # re-made at max_pages
    c = m.kv(5)
    assert b.freed and c.n_seqs == 5 and m.max_pages == 5
    assert m.kv(3) is c and m.kv(1) is c and m.kv() is c and not c.freed and len(eng.kvs) == 3
    m2 = make_model()
    m2.max_pages = 4
    assert m2.kv().n_seqs == 4                                      # the first cache of kv(): max_pages sequences

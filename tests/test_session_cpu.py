"""The planning of callireader_amd/session.py without a GPU: a PageSession over a stub engine that records calls and emits scripted ids.
What is checked is host logic only -- the prefix p every turn keeps, the rows it embeds, the cache operations it issues, the refusals."""
import pytest
import torch

from chat_helpers import FakeTokenizer, SPECIALS
from engine_stubs import EOS, IMG, N_REF, N_TILES, REF, ids_of, make_model, make_session


GEN = dict(num_beams=1, max_new_tokens=6, do_sample=False)


def prefills(eng):
    return [e for e in eng.log if e[0] == 'prefill']


def test_first_turn_embeds_the_whole_prompt_with_the_pages_rows():
    s, eng = make_session()
    eng.script[0] = ids_of('abc') + [EOS] + ids_of('xy')
    resp, hist = s.chat_ocr('what?', GEN, return_history=True, repetition_penalty=1.5)
    assert resp == 'abc' and hist == [('<image>\nwhat?' + '[UNUSED_TOKEN_140]' * N_REF, 'abc')]
    emb = [e for e in eng.log if e[0] == 'embed']
    assert len(emb) == 1 and emb[0][2] == [100 + k for k in range(8)] and emb[0][3] == [200, 201, 202] and emb[0][4] == IMG
    S = len(emb[0][1])
    assert ('truncate', 0, 0) in eng.log and s.rows_prefilled == [S]
    # six ids generated, five of them fed back: the cached positions hold the prompt, the answer, EOS and ONE speculative id
    assert s.kv.length(0) == S + 5 and s.cached_ids == emb[0][1] + ids_of('abc') + [EOS] + ids_of('x')


def turn1(s, eng, tail='xy'):
    eng.script[0] = ids_of('abc') + [EOS] + ids_of(tail)
    _, hist = s.chat_ocr('what?', GEN, return_history=True)
    S1 = len(prefills(eng)[0][2])
    eng.log.clear()
    return hist, S1


def test_identical_reask_keeps_all_but_the_last_row():
    s, eng = make_session()
    _, S1 = turn1(s, eng)
    s.chat_ocr('what?', GEN)
    assert ('truncate', 0, S1 - 1) in eng.log                         # the cap at S - 1: the prefill needs a row
    assert [len(e[2]) for e in prefills(eng)] == [1] and s.rows_prefilled[-1] == 1


def test_second_turn_whose_answer_retokenises_to_the_generated_ids():
    s, eng = make_session()
    hist, S1 = turn1(s, eng)
    s.chat_ocr('who wrote it?', GEN, history=hist)
    # prompt 1, 'abc', EOS are cached; the speculative 'x' behind EOS is not the prompt's next id ('<|im_start|>')
    p = S1 + 4
    assert ('truncate', 0, p) in eng.log
    emb = [e for e in eng.log if e[0] == 'embed']
    ids2 = s.tokenizer(s.m._build_query('<image>\nwho wrote it?', hist[:1], [N_TILES], '<img>', '</img>', '<IMG_CONTEXT>')[0])['input_ids'][0].tolist()
    assert emb[0][1] == ids2[p:] and emb[0][2] is None                # exactly rows [p, S), none of them visual
    assert prefills(eng)[0][2] == ids2[p:] and s.rows_prefilled[-1] == len(ids2) - p


def test_speculative_ids_past_eos_count_only_where_they_are_the_prompts_ids():
    """Behind EOS the trunk holds ONE speculative id (the last generated id is cached nowhere).  It is cut unless it happens to be the next
    prompt's id at that position -- then the cached row is the row that prompt would compute, and it is kept."""
    s, eng = make_session()
    eng.script[0] = ids_of('abc') + [EOS, SPECIALS['<|im_start|>']] + ids_of('u')     # the model "went on" as the next prompt does
    _, hist = s.chat_ocr('what?', GEN, return_history=True)
    S1 = len(prefills(eng)[0][2])
    eng.log.clear()
    s.chat_ocr('who?', GEN, history=hist)
    assert [e for e in eng.log if e[0] == 'truncate'] == [('truncate', 0, S1 + 5)]


def test_second_turn_whose_retokenised_answer_differs_at_its_third_id():
    s, eng = make_session(tok=FakeTokenizer())                        # decodes ids to digits: the answer re-tokenises to other ids
    eng.script[0] = ids_of('12') + [5000, EOS, 5001, 5002]
    resp, hist = s.chat_ocr('what?', GEN, return_history=True)
    S1 = len(prefills(eng)[0][2])
    # FakeTokenizer writes the ids as decimal numbers: the answer text starts with the digits of the first id, not with the ids
    first = [10 + ord(c) for c in resp]
    agree = 0
    while agree < 3 and first[agree] == (ids_of('12') + [5000])[agree]:
        agree += 1
    eng.log.clear()
    s.chat_ocr('who?', GEN, history=hist)
    assert [e for e in eng.log if e[0] == 'truncate'][0][2] == S1 + agree
    s2, eng2 = make_session()                                         # the same with a tokenizer that round-trips, but a third id that does not
    eng2.script[0] = ids_of('ab') + [7500, EOS, 5001, 5002]           # chr(7490) re-encodes as 10 + 7490 % 7000 = 500, not 7500
    _, hist2 = s2.chat_ocr('what?', GEN, return_history=True)
    S1 = len(prefills(eng2)[0][2])
    eng2.log.clear()
    s2.chat_ocr('who?', GEN, history=hist2)
    assert [e for e in eng2.log if e[0] == 'truncate'][0][2] == S1 + 2


def test_a_prompt_shorter_than_the_cache():
    s, eng = make_session()
    turn1(s, eng)
    cached = list(s.cached_ids)
    s.chat_ocr('w', GEN)                                              # another first turn, shorter than what the trunk holds
    ids = [e for e in eng.log if e[0] == 'embed'][0]
    p = [e for e in eng.log if e[0] == 'truncate'][0][2]
    assert cached[:p] == s.cached_ids[:p] and cached[p] != s.cached_ids[p]
    assert cached[p - 1] == 10 + ord('w') and p < len(cached)         # the prefix ends inside the question, after the page's <IMG_CONTEXT> run
    # the tail holds the aligned tokens and no visual one: they still take the page's pseudo-token rows, from row 0
    assert ids[2] == [200, 201, 202] and ids[4] == REF and ids[1].count(REF) == 3 and IMG not in ids[1]


def test_a_cut_inside_the_visual_run_counts_the_rows_used_up():
    s, eng = make_session()
    turn1(s, eng)
    ids = list(s.cached_ids)
    k = ids.index(IMG) + 5                                            # five <IMG_CONTEXT> before the cut
    s._embed(ids, k)
    e = eng.log[-1]
    assert e[2] == [105, 106, 107] and e[1] == ids[k:]


def test_refusals():
    from callireader_amd.session import PageSession
    s, eng = make_session(max_branches=2)
    with pytest.raises(NotImplementedError, match='chat_ocr'):
        s.chat_ocr('what?', dict(GEN, num_beams=2))
    with pytest.raises(NotImplementedError, match='chat_ocr'):
        s.ask_many(['a'], dict(GEN, num_beams=3))
    with pytest.raises(ValueError, match='max_branches'):
        s.ask_many(['a', 'b', 'c'], GEN)
    with pytest.raises(ValueError, match='max_branches'):
        s.ask_many([], GEN)
    with pytest.raises(ValueError, match='max_tokens'):
        s.chat_ocr('what?', dict(GEN, max_new_tokens=512))
    assert eng.log == []                                              # nothing reached the cache
    with pytest.raises(NotImplementedError, match="kv_cache_dtype='bf16'"):
        make_session(kv_cache_dtype='e4m3')
    m = make_model(kv_cache_dtype='e4m3')
    with pytest.raises(NotImplementedError, match="kv_cache_dtype='bf16'"):
        PageSession.open(m, FakeTokenizer(), None, '/nonexistent.jpg')           # refused before the page is even opened
    with s:
        pass
    assert s.kv is None and eng.kvs[0].freed


def test_ask_many_groups_its_forks_by_prefix_length():
    s, eng = make_session(max_branches=4)
    hist, S1 = turn1(s, eng)
    trunk = (s.kv.length(0), list(s.cached_ids))
    for b in (1, 2, 3):
        eng.script[b] = ids_of('r%d' % b) + [EOS]
    qs = ['who?', 'when?', 'who?']                                   # as second turns: all keep prompt 1 + answer + EOS
    out = s.ask_many(qs, GEN, history=hist)
    assert out == ['r1', 'r2', 'r3']
    forks = [e for e in eng.log if e[0] == 'fork']
    # 'who?' and 'when?' share '<|im_start|>user\n<image>\nwh' behind the cached answer; the trunk holds a speculative id there, so all three
    # branches keep the same prefix and go out in ONE fork
    assert forks == [('fork', 0, [1, 2, 3], S1 + 4)]
    pb = [e for e in eng.log if e[0] == 'prefill_batch'][0]
    assert pb[1] == [1, 2, 3] and pb[2][0] == pb[2][2] == pb[2][1] - 1
    assert (s.kv.length(0), s.cached_ids) == trunk and not prefills(eng)
    assert len(hist) == 1                                             # the caller's history is not extended by a batch of questions


def test_ask_many_forks_once_per_distinct_prefix_and_fills_an_empty_trunk():
    from callireader_amd.session import fork_groups
    assert fork_groups([7, 3, 7, 7, 3]) == {7: [0, 2, 3], 3: [1, 4]}
    s, eng = make_session(max_branches=3)
    out = s.ask_many(['what is it?', 'what?', 'who?'], GEN)
    assert out == ['C' * 6] * 3                                       # the stub's default id 77 = 10 + ord('C')
    # the prompts share everything up to '<image>\nwh': that goes into the empty trunk, and the pick its prefill appended is dropped
    shared = prefills(eng)[0][2]
    assert shared[-2:] == ids_of('wh') and shared.count(IMG) == 8 and REF not in shared
    n = len(shared)
    assert [e for e in eng.log if e[0] == 'truncate'] == [('truncate', 0, 0), ('truncate', 0, n)]
    assert s.cached_ids == shared and s.kv.length(0) == n and s.kv.generated(0) == []
    assert [e for e in eng.log if e[0] == 'fork'] == [('fork', 0, [1, 2, 3], n)]
    # a second batch on the filled trunk: 'who?' keeps all of it, 'zzz' only up to the question's first character -> two forks
    eng.log.clear()
    s.ask_many(['who?', 'zzz', 'why?'], GEN)
    assert [e for e in eng.log if e[0] == 'fork'] == [('fork', 0, [1, 3], n), ('fork', 0, [2], n - 2)]
    assert not prefills(eng) and s.kv.length(0) == n


def test_the_two_cache_operations_check_their_arguments_without_a_gpu():
    from callireader_amd import _binding as B
    for name in ('cr_kv_truncate', 'cr_kv_fork'):
        assert name in B.SIGNATURES and hasattr(B.lib, name)
    assert B.lib.cr_kv_truncate(None, 0, 0, None) == -1 and b'cr_kv_truncate' in B.lib.cr_last_error()
    assert B.lib.cr_kv_fork(None, 0, None, 1, 1, None) == -1 and b'cr_kv_fork' in B.lib.cr_last_error()

"""Logits constraints, host side: constraints.parse's values, defaults and errors, the EOS-kept-in-whitelist rule, what stays NotImplementedError
(do_sample, beams, the sharded entry points, callable constraints), and that cr_kv_set_constraints refuses bad values before it refuses a missing cache."""
import ctypes as C

import pytest

from callireader_amd import constraints as K


def test_parse_defaults_and_values():
    assert K.parse({}) is None
    assert K.parse(dict(max_new_tokens=8, do_sample=False, num_beams=1, no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None,
                        begin_suppress_tokens=None, min_new_tokens=None, min_length=0, allowed_token_ids=None)) is None
    assert K.parse(dict(min_new_tokens=5)) is None                                   # no EOS id: nothing to ban
    c = K.parse(dict(no_repeat_ngram_size=3, bad_words_ids=[[5], [1, 2, 3]], suppress_tokens=[9, 8], begin_suppress_tokens=[4], min_new_tokens=2,
                     min_length=6, eos_token_id=7))
    assert c == K.Constraints(3, ((5,), (1, 2, 3)), (9, 8), (4,), 6, None, 7) and c.active
    assert c.banned_static(12) == [5, 8, 9]
    assert K.parse(dict(min_length=2, min_new_tokens=4), eos_token_id=1).min_new_tokens == 4
    assert K.parse(dict(no_repeat_ngram_size=2, eos_token_id=3), eos_token_id=None).eos_token_id is None       # the caller's EOS id wins
    assert K.parse(dict(sequence_bias={(1, 2): float('-inf')})).bad_words_ids == ((1, 2),)
    hash(c)                                                                          # frozen: usable as a key
    with pytest.raises(Exception):
        c.no_repeat_ngram_size = 1


def test_whitelist_always_keeps_the_eos_id():
    c = K.parse(dict(allowed_token_ids=[3, 4], eos_token_id=9))
    assert c.allowed_token_ids == (3, 4, 9)
    assert c.banned_static(11) == [0, 1, 2, 5, 6, 7, 8, 10]
    assert K.parse(dict(allowed_token_ids=[3, 9]), eos_token_id=9).allowed_token_ids == (3, 9)
    assert K.parse(dict(allowed_token_ids=[3, 4]), eos_token_id=None).allowed_token_ids == (3, 4)


@pytest.mark.parametrize('kw, text', [
    (dict(no_repeat_ngram_size=-1), '`ngram_size` has to be a strictly positive integer, but is -1'),
    (dict(no_repeat_ngram_size=2.5), '`ngram_size` has to be a strictly positive integer'),
    (dict(bad_words_ids=[]), '`bad_words_ids` has to be a non-empty list, but is [].'),
    (dict(bad_words_ids=[3]), '`bad_words_ids` has to be a list of lists, but is [3].'),
    (dict(bad_words_ids=[[3], []]), 'Each list in `bad_words_ids` has to be a list of positive integers, but is [[3], []].'),
    (dict(bad_words_ids=[[3, -1]]), 'Each list in `bad_words_ids` has to be a list of positive integers'),
    (dict(min_new_tokens=-2), '`min_new_tokens` has to be a positive integer, but is -2'),
    (dict(min_length=-1), '`min_length` has to be a non-negative integer, but is -1'),
    (dict(suppress_tokens=[1, -4]), '`suppress_tokens`'),
    (dict(begin_suppress_tokens=['a']), '`begin_suppress_tokens`'),
    (dict(allowed_token_ids=[]), '`allowed_token_ids`'),
])
def test_parse_errors_carry_transformers_texts(kw, text):
    with pytest.raises(ValueError) as e:
        K.parse(kw)
    assert text in str(e.value)


def test_transformers_raises_the_same_texts():
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor
    for make, kw in ((lambda: NoRepeatNGramLogitsProcessor(-1), dict(no_repeat_ngram_size=-1)),
                     (lambda: NoBadWordsLogitsProcessor([], eos_token_id=0), dict(bad_words_ids=[])),
                     (lambda: NoBadWordsLogitsProcessor([3], eos_token_id=0), dict(bad_words_ids=[3]))):
        with pytest.raises(ValueError) as hf:
            make()
        with pytest.raises(ValueError) as ours:
            K.parse(kw)
        assert str(ours.value) == str(hf.value)


@pytest.mark.parametrize('kw', [dict(prefix_allowed_tokens_fn=lambda b, ids: [1]), dict(encoder_no_repeat_ngram_size=2), dict(force_words_ids=[[1]]),
                                dict(sequence_bias={(1,): -2.0})])
def test_still_not_implemented_says_so(kw):
    with pytest.raises(NotImplementedError, match='not implemented'):
        K.parse(kw)


def test_greedy_only():
    from callireader_amd import sampling as S
    with pytest.raises(NotImplementedError):
        S.parse(dict(do_sample=True, no_repeat_ngram_size=3))                        # unchanged: sampling.UNSUPPORTED
    assert 'no_repeat_ngram_size' in S.UNSUPPORTED and 'bad_words_ids' in S.UNSUPPORTED and 'suppress_tokens' in S.UNSUPPORTED
    for kw in (dict(no_repeat_ngram_size=3), dict(min_new_tokens=4, eos_token_id=2), dict(allowed_token_ids=[1, 2])):
        with pytest.raises(NotImplementedError, match='do_sample'):
            K.parse(dict(kw, do_sample=True))
        with pytest.raises(NotImplementedError, match='num_beams=3'):
            K.parse(dict(kw, num_beams=3))
    assert K.parse(dict(do_sample=True, temperature=0.7)) is None


def test_gen_args_is_still_a_3_tuple_and_entry_points_refuse():
    from callireader_amd import parallel
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    out = InternVLChatModel._gen_args(dict(max_new_tokens=9, no_repeat_ngram_size=3, eos_token_id=5))
    assert out == (9, 5, None)
    with pytest.raises(NotImplementedError, match='constraints'):
        parallel.chat_ocr_pages_sharded(None, None, None, [], 'q', dict(no_repeat_ngram_size=3))
    with pytest.raises(NotImplementedError, match='constraints'):
        parallel.sharded_generate(None, [], [], [], img_id=0, ref_id=0, max_new_tokens=4, min_new_tokens=2, eos_token_id=1)
    with pytest.raises(NotImplementedError, match='do_sample'):
        next(InternVLChatModel.chat_ocr_stream(None, None, None, [], 'q', dict(do_sample=True, min_new_tokens=3)))
    with pytest.raises(NotImplementedError, match='num_beams'):
        InternVLChatModel.chat_ocr_pages(None, None, None, [], 'q', dict(num_beams=2, bad_words_ids=[[1]]))
    with pytest.raises(NotImplementedError, match='prefix_allowed_tokens_fn'):
        InternVLChatModel.chat_ocr_pages(None, None, None, [], 'q', dict(prefix_allowed_tokens_fn=lambda b, i: [0]))


def test_per_page():
    c = K.Constraints(no_repeat_ngram_size=2)
    assert K.per_page(None, 3) == [None] * 3
    assert K.per_page(c, 2) == [c, c]
    assert K.per_page([c, None, K.Constraints()], 3) == [c, None, None]              # an inactive entry is no constraint
    with pytest.raises(ValueError):
        K.per_page([c], 2)
    with pytest.raises(TypeError):
        K.per_page([dict(no_repeat_ngram_size=2)], 1)


def _struct(**kw):
    from callireader_amd.engine import c_constraints
    return c_constraints(K.Constraints(**kw))


def test_abi_refuses_bad_values_before_the_missing_cache():
    from callireader_amd import _binding as B
    call = lambda c: (B.lib.cr_kv_set_constraints(None, 0, C.byref(c), None), B.lib.cr_last_error().decode())
    good, keep = _struct(no_repeat_ngram_size=3, suppress_tokens=(1, 2), bad_words_ids=((4, 5), (6,)))
    code, msg = call(good)
    assert code == -1 and 'bad sequence' in msg                                      # good values: the missing cache is what is refused
    assert B.lib.cr_kv_set_constraints(None, 0, None, None) == -1 and 'bad sequence' in B.lib.cr_last_error().decode()
    for field, value, word in (('no_repeat_ngram_size', -1, 'no_repeat_ngram_size'), ('min_new_tokens', -3, 'min_new_tokens'),
                               ('n_suppress', -1, 'count')):
        c, keep = _struct(suppress_tokens=(1,))
        setattr(c, field, value)
        code, msg = call(c)
        assert code == -1 and word in msg and 'bad sequence' not in msg, (field, msg)
    c, keep = _struct(suppress_tokens=(1, 2))
    keep[0][1] = -7                                                                  # an id below 0
    code, msg = call(c)
    assert code == -1 and 'suppress id -7' in msg
    c, keep = _struct(bad_words_ids=((4, 5), (6,)))
    keep[4][1] = 0                                                                   # offsets 0, 0, 3: the first word is empty
    code, msg = call(c)
    assert code == -1 and 'empty' in msg
    c, keep = _struct(bad_words_ids=(tuple(range(17)),))                             # one word past the 16-id limit
    code, msg = call(c)
    assert code == -1 and '17 ids' in msg
    c, keep = _struct(bad_words_ids=tuple((i, i + 1) for i in range(257)))           # 257 multi-id words
    code, msg = call(c)
    assert code == -1 and '256' in msg
    c, keep = _struct(bad_words_ids=tuple((i,) for i in range(5000)))                # one-id words live in the mask: no limit
    assert 'bad sequence' in call(c)[1]
    # the op entry checks the same values, then the vocabulary, before any device call
    c, keep = _struct(suppress_tokens=(100,))
    assert B.lib.cr_op_constrain(C.byref(c), None, 1, 50, None, None, 0, None, None) == -1 and 'bad argument' in B.lib.cr_last_error().decode()
    fake = C.c_void_p(16)                                                            # never dereferenced: the vocabulary check comes first
    assert B.lib.cr_op_constrain(C.byref(c), fake, 1, 50, None, None, 0, fake, None) == -1 and 'suppress id 100' in B.lib.cr_last_error().decode()

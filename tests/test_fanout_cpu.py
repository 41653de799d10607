"""num_return_sequences, host side: the parsing (transformers' texts), the seed layout, the 64-row limit, the argument checks cr_kv_fanout makes before
it touches a device, and which entry points refuse the keyword -- on the stub engine of tests/engine_stubs.py, which here also fans out."""
import ctypes as C

import pytest
import torch

from callireader_amd import sampling as S
from engine_stubs import StubEngine, StubKV, make_model, make_session

GREEDY_TEXT = 'Greedy methods without beam search do not support `num_return_sequences` different than 1 (got 4).'     # transformers 4.45.2, GenerationConfig.validate
SP = S.SamplingParams(0.7, 5, 0.8)


def gen_args(**kw):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    return InternVLChatModel._gen_args(kw, allow_returns=True)


def test_parse():
    assert 'num_return_sequences' not in S.UNSUPPORTED
    assert S.parse_returns({}) == 1 and S.parse_returns(dict(num_return_sequences=None)) == 1 and S.parse_returns(dict(num_return_sequences=1)) == 1
    assert S.parse_returns(dict(do_sample=True, num_return_sequences=4)) == 4
    sp = S.parse(dict(do_sample=True, num_return_sequences=4, top_k=7))
    assert isinstance(sp, S.SamplingParams) and sp.top_k == 7                       # parse keeps returning the SamplingParams ...
    max_new, eos, sp = gen_args(do_sample=True, num_return_sequences=4, max_new_tokens=9)
    assert max_new == 9 and (sp.temperature, sp.top_k, sp.top_p) == (1.0, 50, 1.0)   # ... and _gen_args its three values
    for kw in (dict(num_return_sequences=4), dict(num_return_sequences=4, do_sample=False), dict(num_return_sequences=4, do_sample=False, num_beams=1)):
        for fn in (S.parse, S.parse_returns, lambda k: gen_args(**k)):
            with pytest.raises(ValueError) as e:
                fn(kw)
            assert str(e.value) == GREEDY_TEXT
    for bad in (0, -1, 2.0, '2', True):
        with pytest.raises(ValueError, match='`num_return_sequences` has to be a positive integer'):
            S.parse(dict(do_sample=True, num_return_sequences=bad))
    with pytest.raises(NotImplementedError):                                       # beam n-best stays refused (tests/test_beam_cpu.py pins it)
        S.parse(dict(num_beams=2, num_return_sequences=2))
    with pytest.raises(NotImplementedError, match='one answer per page'):           # a caller that has no fan-out path
        from callireader_amd.modeling_internvl_chat import InternVLChatModel
        InternVLChatModel._gen_args(dict(do_sample=True, num_return_sequences=2))


def test_seed_layout():
    P, n, base = 3, 4, 1234
    flat = S.page_seeds(P * n, base)
    fan = S.fan_seeds(P, n, base)
    assert [len(r) for r in fan] == [n] * P
    assert all(fan[i][j] == flat[i * n + j] == S.splitmix64(base + i * n + j) for i in range(P) for j in range(n))
    assert [r[0] for r in S.fan_seeds(5, 1, base)] == S.page_seeds(5, base)          # n = 1: today's seeds
    torch.manual_seed(9)
    a = S.fan_seeds(2, 3)
    torch.manual_seed(9)
    flat = S.page_seeds(6)
    assert a == [flat[:3], flat[3:]] and len(set(flat)) == 6                         # one base seed per call, drawn from torch's generator


def test_64_rows():
    S.check_rows(8, 8)
    S.check_rows(64, 1)
    S.check_rows(1, 64)
    for P, n in ((65, 1), (13, 5), (1, 65), (9, 8)):
        with pytest.raises(ValueError, match='at most 64'):
            S.check_rows(P, n)


def test_abi_refuses_bad_arguments_without_a_device():
    from callireader_amd import _binding as B
    one, seed = (C.c_int32 * 1)(1), (C.c_uint64 * 1)(7)
    assert B.lib.cr_kv_fanout(None, 0, one, 1, seed, None, None) == -1
    assert b'cr_kv_fanout' in B.lib.cr_last_error()
    assert B.lib.cr_kv_fanout(None, 0, None, 1, seed, None, None) == -1
    assert B.lib.cr_kv_fanout(None, -1, one, 0, None, None, None) == -1
    assert B.ABI_VERSION == 13 and B.lib.cr_abi_version() == 13                     # an addition within the ABI


class FanKV(StubKV):
    def fanout(self, src, dsts, seeds, last_logits):
        assert len(self.gen[src]) == 1 and src not in dsts and len(set(dsts)) == len(dsts) == len(seeds) and last_logits is not None
        self.log.append(('fanout', src, list(dsts), list(seeds)))
        for d, sd in zip(dsts, seeds):
            self.len[d], self.gen[d] = self.len[src], [sd % 1000]


class FanEngine(StubEngine):
    def kv_alloc(self, n_seqs, max_tokens, dtype='bf16'):
        self.kvs.append(FanKV(n_seqs, max_tokens, self.log))
        return self.kvs[-1]

    def prefill_batch(self, kv, seqs, embeds_list, penalty=1.0, want_logits=False):
        super().prefill_batch(kv, seqs, embeds_list, penalty)
        return torch.zeros(len(seqs), 4) if want_logits else None


def fan_model(**kw):
    m = make_model(**kw)
    m.engine = FanEngine()
    m.kv = lambda n=None: m.engine.kv_alloc(n or 1, 512)
    return m


def test_generate_pages_fans_out_on_the_stub():
    m = fan_model()
    pages = [torch.zeros(5, 8), torch.zeros(9, 8)]
    seeds = [100, 101, 102, 200, 201, 202]
    out = m.generate_pages(pages, max_new_tokens=3, eos_token_id=None, sampling=SP, seeds=seeds, num_return_sequences=3)
    assert [[o[0] for o in page] for page in out] == [[77, 101, 102], [77, 201, 202]] and all(len(o) == 3 for page in out for o in page)
    log = m.engine.log
    assert [e for e in log if e[0] == 'prefill_batch'] == [('prefill_batch', [0, 3], [5, 9])]                    # one prefill per page
    assert [e for e in log if e[0] == 'fanout'] == [('fanout', 0, [1, 2], [101, 102]), ('fanout', 3, [4, 5], [201, 202])]
    assert [e for e in log if e[0] == 'decode'] == [('decode', [0, 1, 2, 3, 4, 5])] * 2                          # all P * n rows as one batch per step
    ids, sc = m.generate_pages(pages, max_new_tokens=3, eos_token_id=None, sampling=SP, seeds=seeds, num_return_sequences=3, logprobs=1)
    assert ids == out and [len(s) for s in sc] == [3, 3] and len(sc[1][2].logprobs) == 3
    with pytest.raises(ValueError, match='seeds: 5 entries'):
        m.generate_pages(pages, max_new_tokens=3, sampling=SP, seeds=seeds[:5], num_return_sequences=3)
    with pytest.raises(ValueError, match='at most 64'):
        m.generate_pages([pages[0]] * 13, max_new_tokens=3, sampling=SP, num_return_sequences=5)
    m.generate_pages([pages[0]] * 8, max_new_tokens=2, eos_token_id=None, sampling=SP, num_return_sequences=8)    # P * n = 64 is taken
    t = m._generate_kw(pages[0], 1.0, dict(do_sample=True, num_return_sequences=2, max_new_tokens=3, eos_token_id=None))
    assert t.shape == (2, 3) and t.dtype == torch.long


def test_what_refuses_the_keyword():
    from callireader_amd import parallel
    from callireader_amd.constraints import Constraints
    m = fan_model()
    page = torch.zeros(5, 8)
    kw = dict(max_new_tokens=4, sampling=SP, num_return_sequences=2)
    with pytest.raises(ValueError) as e:
        m.generate_pages([page], max_new_tokens=4, num_return_sequences=4)
    assert str(e.value) == GREEDY_TEXT
    with pytest.raises(ValueError, match='Greedy methods'):
        m.generate_pages([page, page], max_new_tokens=4, sampling=[SP, None], num_return_sequences=2)            # a greedy page among them
    with pytest.raises(NotImplementedError):
        m.generate_pages([page], max_new_tokens=4, num_beams=2, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match='not implemented with a draft'):
        m.generate_pages([page], drafts=[[1, 2]], **kw)
    with pytest.raises(NotImplementedError, match='constraints'):
        m.generate_pages([page], constraints=Constraints(no_repeat_ngram_size=2), **kw)
    with pytest.raises(NotImplementedError, match='not implemented with a draft'):
        m._generate_kw(page, 1.0, dict(do_sample=True, num_return_sequences=2, max_new_tokens=4, draft_ids=[1, 2]))
    with pytest.raises(NotImplementedError, match='page session'):
        m._generate_kw(page, 1.0, dict(do_sample=True, num_return_sequences=2, max_new_tokens=4), kv=None, seq=0, reset=False)
    m8 = fan_model(kv_cache_dtype='e4m3')
    with pytest.raises(NotImplementedError, match='e4m3'):
        m8.generate_pages([page], **kw)
    with pytest.raises(NotImplementedError, match='e4m3'):
        m8.chat_ocr(None, None, None, 'q', dict(do_sample=True, num_return_sequences=2))
    gc = dict(max_new_tokens=4, do_sample=True, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match='PagePipeline'):
        next(m.chat_ocr_stream(None, None, [], 'q', gc))
    with pytest.raises(NotImplementedError, match='ContinuousPipeline'):
        next(m.chat_ocr_continuous(None, None, [], 'q', gc))
    with pytest.raises(NotImplementedError, match='sharded'):
        parallel.sharded_generate(m, [], [], [], img_id=1, ref_id=2, max_new_tokens=4, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match='sharded'):
        parallel.chat_ocr_pages_sharded(m, None, None, [], 'q', gc)
    sess, _ = make_session()
    for call in (lambda: sess.chat_ocr('q', gc), lambda: sess.ask_many(['q'], gc)):
        with pytest.raises(NotImplementedError, match='num_return_sequences'):
            call()
    assert sess.kv.len[0] == 0                                                      # a refused turn leaves the trunk as it was

"""Shared prompts (share_prompt=, KVCache.fork_shared / set_prefix_sharing) without a GPU: the keyword's parsing, the refusals made in Python, the
host's reset order over tests/engine_stubs.py, and the header / binding pair of the new symbols."""
import os
import re

import pytest
import torch

from engine_stubs import HID, StubEngine, StubKV, make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_share():
    from callireader_amd.sampling import parse_share
    assert parse_share({}) is False and parse_share({'share_prompt': None}) is False
    assert parse_share({'share_prompt': True}) is True and parse_share({'share_prompt': False}) is False
    for bad in (1, 0, 'yes', 'true', [True], 1.0):
        with pytest.raises(ValueError, match='share_prompt'):
            parse_share({'share_prompt': bad})


def test_cli_flag():
    from callireader_amd.inference import build_parser
    p = build_parser()
    base = ['--tgt', 'x.jpg'] if any(a.dest == 'tgt' and a.required for a in p._actions) else []
    assert p.parse_args(base).share_prompt is False
    assert p.parse_args(base + ['--share_prompt']).share_prompt is True


def test_entry_points_that_own_their_caches_refuse_the_keyword():
    m = make_model()
    gc = dict(max_new_tokens=4, share_prompt=True)
    with pytest.raises(NotImplementedError, match='share_prompt=True is not implemented with this entry point'):
        m._gen_args(dict(gc))                                            # what the pipelines, the sharded entry points, page sessions and chat parse with
    assert m._gen_args(dict(gc), allow_beams=True, allow_returns=True)[0] == 4      # the entry points that fan a page out take it
    with pytest.raises(ValueError, match='share_prompt'):
        m._gen_args(dict(max_new_tokens=4, share_prompt='on'), allow_returns=True) and m._generate_kw(torch.zeros(3, HID), 1.0, dict(share_prompt='on'))
    for name, args in (('chat_ocr_stream', (None, None, [], 'q', gc)), ('chat_ocr_continuous', (None, None, [], 'q', gc))):
        with pytest.raises(NotImplementedError, match='share_prompt=True is not implemented with (PagePipeline|ContinuousPipeline)'):
            out = getattr(m, name)(*args)
            if hasattr(out, '__next__'):
                next(out)
    emb = torch.zeros(3, HID)
    with pytest.raises(NotImplementedError, match='a draft'):
        m._generate_kw(emb, 1.0, dict(max_new_tokens=2, share_prompt=True, draft_ids=[1, 2]))
    with pytest.raises(NotImplementedError, match='a page session'):
        m._generate_kw(emb, 1.0, dict(max_new_tokens=2, share_prompt=True), kv=object(), seq=0, reset=False)
    with pytest.raises(NotImplementedError, match='drafts'):
        m.generate_pages([emb], max_new_tokens=2, share_prompt=True, drafts=[[1]])
    with pytest.raises(ValueError, match='share_prompt'):
        m.generate_pages([emb], max_new_tokens=2, share_prompt=1)
    e4 = make_model(kv_cache_dtype='e4m3')
    with pytest.raises(NotImplementedError, match="kv_cache_dtype='e4m3'"):
        e4.generate_pages([emb], max_new_tokens=2, share_prompt=True)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype='e4m3'"):
        e4._generate_kw(emb, 1.0, dict(max_new_tokens=2, share_prompt=True))
    with pytest.raises(NotImplementedError, match="kv_cache_dtype='e4m3'"):
        e4.chat_ocr_pages(None, None, [], 'q', dict(max_new_tokens=2), share_prompt=True)


class SharingKV(StubKV):
    """StubKV with the calls of the fan-out and beam paths: it logs them, and refuses a reset of a source that still has sharers, as the cache does."""

    def __init__(self, *a):
        super().__init__(*a)
        self.prefix_sharing, self.src_of = False, {}

    def set_prefix_sharing(self, on=True):
        assert not any(self.len) and not self.src_of
        self.log.append(('set_prefix_sharing', bool(on)))
        self.prefix_sharing = bool(on)

    def reset(self, seq=-1):
        if seq >= 0:
            assert seq not in self.src_of.values(), f'reset of source {seq} before its sharers'
            self.src_of.pop(seq, None)
        else:
            self.src_of.clear()
        super().reset(seq)

    def fanout(self, src, dsts, seeds, row):
        self.log.append(('fanout', src, list(dsts)))
        for d in dsts:
            self.len[d], self.gen[d] = self.len[src], [55]
            if self.prefix_sharing:
                self.src_of[d] = src

    def set_beam(self, first, B, *a):
        self.log.append(('set_beam', first, B))
        self.beams = getattr(self, 'beams', {})
        self.beams[first] = B

    def beam_result(self, first):
        return [7, 8], -1.0, True


class SharingEngine(StubEngine):
    def kv_alloc(self, n_seqs, max_tokens, dtype='bf16'):
        self.kvs.append(SharingKV(n_seqs, max_tokens, self.log))
        return self.kvs[-1]

    def prefill_batch(self, kv, seqs, embeds_list, penalty=1.0, want_logits=False):
        super().prefill_batch(kv, seqs, embeds_list, penalty)
        for s in seqs:                                                   # a beam group's fan-out
            for j in range(1, getattr(kv, 'beams', {}).get(s, 1)):
                kv.len[s + j], kv.gen[s + j] = kv.len[s], list(kv.gen[s])
                if kv.prefix_sharing:
                    kv.src_of[s + j] = s
        return [None] * len(seqs)


def sharing_model():
    m = make_model()
    m.engine = SharingEngine()
    m.max_pages = 8
    m.kv = lambda n=None: m.engine.kvs[0] if m.engine.kvs else m.engine.kv_alloc(8, 512)
    return m


def test_fanout_call_shares_then_resets_sharers_before_sources():
    from callireader_amd.sampling import SamplingParams
    m = sharing_model()
    emb = [torch.zeros(300, HID), torch.zeros(280, HID)]
    kw = dict(max_new_tokens=3, eos_token_id=None, sampling=SamplingParams(0.7, 5, 0.8), num_return_sequences=3)
    ids = m.generate_pages(emb, share_prompt=True, **kw)
    log = m.engine.log
    assert [len(p) for p in ids] == [3, 3]
    assert log[0] == ('reset', -1) and log[1] == ('set_prefix_sharing', True)
    tail = [e for e in log if e[0] in ('reset', 'set_prefix_sharing')][2:]
    assert tail == [('reset', 1), ('reset', 2), ('reset', 4), ('reset', 5), ('reset', 0), ('reset', 3), ('set_prefix_sharing', False)]
    assert not m.engine.kvs[0].src_of and not m.engine.kvs[0].prefix_sharing
    # the same call without the keyword issues none of it, and gives the same ids
    m.engine.log.clear()
    assert m.generate_pages(emb, **kw) == ids
    assert [e for e in m.engine.log if e[0] in ('reset', 'set_prefix_sharing')] == [('reset', -1)]


def test_beam_call_shares_then_resets_sharers_before_sources():
    m = sharing_model()
    emb = [torch.zeros(300, HID), torch.zeros(280, HID)]
    m.generate_pages(emb, max_new_tokens=2, eos_token_id=None, num_beams=2, share_prompt=True)
    marks = [e for e in m.engine.log if e[0] in ('reset', 'set_prefix_sharing')]
    assert marks == [('reset', -1), ('set_prefix_sharing', True), ('reset', 1), ('reset', 3), ('reset', 0), ('reset', 2), ('set_prefix_sharing', False)]
    m.engine.log.clear()
    m.generate_pages(emb, max_new_tokens=2, eos_token_id=None, num_beams=2)
    assert [e for e in m.engine.log if e[0] in ('reset', 'set_prefix_sharing')] == [('reset', -1)]


def test_one_row_per_page_accepts_the_keyword_and_does_nothing():
    m = sharing_model()
    emb = [torch.zeros(5, HID)]
    a = m.generate_pages(emb, max_new_tokens=3, eos_token_id=None, share_prompt=True)
    log_a = list(m.engine.log)
    m.engine.log.clear()
    b = m.generate_pages(emb, max_new_tokens=3, eos_token_id=None)
    assert a == b and log_a == m.engine.log and not any(e[0] == 'set_prefix_sharing' for e in log_a)


def test_header_and_binding_hold_the_new_symbols():
    from callireader_amd import _binding as B
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'callireader_hip.h')).read(), flags=re.S)
    for name, n_args in (('cr_kv_fork_shared', 6), ('cr_kv_set_prefix_sharing', 2), ('cr_op_decode_attention_shared', 14)):
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)', src)
        assert m and len(m.group(1).split(',')) == n_args, name
        assert len(B.SIGNATURES[name][1]) == n_args and hasattr(B.lib, name)
    assert B.SIGNATURES['cr_kv_fork_shared'] == B.SIGNATURES['cr_kv_fork']                  # cr_kv_fork's signature
    assert B.ABI_VERSION == 13 and B.lib.cr_abi_version() == 13                             # additions within v13
    # argument checks happen before any device call
    assert B.lib.cr_kv_set_prefix_sharing(None, 1) == -1 and b'cr_kv_set_prefix_sharing' in B.lib.cr_last_error()
    assert B.lib.cr_kv_fork_shared(None, 0, None, 1, 1, None) == -1 and b'cr_kv_fork_shared' in B.lib.cr_last_error()
    assert B.lib.cr_op_decode_attention_shared(None, None, None, 8, None, None, None, None, 1, 8, 1.0, None, None, None) == -1

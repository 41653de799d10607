"""num_return_sequences at the generation level (generate_pages, generate_ocr): sample j of page i is EXACTLY what a lone call for page i with seed
s(i, j) returns -- ids and, with logprobs, every score bit -- from one prefill per page.  Both sides draw with the same noise from the same bits (a
decode row's bits do not depend on its batch), so the comparison is exact and no tie caveat applies."""
import numpy as np
import pytest
import torch

from callireader_amd import sampling as S
from callireader_amd import synthetic
from callireader_amd.config import ModelDims

pytestmark = pytest.mark.gpu

V = 9000
SP = S.SamplingParams(0.9, 40, 0.95)
GEN = dict(max_new_tokens=24, eos_token_id=None, repetition_penalty=1.5)


@pytest.fixture(scope='module')
def llm():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=V)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=3), dims, max_tokens=512, max_pages=64)
    g = torch.Generator().manual_seed(1)
    ids = [torch.randint(0, V, (n,), generator=g) for n in (5, 64, 250)]
    pages = [m.engine.embed_splice(i) for i in ids]
    m.img_context_token_id = 8990                 # generate_ocr asserts that a tokenizer has set it
    yield m, pages, ids
    m.close()


def lone(m, page, seed, **kw):
    return m.generate_pages([page], **dict(GEN, **kw), sampling=SP, seeds=[seed])


def same_scores(a, b):
    return all(np.array_equal(x, y) for x, y in ((a.logprobs, b.logprobs), (a.top_ids, b.top_ids), (a.top_logprobs, b.top_logprobs)))


@pytest.mark.parametrize('P,n', [(3, 4), (1, 8)])
def test_samples_equal_lone_calls(llm, P, n):
    m, pages, _ = llm
    pages = pages[:P] if P > 1 else pages[1:2]
    seeds = [S.splitmix64(77 + k) for k in range(P * n)]
    out = m.generate_pages(pages, **GEN, sampling=SP, seeds=seeds, num_return_sequences=n)
    assert len(out) == P and all(len(o) == n for o in out)
    for i in range(P):
        for j in range(n):
            assert out[i][j] == lone(m, pages[i], seeds[i * n + j])[0], (i, j)
        assert len({tuple(o) for o in out[i]}) > 1                                  # different seeds, different answers
    ids, sc = m.generate_pages(pages, **GEN, sampling=SP, seeds=seeds, num_return_sequences=n, logprobs=2)
    assert ids == out
    for i in range(P):
        for j in range(n):
            lids, lsc = lone(m, pages[i], seeds[i * n + j], logprobs=2)
            assert lids[0] == ids[i][j] and same_scores(sc[i][j], lsc[0]), (i, j)
            assert sc[i][j].top_ids.shape == (len(ids[i][j]), 2)


def test_one_prefill_per_page(llm, monkeypatch):
    from callireader_amd import _binding as B
    m, pages, _ = llm
    rows, calls = [], []
    real = m.engine.prefill_batch

    def counted(kv, seqs, embeds_list, **kw):
        rows.extend(e.shape[0] for e in embeds_list)
        return real(kv, seqs, embeds_list, **kw)
    monkeypatch.setattr(m.engine, 'prefill_batch', counted)

    real_lib = B.lib

    class Lib:
        """the library with its prefill entry points counted"""
        def __getattr__(self, name):
            fn = getattr(real_lib, name)
            if not name.startswith('cr_llm_prefill'):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    import callireader_amd.engine as E
    monkeypatch.setattr(E.B, 'lib', Lib())
    m.generate_pages(pages, **GEN, sampling=SP, seeds=list(range(12)), num_return_sequences=4)
    assert sorted(rows) == [5, 64, 250]                                            # the rows prefilled: sum of S_i, not n * sum of S_i
    assert calls == ['cr_llm_prefill_batch']                                       # and no prefill call after the first


def test_early_stops_and_padding(llm):
    m, pages, ids = llm
    page = pages[1]
    n = 6
    seeds = [S.splitmix64(500 + k) for k in range(n)]
    free = m.generate_pages([page], **GEN, sampling=SP, seeds=seeds, num_return_sequences=n)[0]
    eos = free[2][3]                                                               # an id sample 2 draws at its fourth step: it stops there
    gen = dict(GEN, eos_token_id=eos)
    out = m.generate_pages([page], **gen, sampling=SP, seeds=seeds, num_return_sequences=n)[0]
    assert out[2] == free[2][:free[2].index(eos) + 1] and len(out[2]) <= 4
    lens = [len(o) for o in out]
    assert len(set(lens)) > 1 and all(eos not in o[:-1] for o in out)              # unpadded, each cut at its own stop
    for j in range(n):
        assert out[j] == m.generate_pages([page], **gen, sampling=SP, seeds=[seeds[j]])[0], j       # an early stop does not change the siblings' ids
    # generate_ocr: the [n, L] tensor, right-padded with the pad id (the EOS id by default)
    kw = dict(repetition_penalty=GEN['repetition_penalty'], max_new_tokens=GEN['max_new_tokens'], eos_token_id=eos, do_sample=True,
              temperature=SP.temperature, top_k=SP.top_k, top_p=SP.top_p, num_return_sequences=n)
    torch.manual_seed(11)
    t = m.generate_ocr(input_ids=ids[1][None], **kw)
    torch.manual_seed(11)
    want = m.generate_pages([page], **gen, sampling=SP, seeds=S.page_seeds(n), num_return_sequences=n)[0]
    assert t.shape == (n, max(len(w) for w in want)) and t.dtype == torch.long
    for j, w in enumerate(want):
        assert t[j, :len(w)].tolist() == w and t[j, len(w):].tolist() == [eos] * (t.shape[1] - len(w))
    torch.manual_seed(11)
    o = m.generate_ocr(input_ids=ids[1][None], **kw, pad_token_id=0, return_dict_in_generate=True, output_scores=True, top_logprobs=2)
    assert o.sequences.shape == t.shape and isinstance(o.scores, list) and len(o.scores) == len(o.token_logprobs) == len(o.top_ids) == n
    for j, w in enumerate(want):
        assert o.sequences[j, :len(w)].tolist() == w and o.sequences[j, len(w):].tolist() == [0] * (t.shape[1] - len(w))
        assert o.token_logprobs[j].shape == (len(w),) and o.top_ids[j].shape == (len(w), 2)


def test_n_1_is_unchanged(llm):
    m, pages, ids = llm
    kw = dict(repetition_penalty=1.5, max_new_tokens=12, eos_token_id=None, do_sample=True, top_k=30)
    torch.manual_seed(5)
    a = m.generate_ocr(input_ids=ids[0][None], **kw)
    torch.manual_seed(5)
    b = m.generate_ocr(input_ids=ids[0][None], **kw, num_return_sequences=1)
    assert type(a) is type(b) and a.shape == b.shape == (1, 12) and torch.equal(a, b)
    torch.manual_seed(5)
    p = m.generate_pages(pages, **GEN, sampling=SP)
    torch.manual_seed(5)
    q = m.generate_pages(pages, **GEN, sampling=SP, num_return_sequences=1)
    assert p == q and isinstance(q[0][0], int)                                     # a list of id lists, not nested
    with pytest.raises(ValueError, match='Greedy methods without beam search do not support `num_return_sequences` different than 1'):
        m.generate_pages(pages, **GEN, num_return_sequences=2)


def test_64_rows_run(llm):
    m, pages, _ = llm
    eight = [pages[0]] * 8
    seeds = list(range(64))
    out = m.generate_pages(eight, max_new_tokens=4, eos_token_id=None, repetition_penalty=1.5, sampling=SP, seeds=seeds, num_return_sequences=8)
    assert len(out) == 8 and all(len(o) == 8 and all(len(x) == 4 for x in o) for o in out)
    assert out[3][5] == m.generate_pages([pages[0]], max_new_tokens=4, eos_token_id=None, repetition_penalty=1.5, sampling=SP, seeds=[29])[0]
    with pytest.raises(ValueError, match='at most 64'):
        m.generate_pages(eight + [pages[0]], max_new_tokens=4, sampling=SP, num_return_sequences=8)

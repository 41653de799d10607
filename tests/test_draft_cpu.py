"""Host side of draft-verified decoding without a GPU: draft.py's cursor and row cap, generation.decode_rows_drafted against a stub engine whose
decode_draft accepts exactly what cr_llm_decode_draft accepts, and the combinations the entry points refuse."""
import pytest
import torch

from engine_stubs import StubEngine, StubKV, make_model, make_session, EOS

from callireader_amd import draft as D
from callireader_amd.generation import decode_rows, decode_rows_drafted


class DraftKV(StubKV):
    format = 'bf16'


class DraftEngine(StubEngine):
    """decode_draft: the scripted ids are what the model picks; a drafted id is kept while it equals the pick, then the pick itself is appended"""

    def kv_alloc(self, n_seqs, max_tokens, dtype='bf16'):
        self.kvs.append(DraftKV(n_seqs, max_tokens, self.log))
        self.kvs[-1].format = dtype
        return self.kvs[-1]

    def decode_draft(self, kv, seqs, drafts, penalty=1.0):
        assert len(seqs) <= 64 and sum(len(d) + 1 for d in drafts) <= 64 and all(len(d) <= 7 for d in drafts)
        self.log.append(('decode_draft', list(seqs), [list(d) for d in drafts]))
        app = []
        for s, d in zip(seqs, drafts):
            assert kv.len[s] + len(d) + 1 <= kv.max_tokens
            n = 0
            while True:
                self._pick(kv, s)
                kv.len[s] += 1
                n += 1
                if n > len(d) or kv.gen[s][-1] != d[n - 1]:
                    break
            app.append(n)
        return app


def run(scripts, drafts, max_new, eos=None, budgets=None, max_tokens=512, prompt=10):
    """(ids per sequence, steps, the engine) of a drafted run: sequence i is prefilled, then picks scripts[i] in order"""
    eng = DraftEngine()
    kv = eng.kv_alloc(len(scripts), max_tokens)
    for i, s in enumerate(scripts):
        eng.script[i] = list(s)
        eng.prefill(kv, i, torch.zeros(prompt, 8))
    stats = {}
    outs = decode_rows_drafted(eng, kv, list(range(len(scripts))), max_new, eos, 1.0, drafts, budgets=budgets, stats=stats)
    return outs, stats, eng


def plain(scripts, max_new, eos=None, budgets=None):
    eng = StubEngine()
    kv = eng.kv_alloc(len(scripts), 512)
    for i, s in enumerate(scripts):
        eng.script[i] = list(s)
        eng.prefill(kv, i, torch.zeros(10, 8))
    return decode_rows(eng, kv, list(range(len(scripts))), max_new, eos, 1.0, budgets=budgets)


def steps_of(eng):
    return [e for e in eng.log if e[0] in ('decode_draft', 'decode')]


ANSWER = list(range(100, 140))


def test_exact_draft_takes_an_eighth_of_the_steps():
    outs, stats, eng = run([ANSWER], [ANSWER], max_new=40)
    assert outs == [ANSWER] == plain([ANSWER], 40)
    assert stats['steps'] == len(steps_of(eng)) == -(-39 // 8)
    assert stats['accepted'] == 39 - stats['steps'] and stats['drafted'] >= stats['accepted']


def test_eos_and_budget_cut_as_the_plain_loop_cuts():
    script = ANSWER[:20] + [EOS] + ANSWER[20:]
    for kw in (dict(max_new=40, eos=EOS), dict(max_new=13), dict(max_new=40, eos=EOS, budgets=[9])):
        outs, _, _ = run([script], [script], **kw)
        assert outs == plain([script], **kw), kw
    outs, _, eng = run([[EOS] + ANSWER], [ANSWER], max_new=40, eos=EOS)            # the prefill's own pick is EOS: no step at all
    assert outs == [[EOS]] and steps_of(eng) == []


def test_insertions_and_deletions_resynchronise():
    draft = ANSWER
    out = ANSWER[:10] + [900, 901] + ANSWER[10:20] + ANSWER[24:]                      # two ids inserted, four deleted
    outs, stats, _ = run([out], [draft], max_new=len(out))
    assert outs == [out]
    assert stats['steps'] < len(out) - 1 and stats['accepted'] >= 20                  # most of the draft still pays
    assert stats['steps'] + stats['accepted'] == len(out) - 1


def test_cursor_resynchronises_within_the_lookahead():
    c = D.DraftCursor(list(range(50)), lookahead=8)
    c.feed([0, 1, 2])
    assert c.window(7) == [3, 4, 5, 6, 7, 8, 9] and c.window(2) == [3, 4] and c.window(0) == []
    c.feed([77])                                      # not in the draft: out of step, nothing offered
    assert c.window(7) == []
    c.feed([78])
    assert c.window(7) == []
    c.feed([5])                                       # found ahead of the cursor: in step again behind it
    assert c.window(3) == [6, 7, 8]
    c.feed([30])                                      # beyond the look-ahead: stays out of step
    assert c.window(7) == []
    c.feed([9])
    assert c.window(2) == [10, 11]
    c.feed(list(range(10, 50)))
    assert c.window(7) == []                          # the draft is used up
    c.feed([3])
    assert c.window(7) == []


def test_a_wrong_draft_costs_one_step_per_id_and_no_more():
    wrong = [t + 1000 for t in ANSWER]
    outs, stats, eng = run([ANSWER], [wrong], max_new=40)
    assert outs == [ANSWER] and stats['steps'] == 39 and stats['accepted'] == 0
    assert all(e[2] == [[]] for e in steps_of(eng)[1:])                               # after the first miss nothing is offered
    for draft in ([], None, ANSWER[5:], list(reversed(ANSWER)), ANSWER * 3):
        outs, stats, _ = run([ANSWER], [draft], max_new=40)
        assert outs == [ANSWER] and stats['steps'] <= 39, draft


def test_windows_respect_budget_and_cache():
    _, _, eng = run([ANSWER], [ANSWER], max_new=12)
    offered = [e[2][0] for e in steps_of(eng)]
    assert [len(w) for w in offered] == [7, 2]                                        # 1 + 8 + 3 = the budget of 12: never an id past it
    # the cache: 10 prompt tokens + 20 leave room for 20 ids; the last window shrinks to what still fits (the stub asserts it)
    outs, _, eng = run([ANSWER], [ANSWER], max_new=20, max_tokens=30)
    assert outs == [ANSWER[:20]]


def test_a_batch_stays_within_64_rows():
    scripts = [[1000 * i + t for t in range(30)] for i in range(12)]
    outs, stats, eng = run(scripts, scripts, max_new=30)
    assert outs == scripts
    for e in steps_of(eng):
        assert sum(len(w) + 1 for w in e[2]) <= 64
    first = [len(w) for w in steps_of(eng)[0][2]]
    assert sum(first) + 12 == 64 and max(first) - min(first) <= 1                     # shortened evenly, the longest first
    assert D.fit_rows([[1] * 7] * 8) == [[1] * 7] * 8 and D.fit_rows([[]] * 70) == [[]] * 70
    # more than 64 unfinished rows: plain steps
    many = [[7000 + i] * 3 for i in range(70)]
    outs, _, eng = run(many, many, max_new=3)
    assert outs == many and {e[0] for e in steps_of(eng)} == {'decode'}


def test_from_indices():
    assert D.from_indices(torch.tensor([[5, 0, 7], [0, 0, 0], [9, 9, 1]])) == [5, 7, 9, 9, 1]
    assert D.from_indices(torch.tensor([4, 0, 6])) == [4, 6]                           # a single box: the squeezed (3,) form
    assert D.from_indices([[1, 2, 3]]) == [1, 2, 3] and D.from_indices(None) == []


# ---- what does not combine with a draft ----

def embeds(n=5):
    return torch.zeros(n, 8)


def test_generate_refuses_what_a_draft_does_not_take():
    from callireader_amd.constraints import Constraints
    from callireader_amd.sampling import SamplingParams
    m = make_model()
    m.engine = DraftEngine()
    for kw in (dict(do_sample=True), dict(num_beams=2), dict(return_dict_in_generate=True, output_scores=True), dict(no_repeat_ngram_size=2)):
        with pytest.raises(NotImplementedError, match='not implemented with a draft'):
            m._generate_kw(embeds(), 1.0, dict(kw, max_new_tokens=4, draft_ids=[1, 2]))
    for kw in (dict(sampling=SamplingParams(temperature=0.7, top_k=0, top_p=1.0)), dict(num_beams=2), dict(logprobs=1),
               dict(constraints=Constraints(no_repeat_ngram_size=2))):
        with pytest.raises(NotImplementedError, match='not implemented with a draft'):
            m.generate_pages([embeds()], max_new_tokens=4, drafts=[[1, 2]], **kw)
    with pytest.raises(ValueError):
        m.generate_pages([embeds()], max_new_tokens=4, drafts=[[1], [2]])
    m8 = make_model(kv_cache_dtype='e4m3')
    m8.engine = DraftEngine()
    with pytest.raises(NotImplementedError, match='e4m3'):
        m8.generate_pages([embeds()], max_new_tokens=4, drafts=[[1, 2]])
    with pytest.raises(NotImplementedError, match='e4m3'):
        m8._generate_kw(embeds(), 1.0, dict(max_new_tokens=4, draft_ids=[1, 2]))
    # and with everything off a draft goes through, with the plain ids
    m.engine.script[0] = [5, 6, 7, 8]
    assert m.generate_pages([embeds()], max_new_tokens=4, eos_token_id=None, drafts=[[5, 6, 7, 8]]) == [[5, 6, 7, 8]]
    assert m.draft_stats == dict(steps=1, drafted=2, accepted=2)


def test_pipelines_and_shards_refuse_a_draft():
    from callireader_amd import parallel
    m = make_model()
    with pytest.raises(NotImplementedError, match='PagePipeline'):
        next(m.chat_ocr_stream(None, None, [], 'q', dict(max_new_tokens=4), draft='align'))
    with pytest.raises(NotImplementedError, match='ContinuousPipeline'):
        next(m.chat_ocr_continuous(None, None, [], 'q', dict(max_new_tokens=4), draft='align'))
    with pytest.raises(NotImplementedError, match='sharded'):
        parallel.sharded_generate(m, [], [], [], img_id=1, ref_id=2, max_new_tokens=4, drafts=[[1]])
    with pytest.raises(NotImplementedError, match='sharded'):
        parallel.chat_ocr_pages_sharded(m, None, None, [], 'q', dict(max_new_tokens=4), draft='align')


def test_session_drafts():
    sess, eng = make_session()
    sess.m.engine = de = DraftEngine()
    sess.kv = de.kv_alloc(2, 512)
    gc = dict(max_new_tokens=6, do_sample=False)
    for kw in (dict(return_scores=True), dict(generation_config=dict(gc, do_sample=True)), dict(generation_config=dict(gc, no_repeat_ngram_size=2)),
               dict(generation_config=dict(gc, num_beams=2))):
        with pytest.raises(NotImplementedError):
            sess.chat_ocr('q', **dict(dict(generation_config=gc), **kw), draft=[1, 2])
        assert sess.kv.len[0] == 0                                                   # a refused turn leaves the trunk as it was
    with pytest.raises(ValueError):
        sess.chat_ocr('q', gc, draft='next')
    answer = [40, 41, 42, 43, EOS]
    de.script[0] = list(answer)
    first = sess.chat_ocr('q', gc)
    assert sess.answer_ids == answer
    de.script[0] = list(answer)
    again = sess.chat_ocr('q2', gc, draft='previous')                               # the second turn repeats the first answer: one step checks it all
    assert again == first and sess.m.draft_stats['steps'] == 1 and sess.m.draft_stats['accepted'] == 4
    for b in (1,):
        de.script[b] = list(answer)
    assert sess.ask_many(['q3'], gc, draft='previous') == [first]
    with pytest.raises(NotImplementedError):
        sess.ask_many(['q3'], dict(gc, do_sample=True), draft='previous')

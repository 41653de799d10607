"""Constrained greedy decoding on the device (csrc/constrain.hip, cr_kv_set_constraints / cr_op_constrain).

  - the kernel against the installed transformers' own processors, run on the CPU: equal -inf sets, every other value bit-equal to the input;
  - a fully masked row picks id 0;
  - a free-running constrained stream, replayed step by step from the raw logits the decode returns;
  - no_repeat_ngram_size=1 gives 48 distinct ids where the unconstrained page repeats one;
  - a constrained page's ids do not depend on its batch or pipeline, and its unconstrained neighbours keep their bits (fp8 decode off and on);
  - min_new_tokens, begin_suppress_tokens, sessions, token scores."""
import numpy as np
import pytest
import torch

from callireader_amd import constraints as K
from callireader_amd import synthetic
from callireader_amd.config import ModelDims

pytestmark = pytest.mark.gpu

V_FULL, V_RAGGED = 92553, 9001
NEG = -float('inf')


def hf_process(c, hist, row):
    """transformers' processors for the constraints `c` on one fp32 row (CPU) against the generated ids `hist`; returns the processed row and, per
    processor, the number of ids it newly set to -inf.  The whitelist is SuppressTokensLogitsProcessor over its complement."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor)
    x = torch.as_tensor(row, dtype=torch.float32).reshape(1, -1).clone()
    V = x.shape[1]
    ids = torch.as_tensor(list(hist), dtype=torch.long).reshape(1, -1)
    procs = []
    if c.no_repeat_ngram_size:
        procs.append(('ngram', NoRepeatNGramLogitsProcessor(c.no_repeat_ngram_size)))
    if c.bad_words_ids:
        procs.append(('bad_words', NoBadWordsLogitsProcessor([list(w) for w in c.bad_words_ids])))
    if c.suppress_tokens:
        procs.append(('suppress', SuppressTokensLogitsProcessor(list(c.suppress_tokens))))
    if c.allowed_token_ids is not None:
        procs.append(('whitelist', SuppressTokensLogitsProcessor(sorted(set(range(V)) - set(c.allowed_token_ids)))))
    if c.begin_suppress_tokens:
        procs.append(('begin', SuppressTokensAtBeginLogitsProcessor(list(c.begin_suppress_tokens), 0)))
    if c.min_new_tokens and c.eos_token_id is not None:
        procs.append(('min_new', MinNewTokensLengthLogitsProcessor(0, c.min_new_tokens, c.eos_token_id)))
    banned = {}
    for name, p in procs:
        before = int(torch.isinf(x).sum())
        x = p(ids, x)
        banned[name] = int(torch.isinf(x).sum()) - before
    return x[0], banned


@pytest.fixture(scope='module')
def rows():
    """Per vocabulary: 6 raw rows and 6 small-alphabet histories of 5000 ids (n-grams recur), made once and never changed."""
    out = {}
    for V in (V_RAGGED, V_FULL):
        g = torch.Generator().manual_seed(V)
        logits = torch.randn(6, V, generator=g) * 2.5
        alphabet = torch.tensor([0, 1, 31, 32, 4097, V - 33, V - 2, V - 1])             # both ends of a mask word, the ragged last word
        hist = alphabet[torch.randint(0, len(alphabet), (6, 5000), generator=g)]
        out[V] = (logits, hist)
    return out


def lens_for(N):
    return [0, max(N - 2, 0), max(N - 1, 0), N, 40, 5000]          # 5000: past the 4096 ids the penalty keeps in registers


PERM = [3, 0, 5, 1, 4, 2]


def check_against_hf(logits, hist, lens, c, seqs=None):
    """One op_constrain launch over the 6 rows against the processors; returns the per-processor ban counts summed over the rows."""
    from callireader_amd.engine import op_constrain
    dev = op_constrain(logits.cuda().contiguous(), c, history=hist, hist_len=lens, seqs=seqs).cpu()
    total = {}
    for r in range(logits.shape[0]):
        s = seqs[r] if seqs is not None else r
        want, banned = hf_process(c, hist[s, :lens[s]].tolist(), logits[r])
        for k, v in banned.items():
            total[k] = total.get(k, 0) + v
        got_inf, want_inf = torch.isinf(dev[r]), torch.isinf(want)
        assert torch.equal(got_inf, want_inf), (r, int(got_inf.sum()), int(want_inf.sum()))
        assert torch.equal(dev[r][~got_inf].view(torch.int32), logits[r][~got_inf].view(torch.int32)), r      # untouched: the input's bits
        assert bool((dev[r][got_inf] == NEG).all())
    return total


@pytest.mark.parametrize('V', [V_RAGGED, V_FULL])
def test_kernel_matches_transformers_processors(rows, V):
    logits, hist = rows[V]
    seen = {}

    def run(lens, c, seqs=None):
        for k, v in check_against_hf(logits, hist, lens, c, seqs).items():
            seen[k] = seen.get(k, 0) + v
    for N in (1, 2, 3, 5):
        run(lens_for(N), K.Constraints(no_repeat_ngram_size=N))
        run(lens_for(N), K.Constraints(no_repeat_ngram_size=N), PERM)
    lens = lens_for(3)
    t40, t5k = hist[4, :40].tolist(), hist[5, :5000].tolist()
    words = ((7,), (V - 1,),                                    # one id: the static mask (also its last bit)
             (t40[-1], 100), (2, 101),                          # two ids: a prefix that is row 4's tail, and one that is no id of the alphabet
             tuple(t5k[-15:]) + (102,), tuple(t40[-15:]) + (V - 3,), tuple([2] * 15) + (103,),      # 16 ids: rows 5 and 4 match, the last never
             (3, 104))
    run(lens, K.Constraints(bad_words_ids=words))
    run(lens, K.Constraints(bad_words_ids=words), PERM)
    run(lens, K.Constraints(suppress_tokens=(0, 31, 32, 63, 64, V - 1, V - 32, 5000)))
    run(lens, K.Constraints(begin_suppress_tokens=(5, V - 1, 33)))
    run(lens_for(5), K.Constraints(min_new_tokens=4, eos_token_id=V - 2))
    g = torch.Generator().manual_seed(1)
    white = tuple(sorted(set(torch.randint(0, V, (4000,), generator=g).tolist()) | {0, V - 1}))
    run(lens, K.Constraints(allowed_token_ids=white))
    run(lens, K.Constraints(allowed_token_ids=(V - 1,)))
    everything = K.Constraints(no_repeat_ngram_size=2, bad_words_ids=words, suppress_tokens=(11, V - 5), begin_suppress_tokens=(12, 13),
                               min_new_tokens=41, allowed_token_ids=white, eos_token_id=white[7])
    run(lens, everything, PERM)
    print(f'V={V}: ids banned per processor {seen}')
    assert set(seen) == {'ngram', 'bad_words', 'suppress', 'whitelist', 'begin', 'min_new'} and all(v > 0 for v in seen.values()), seen


def test_matches_inside_bad_words_fire(rows):
    """The bad-word cases above are not vacuous: the two- and sixteen-id words ban exactly where the history's tail is their prefix."""
    from callireader_amd.engine import op_constrain
    logits, hist = rows[V_RAGGED]
    lens = lens_for(3)
    t40, t5k = hist[4, :40].tolist(), hist[5, :5000].tolist()
    c = K.Constraints(bad_words_ids=((t40[-1], 100), tuple(t5k[-15:]) + (102,), tuple([2] * 15) + (103,)))
    dev = op_constrain(logits.cuda().contiguous(), c, history=hist, hist_len=lens).cpu()
    assert bool(torch.isinf(dev[4, 100])) and bool(torch.isinf(dev[5, 102])) and not bool(torch.isinf(dev[:, 103]).any())
    assert not bool(torch.isinf(dev[0]).any())                     # an empty history matches no prefix


def test_fully_masked_row_picks_id_0():
    from callireader_amd.engine import Engine, op_constrain, op_sample
    eng = Engine(ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1))
    try:
        g = torch.Generator().manual_seed(3)
        raw = torch.randn(2, V_RAGGED, generator=g)
        raw[:, 0] = -3.0                                           # far from the maximum: only the mask can make id 0 the pick
        w = int(raw[0].argmax())
        hist = torch.tensor([[w], [w]])
        c = K.Constraints(allowed_token_ids=(w,), no_repeat_ngram_size=1)
        out = op_constrain(raw.cuda().contiguous(), c, history=hist, hist_len=[1, 0])
        ids, _ = op_sample(eng, out, 0.0, 0, 1.0, 0, 0)
        assert ids.cpu().tolist() == [0, w]                         # row 1 has no history: its one permitted id survives
        out = out.cpu()
        assert out[0, 0] == raw[0, 0] and bool(torch.isinf(out[0, 1:]).all())
        assert out[1, w] == raw[1, w] and int(torch.isinf(out[1]).sum()) == V_RAGGED - 1
    finally:
        eng.close()


@pytest.fixture(scope='module')
def llm():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=9000)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=3), dims, max_tokens=512, max_pages=64)
    g = torch.Generator().manual_seed(1)
    ids = [torch.randint(0, 9000, (int(n),), generator=g) for n in torch.randint(20, 90, (64,), generator=g)]
    pages = [m.engine.embed_splice(i) for i in ids]
    yield m, pages, ids
    m.close()


def stream(m, page, c, pen, steps):
    """One sequence driven step by step: (raw logits per step on the CPU, the ids)."""
    kv = m.kv()
    kv.reset()
    if c is not None:
        kv.set_constraints(0, c)
    lgs = [m.engine.prefill(kv, 0, page, penalty=pen, want_logits=True).cpu().reshape(-1)]
    for _ in range(steps - 1):
        lgs.append(m.engine.decode(kv, [0], penalty=pen, want_logits=True)[0].cpu())
    return lgs, kv.generated(0)


def replay(lgs, ids, c, pen):
    """Every id against the CPU: the raw row through the constraint processors and the repetition penalty, np.argmax (first maximum).  At a penalty
    other than 1 a step whose two best processed scores lie within 1e-4 is not compared (test_gpu_sampling.py's replay rule); returns how many."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    near = 0
    for step, lg in enumerate(lgs):
        z = lg.clone() if c is None else hf_process(c, ids[:step], lg)[0]
        if pen != 1.0 and step:
            z = RepetitionPenaltyLogitsProcessor(pen)(torch.tensor([ids[:step]]), z[None])[0]
        z = z.numpy()
        top2 = np.partition(z, -2)[-2:]
        if pen != 1.0 and top2[1] - top2[0] < 1e-4:
            near += 1
            continue
        assert int(np.argmax(z)) == ids[step], (step, int(np.argmax(z)), ids[step])
    return near


@pytest.mark.parametrize('pen', [1.0, 1.5])
def test_free_running_stream_replays_exactly(llm, pen):
    m, pages, _ = llm
    _, free = stream(m, pages[0], None, pen, 48)
    c = K.Constraints(no_repeat_ngram_size=2, bad_words_ids=((free[1],), (free[2], free[3])), suppress_tokens=(free[4], free[5]),
                      begin_suppress_tokens=(free[0],), min_new_tokens=6, eos_token_id=free[1])
    lgs, ids = stream(m, pages[0], c, pen, 48)
    assert len(ids) == 48 and ids != free and ids[0] != free[0]
    assert all(torch.isfinite(lg).all() for lg in lgs)             # the rows the decode returns stay raw
    assert replay(lgs, ids, c, pen) <= 1


def test_no_repeat_1_gives_distinct_ids_where_the_free_page_repeats(llm):
    m, pages, ids = llm
    gen = dict(max_new_tokens=48, eos_token_id=None, repetition_penalty=1.0)
    frees = m.generate_pages(pages[:64], **gen)
    # the input has to be a page that repeats an id when unconstrained (the synthetic model's streams rarely do within 48 ids): the first such page
    k = next((i for i, f in enumerate(frees) if len(set(f)) < 48), None)
    assert k is not None, 'no page of the fixture repeats an id in 48: pick another seed'
    free = frees[k]
    assert len(free) == 48 and len(set(free)) < 48
    got = m.generate_pages([pages[k]], **gen, constraints=K.Constraints(no_repeat_ngram_size=1))[0]
    assert len(got) == 48 and len(set(got)) == 48
    first = next(t for t in range(48) if free[t] in free[:t])
    assert got[:first] == free[:first] and got[first] != free[first]          # the streams part exactly where the free one first repeats
    m.img_context_token_id = 8990
    plain = m.generate_ocr(input_ids=ids[k][None], repetition_penalty=1.0, max_new_tokens=48, eos_token_id=None)[0].tolist()
    keyed = m.generate_ocr(input_ids=ids[k][None], repetition_penalty=1.0, max_new_tokens=48, eos_token_id=None, no_repeat_ngram_size=1)[0].tolist()
    assert plain == free and keyed == got                          # the public keyword reaches the device (it used to be ignored)


GEN = dict(max_new_tokens=24, eos_token_id=None, repetition_penalty=1.3)


def test_batch_invariance(llm):
    m, pages, ids = llm
    m.img_context_token_id = 8990
    try:
        for fp8 in (False, True):
            m.engine.enable_fp8_decode(fp8)
            _batch_invariance(m, pages, ids, fp8)
    finally:
        m.engine.enable_fp8_decode(False)


def _batch_invariance(m, pages, ids, fp8):
    from callireader_amd.continuous import ContinuousPipeline
    free = m.generate_pages(pages[:64], **GEN)                     # every page's own unconstrained ids (batches of this path keep a page's bits)
    f7 = free[7]
    kw = dict(no_repeat_ngram_size=2, bad_words_ids=[[f7[2]], [f7[3], f7[4]]], suppress_tokens=[f7[6]], begin_suppress_tokens=[f7[0]])
    c = K.parse(kw)
    alone = m.generate_ocr(input_ids=ids[7][None], repetition_penalty=GEN['repetition_penalty'], max_new_tokens=GEN['max_new_tokens'],
                           eos_token_id=None, **kw)[0].tolist()
    assert alone != f7 and alone[0] != f7[0]
    assert alone == m.generate_pages([pages[7]], **GEN, constraints=c)[0]
    for P, at in ((13, 5), (64, 40)):
        order = [i for i in range(P) if i != 7]
        order.insert(at, 7)
        out = m.generate_pages([pages[i] for i in order], **GEN, constraints=[c if j == at else None for j in range(P)])
        assert out[at] == alone, (fp8, P)
        for j, i in enumerate(order):
            if j != at:
                assert out[j] == free[i], (fp8, P, j)              # the unconstrained pages of the batch: bit for bit their own runs
    pipe = m.page_pipeline(max_new_tokens=GEN['max_new_tokens'], eos_token_id=None, repetition_penalty=GEN['repetition_penalty'])
    try:
        pipe.start([pages[1], pages[7], pages[2]], constraints=[None, c, None])
        out = pipe.finish()
        assert out == [free[1], alone, free[2]]
    finally:
        pipe.close()
    cp = ContinuousPipeline(m, slots=2, max_new_tokens=GEN['max_new_tokens'], eos_token_id=None, repetition_penalty=GEN['repetition_penalty'],
                            admit_group=1)
    try:
        order = (3, 4, 7, 5, 6)
        tickets = [cp.submit(pages[i], constraints=c if i == 7 else None) for i in order]
        got = dict(cp.results())
        for t, i in zip(tickets, order):
            assert got[t] == (alone if i == 7 else free[i]), (fp8, i)     # also the page that takes the constrained page's slot after it
    finally:
        cp.close()


def test_min_new_tokens_and_begin_suppress(llm):
    m, pages, _ = llm
    lgs0, free = stream(m, pages[5], None, 1.0, 12)
    eos = free[0]                                                  # a page whose unconstrained first pick is the EOS id
    gen = dict(max_new_tokens=12, eos_token_id=eos, repetition_penalty=1.0)
    assert m.generate_pages([pages[5]], **gen)[0] == [eos]
    for mnt in (1, 3, 7):
        c = K.parse(dict(min_new_tokens=mnt), eos_token_id=eos)
        got = m.generate_pages([pages[5]], **gen, constraints=c)[0]
        assert len(got) > mnt or (len(got) == 12 and eos not in got)
        assert eos not in got[:mnt]                                # exactly m ids without the EOS id ...
        lgs, ids = stream(m, pages[5], c, 1.0, mnt + 1)
        assert ids[:mnt] == got[:mnt] and ids[mnt] == int(lgs[mnt].argmax())        # ... and at step m nothing is banned any more
        assert replay(lgs, ids, c, 1.0) == 0
    c = K.Constraints(begin_suppress_tokens=(eos,))
    lgs, ids = stream(m, pages[5], c, 1.0, 12)
    assert ids[0] != eos and replay(lgs, ids, c, 1.0) == 0
    assert all(ids[t] == int(lgs[t].argmax()) for t in range(1, 12))                # step 0 only: every later id is the raw row's argmax


def test_state_is_cleared_by_reset_truncate_fork_and_refused_with_beams(llm):
    from callireader_amd import _binding as B
    from callireader_amd.engine import _stream, c_constraints
    m, pages, _ = llm
    kv = m.kv(4)
    free = m.generate_pages([pages[3]], **GEN)[0]
    c = K.Constraints(no_repeat_ngram_size=1, suppress_tokens=(free[0],))

    def first_ids(seq, n=4):
        m.engine.prefill(kv, seq, pages[3], penalty=GEN['repetition_penalty'])
        for _ in range(n - 1):
            m.engine.decode(kv, [seq], penalty=GEN['repetition_penalty'])
        return kv.generated(seq)
    kv.reset()
    kv.set_constraints(0, c)
    assert first_ids(0)[0] != free[0]
    kv.reset(0)                                                    # reset: no constraints
    assert first_ids(0) == free[:4]
    kv.reset(0)
    kv.set_constraints(0, c)
    kv.set_constraints(0, None)                                    # NULL switches off
    assert first_ids(0) == free[:4]
    S = pages[3].shape[0]
    kv.set_constraints(0, c)
    kv.truncate(0, S - 1)                                          # truncate: no constraints; the last prompt row again
    m.engine.prefill(kv, 0, pages[3][S - 1:], penalty=GEN['repetition_penalty'])
    assert kv.generated(0) == free[:1]
    kv.set_constraints(1, c)
    kv.fork(0, [1], S - 1)                                         # fork: its destinations hold none
    m.engine.prefill(kv, 1, pages[3][S - 1:], penalty=GEN['repetition_penalty'])
    assert kv.generated(1) == free[:1]
    kv.reset()
    kv.set_constraints(2, c)
    assert B.lib.cr_kv_set_beam(kv._h, 2, 2, 1.0, 0, -1, 8, _stream()) == -3         # CR_ERR_STATE: a constrained sequence joins no group
    kv.reset()
    kv.set_beam(2, 2, max_new=8)
    st, _keep = c_constraints(c)
    import ctypes
    assert B.lib.cr_kv_set_constraints(kv._h, 3, ctypes.byref(st), _stream()) == -3  # CR_ERR_STATE: a member of a beam group
    bad, _keep2 = c_constraints(K.Constraints(suppress_tokens=(9000,)))
    assert B.lib.cr_kv_set_constraints(kv._h, 0, ctypes.byref(bad), _stream()) == -1  # an id outside the vocabulary of 9000
    kv.reset()


def test_session_turns_do_not_inherit_constraints():
    from chat_helpers import FakeTokenizer
    from PIL import Image
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=9000)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=0), dims, max_tokens=4096)
    try:
        tok = FakeTokenizer()
        img = Image.fromarray(np.random.default_rng(0).integers(0, 255, (448, 448, 3), dtype=np.uint8))
        gen = dict(max_new_tokens=12)
        qs = ('first question', 'second one', 'and a third')

        def turns(second_kw):
            with m.open_page(tok, None, img, use_p=False) as s:
                hist, out = None, []
                for q, kw in zip(qs, (gen, dict(gen, **second_kw), gen)):
                    r, hist = s.chat_ocr(q, kw, history=hist, return_history=True, repetition_penalty=1.0)
                    out.append(r)
                return out, hist
        plain, _ = turns({})
        cons, hist = turns(dict(no_repeat_ngram_size=1, min_new_tokens=12))
        assert cons[0] == plain[0] and cons[1] != plain[1]
        # turn 3 of the constrained conversation equals its own unconstrained run: a fresh chat_ocr over the same history
        with m.open_page(tok, None, img, use_p=False) as s:
            again = s.chat_ocr(qs[2], gen, history=hist[:2], repetition_penalty=1.0)
        assert again == cons[2]
        lone = m.chat_ocr(tok, None, img, qs[2], gen, history=[tuple(h) for h in hist[:2]], use_p=False, repetition_penalty=1.0)
        assert lone == cons[2]
    finally:
        m.close()


def test_token_scores_of_a_constrained_page(llm):
    m, pages, _ = llm
    pen = 1.3
    _, free = stream(m, pages[2], None, pen, 16)
    c = K.Constraints(no_repeat_ngram_size=1, suppress_tokens=(free[0], free[1]), bad_words_ids=((free[2],),))
    kv = m.kv()
    kv.reset()
    kv.set_constraints(0, c)
    kv.set_logprobs(0, 8)
    lgs = [m.engine.prefill(kv, 0, pages[2], penalty=pen, want_logits=True).cpu().reshape(-1)]
    for _ in range(15):
        lgs.append(m.engine.decode(kv, [0], penalty=pen, want_logits=True)[0].cpu())
    ids = kv.generated(0)
    lp, top_ids, top_lp = kv.logprobs(0)
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    for t, lg in enumerate(lgs):
        z = hf_process(c, ids[:t], lg)[0]
        if t:
            z = RepetitionPenaltyLogitsProcessor(pen)(torch.tensor([ids[:t]]), z[None])[0]
        masked = set(torch.nonzero(torch.isinf(z)).reshape(-1).tolist())
        assert masked and not (set(top_ids[t].tolist()) & masked), t          # no masked id among the alternatives
        want = torch.log_softmax(z.double(), 0)
        # test_gpu_logprobs.py's TOL for the unconstrained case: 1e-5 absolute of the float64 log-softmax (|z| <= 32; -inf entries contribute 0)
        assert abs(float(lp[t]) - float(want[ids[t]])) <= 1e-5, t
        assert np.allclose(top_lp[t], want[top_ids[t].astype(np.int64)].numpy(), rtol=0, atol=1e-5), t
        assert int(top_ids[t][0]) == ids[t]

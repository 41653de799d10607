"""cr_llm_ground_batch on a real MI355X: the scoring pass that also reports the attention mass of every scored row over spans of key positions (reduced model
of tests/test_gpu_score.py: 2 LLM layers, full width, vocab 8201; its prompt and answer helpers).

Reference: tests/ground_ref.py, a layer loop of oracle.internlm2's own functions that keeps every layer's fp32 softmax; the mass is computed from that.
Bound: two independent bf16 paths are compared, so the test measures how far bf16 moves the oracle itself, B = 2 * max |mass(oracle in bf16) - mass(oracle
in fp32)| on its own inputs (per case and layer range), and asserts |HIP - oracle in bf16| <= B.  It also asserts, on the oracle alone, what makes that
bound mean something: shortening every span by one key moves more than 90 % of the entries by more than 4 B, and layer 0 alone and layer 1 alone differ by
more than 4 B on more than half of them -- "entries" being the (row, span) pairs that can hold mass at all (a non-empty span that is not wholly behind the
row)."""
import ctypes as C

import pytest
import torch

from ground_ref import layer_softmax, span_mass
from test_gpu_score import V, answer, prompt, rows_of, setup  # noqa: F401  (module fixture: the reduced model)

pytestmark = pytest.mark.gpu

BASE = [(0, 2)] + [(5 + 3 * i, 8 + 3 * i) for i in range(14)] + [(50, 51), (62, 66), (68, 68)]      # tests/test_gpu_ground_ops.py's span set
SPANS = {(70, 37): BASE + [(80, 90)], (17, 130): BASE + [(80, 90), (126, 131)], (40, 37): BASE + [(70, 74)]}
LAYERS = [(0, 2), (0, 1), (1, 2)]

_case = {}


def case(setup, P, T):
    """rows, targets and the oracle's softmax in bf16 and fp32, computed once per (P, T)"""
    if (P, T) not in _case:
        seed = 1000 + P
        y = answer(T, seed)
        e, targets = rows_of(setup, P, y, seed)
        _case[(P, T)] = dict(e=e, targets=targets, y=y, rows=list(range(P - 1, P + T - 1)), spans=SPANS[(P, T)],
                             bf=layer_softmax(setup['sd'], 2, e, torch.bfloat16), fp=layer_softmax(setup['sd'], 2, e, torch.float32))
    return _case[(P, T)]


def oracle(c, layers, spans=None):
    spans = c['spans'] if spans is None else spans
    return span_mass(c['bf'], c['rows'], spans, layers), span_mass(c['fp'], c['rows'], spans, layers)


def live(c):
    """[rows, spans] bool: the entries that can hold mass"""
    pos = torch.tensor(c['rows'])[:, None]
    return torch.tensor([[e > s and s <= int(p) for s, e in c['spans']] for p in pos[:, 0]])


def close(got, c, layers, what):
    bf, fp = oracle(c, layers)
    B = 2 * float((bf - fp).abs().max())
    d = float((got.double() - bf).abs().max())
    m = bf[live(c)]
    print(f'{what} layers {layers}: B = {B:.3e}, max |HIP - oracle bf16| = {d:.3e}, live masses {float(m.min()):.4f} .. {float(m.max()):.4f}')
    assert d <= B, (what, layers, d, B)
    return B


def bound_means_something(c):
    """On the oracle alone; B is the case's bound over all layers.  Measured on the CPU for (70, 37): B 1.22e-3, 98.2 % moved, 64.7 % differ."""
    on = live(c)
    Bs = {ly: 2 * float((oracle(c, ly)[0] - oracle(c, ly)[1]).abs().max()) for ly in LAYERS}
    full = oracle(c, (0, 2))[0]
    short = oracle(c, (0, 2), [(s, max(s, e - 1)) for s, e in c['spans']])[0]
    moved = float(((full - short).abs() > 4 * Bs[(0, 2)])[on].float().mean())
    l0, l1 = oracle(c, (0, 1))[0], oracle(c, (1, 2))[0]
    differ = float(((l0 - l1).abs() > 4 * Bs[(0, 2)])[on].float().mean())
    print(f'B {Bs}; one key less moves {100 * moved:.1f} % of {int(on.sum())} entries by > 4 B; layer 0 and layer 1 differ by > 4 B on {100 * differ:.1f} %')
    assert moved > 0.9 and differ > 0.5


@pytest.mark.parametrize('layers', LAYERS)
def test_one_page_against_the_oracle(setup, layers):
    eng = setup['eng']
    c = case(setup, 70, 37)
    kv = eng.kv_alloc(1, 512)
    try:
        (ts,), (mass,) = eng.ground_batch(kv, [0], [c['e'].cuda()], [c['targets']], [c['spans']], layers=layers, penalty=1.5, top_n=3)
        assert mass.shape == (37, len(c['spans'])) and len(ts) == 37 and kv.length(0) == 70 + 37 - 1 and kv.generated(0) == []
        close(mass, c, layers, '(70, 37)')
        if layers == (0, 2):
            bound_means_something(c)
        assert bool((mass[~live(c)] == 0).all())
    finally:
        kv.free()


@pytest.mark.parametrize('layers', LAYERS)
def test_two_pages_in_one_call(setup, layers):
    """(17, 130) together with (40, 37): against the oracle, and each page's bits are those of the page alone"""
    eng = setup['eng']
    cs = [case(setup, 17, 130), case(setup, 40, 37)]
    kv = eng.kv_alloc(3, 512)
    try:
        _, both = eng.ground_batch(kv, [2, 0], [c['e'].cuda() for c in cs], [c['targets'] for c in cs], [c['spans'] for c in cs], layers=layers,
                                   want_scores=False)
        assert [kv.length(s) for s in (2, 0, 1)] == [17 + 130 - 1, 40 + 37 - 1, 0]
        for c, m, what in zip(cs, both, ('(17, 130)', '(40, 37)')):
            assert m.shape == (len(c['rows']), len(c['spans']))
            close(m, c, layers, what)
        for i, c in enumerate(cs):
            _, (alone,) = eng.ground_batch(kv, [1], [c['e'].cuda()], [c['targets']], [c['spans']], layers=layers, want_scores=False)
            assert torch.equal(alone, both[i]), i
            kv.reset(1)
    finally:
        kv.free()


def test_scores_and_cache_are_score_batch_s(setup):
    eng = setup['eng']
    c = case(setup, 70, 37)
    kv = eng.kv_alloc(3, 512)
    try:
        e = c['e'].cuda()
        (a,) = eng.score_batch(kv, [0], [e], [c['targets']], penalty=1.5, top_n=3)
        (b,), (mass,) = eng.ground_batch(kv, [1], [e], [c['targets']], [c['spans']], penalty=1.5, top_n=3)
        assert (a.logprobs.view('int32') == b.logprobs.view('int32')).all() and (a.top_ids == b.top_ids).all()
        assert (a.top_logprobs.view('int32') == b.top_logprobs.view('int32')).all()
        (none,), (only,) = eng.ground_batch(kv, [2], [e], [c['targets']], [c['spans']], want_scores=False)      # grounding only: no LM head, the same mass bits
        assert none is None and torch.equal(only, mass)
        assert kv.length(0) == kv.length(1) == kv.length(2) == 106 and kv.generated(1) == [] and kv.generated(2) == []
        for pos in (0, 69, 105):
            for which in (0, 1):
                assert torch.equal(kv.read(1, 0, pos, which), kv.read(1, 1, pos, which)) and torch.equal(kv.read(1, 0, pos, which), kv.read(1, 2, pos, which))
    finally:
        kv.free()


def test_refusals_change_nothing(setup):
    from callireader_amd import _binding as B
    eng = setup['eng']
    e, targets = rows_of(setup, 4, answer(3, 1), 1)
    e = e.cuda()
    kv, kv8 = eng.kv_alloc(4, 16), eng.kv_alloc(1, 16, dtype='e4m3')
    try:
        eng.prefill(kv, 3, prompt(5, 2).cuda())                      # sequence 3 holds a generated id
        kv.set_beam(1, 2, max_new=4)                                 # sequences 1 and 2 are a beam group
        lens0 = [kv.length(s) for s in range(4)]
        mass = torch.zeros(8, 4, device='cuda')
        lp = torch.empty(8, device='cuda')

        def call(seq=0, spans=((0, 2), (3, 5)), layers=(0, 2), ld=4, kvx=kv, m=mass, lpx=lp, top_n=0, count=None):
            flat = [v for sp in spans for v in sp] or [0]
            return B.lib.cr_llm_ground_batch(eng._h, kvx._h, (C.c_int32 * 1)(seq), 1, C.c_void_p(e.data_ptr()), (C.c_int32 * 1)(6), (C.c_int64 * 6)(*targets), 1.0,
                                             top_n, None if lpx is None else C.c_void_p(lpx.data_ptr()), None, None, (C.c_int32 * len(flat))(*flat),
                                             (C.c_int32 * 1)(len(spans) if count is None else count), layers[0], layers[1],
                                             None if m is None else C.c_void_p(m.data_ptr()), ld, None)

        def refused(code, **kw):
            assert call(**kw) == code, kw
            assert [kv.length(s) for s in range(4)] == lens0 and kv8.length(0) == 0 and kv.generated(0) == []
        refused(-1, m=None)                                          # null mass
        refused(-1, spans=((3, 5), (0, 2)))                          # unsorted
        refused(-1, spans=((0, 3), (2, 5)))                          # overlapping
        refused(-1, spans=((3, 1),))                                 # reversed
        refused(-1, spans=((0, 2), (5, 7)))                          # outside [0, 0 + 6)
        refused(-1, spans=((-1, 2),))
        refused(-1, count=-1)
        refused(-1, count=1025)
        refused(-1, ld=1)                                            # mass_ld below the span count
        refused(-1, layers=(-1, 2))
        refused(-1, layers=(0, 3))
        refused(-1, layers=(1, 1))
        refused(-1, lpx=None, top_n=2)                               # top_n > 0 with a null lp
        refused(-1, seq=4)                                           # everything cr_llm_score_batch refuses ...
        refused(-1, kvx=kv8)                                         # ... an e4m3 cache
        refused(-1, seq=1)                                           # ... a beam-group member
        refused(-3, seq=3)                                           # ... a sequence that holds generated ids
        with pytest.raises(ValueError):
            eng.ground_batch(kv, [0], [e], [targets], [[(3, 1)]])
        with pytest.raises(ValueError):
            eng.ground_batch(kv, [0], [e], [targets], [[(0, 1)]], layers=(0, 3))
        assert [kv.length(s) for s in range(4)] == lens0
        # and the same call is accepted once nothing is wrong
        assert call() == 0 and kv.length(0) == 6
        torch.cuda.synchronize()
        assert bool((mass[:3, 2:] == 0).all()) and bool((mass[:3, :2] > 0).all())
    finally:
        kv.free(); kv8.free()

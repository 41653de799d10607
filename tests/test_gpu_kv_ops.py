"""cr_kv_reset / cr_kv_truncate / cr_kv_fork (csrc/kv.hip) on a real MI355X: a 2-layer LLM at full width, the fixture style of test_gpu_llm.py.

Truncate is state only, fork copies exactly a prefix, and a sequence that was rolled back or forked computes the bits of one that never ran ahead --
the properties callireader_amd/session.py builds a page's second turn and its branches on.  The composed path is held against the CPU oracle under
decode_checks.check_step, as test_gpu_llm.py's continued prefill is."""
import pytest
import torch

from callireader_amd.config import ModelDims
from callireader_amd import synthetic

from decode_checks import rel_l2, check_step

pytestmark = pytest.mark.gpu

ARG, STATE = r'error -1\b', r'error -3\b'          # CR_ERR_ARG, CR_ERR_STATE as CalliReaderError words them


@pytest.fixture(scope='module')
def setup():
    from callireader_amd.engine import Engine
    dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=8201)
    sd = synthetic.make_state_dict(dims, parts=('llm',), seed=0)
    eng = Engine(dims, max_pos=2048)
    eng.load_state_dict(sd)
    eng.load_rope()
    eng.finalize()
    return dict(eng=eng, dims=dims, sd=sd)


def prompt(S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, S, 4096, generator=g) * 0.02).to(torch.bfloat16)


def two_prompts(a, b):
    whole = prompt(a + b, 4000 + 7 * a + b)
    return whole, whole[:, :a], whole[:, a:]


def rows(kv, seq, positions, layers=(0, 1)):
    """{(layer, which, pos): (8, 128) bf16} of one sequence"""
    return {(l, w, p): kv.read(l, seq, p, w).clone() for l in layers for w in (0, 1) for p in positions}


def poll(kv):
    out = torch.zeros(1 + 2 * kv.n_seqs, dtype=torch.int32).pin_memory()
    kv.poll_finished(out)
    torch.cuda.synchronize()
    return out.tolist()


def test_truncate_keeps_rows_and_clears_state(setup):
    from callireader_amd._binding import CalliReaderError
    eng = setup['eng']
    a = 70
    kv = eng.kv_alloc(3, 256)
    eng.prefill(kv, 1, prompt(a, 1).cuda(), penalty=1.5)
    kv.set_stop(1, max_new=3)
    for _ in range(5):
        eng.decode(kv, [1], penalty=1.5)
    assert kv.length(1) == a + 5 and len(kv.generated(1)) == 6
    assert poll(kv)[1 + 3 + 1] == 3                                   # the budget stopped it at its third id
    before = rows(kv, 1, (0, 69, 70, 74))
    with pytest.raises(CalliReaderError, match=ARG):
        kv.truncate(1, a + 6)                                         # n > length
    with pytest.raises(CalliReaderError, match=ARG):
        kv.truncate(1, -1)
    kv.truncate(1, a)
    assert kv.length(1) == a and kv.generated(1) == []
    after = rows(kv, 1, (0, 69, 70, 74))
    for key in before:                                                # the cut is state only: the rows past it read back too
        assert torch.equal(before[key], after[key]), key
    assert poll(kv)[1 + 3 + 1] == 0                                   # no stop for the sequence
    kv.set_stop(1, max_new=2)                                         # a budget counts from 0 again
    assert poll(kv)[1 + 3 + 1] == 0
    eng.prefill(kv, 1, prompt(4, 2).cuda(), penalty=1.5)
    assert poll(kv)[1 + 3 + 1] == 0 and len(kv.generated(1)) == 1
    eng.decode(kv, [1], penalty=1.5)
    assert poll(kv)[1 + 3 + 1] == 2 and kv.length(1) == a + 5
    kv.truncate(1, 0)                                                 # n = 0 is reset(seq)
    assert kv.length(1) == 0 and kv.generated(1) == [] and poll(kv)[1 + 3 + 1] == 0
    kv.reset()
    kv.set_beam(1, 2, eos_id=None, max_new=8)
    with pytest.raises(CalliReaderError, match=STATE):
        kv.truncate(2, 0)                                             # a beam-group member
    kv.free()


@pytest.mark.parametrize('a,b', [(70, 130), (255, 1), (256, 31), (257, 64)])
def test_truncate_then_continue_equals_never_having_run_ahead(setup, a, b):
    """Sequence 0 runs 7 decode steps past A, is rolled back to A and continued with B; sequence 1 goes from A to B directly.  The raw logits of the
    continued prefill and of three teacher-forced decode steps are the same bits (the cut sits on and around the decode attention's 256-key split).
    Sequence 0 then holds one id and sequence 1 two: only raw logits and cache rows are compared."""
    eng = setup['eng']
    _, A, B = two_prompts(a, b)
    kv = eng.kv_alloc(2, 512)
    eng.prefill(kv, 0, A.cuda())
    for _ in range(7):
        eng.decode(kv, [0])
    kv.truncate(0, a)
    l0 = eng.prefill(kv, 0, B.cuda(), want_logits=True).clone()
    eng.prefill(kv, 1, A.cuda())
    l1 = eng.prefill(kv, 1, B.cuda(), want_logits=True).clone()
    assert torch.equal(l0, l1), float((l0 - l1).abs().max())
    assert kv.length(0) == kv.length(1) == a + b and len(kv.generated(0)) == 1 and len(kv.generated(1)) == 2
    for t in range(3):
        tok = torch.tensor([11 + 97 * t])
        d0 = eng.decode(kv, [0], force_tokens=tok, want_logits=True).clone()
        d1 = eng.decode(kv, [1], force_tokens=tok, want_logits=True).clone()
        assert torch.equal(d0, d1), (t, float((d0 - d1).abs().max()))
    for pos in (0, a - 1, a, a + b - 1, a + b + 2):
        for key, r in rows(kv, 0, (pos,)).items():
            assert torch.equal(r, kv.read(key[0], 1, pos, key[1])), key
    kv.free()


@pytest.mark.parametrize('n', [1, 70, 256, 257])
def test_fork_copies_exactly_the_prefix(setup, n):
    eng = setup['eng']
    kv = eng.kv_alloc(4, 384)
    eng.prefill_batch(kv, [0, 1, 2, 3], [prompt(S, 50 + S).cuda() for S in (300, 290, 310, 320)])
    at = sorted({0, n - 1, n, n + 20})
    old = {s: rows(kv, s, at) for s in range(4)}
    kv.fork(0, [2, 1, 3], n)
    new = {s: rows(kv, s, at) for s in range(4)}
    for key in old[0]:
        assert torch.equal(new[0][key], old[0][key]), key             # src is unchanged
        for d in (1, 2, 3):
            want = old[0][key] if key[2] < n else old[d][key]         # the prefix is the source's, the rest the destination's old rows
            assert torch.equal(new[d][key], want), (d, key)
            assert float(new[d][key].float().abs().max()) > 0
    assert [kv.length(s) for s in range(4)] == [300, n, n, n]
    assert [kv.generated(s) for s in (1, 2, 3)] == [[], [], []] and len(kv.generated(0)) == 1
    kv.free()


def test_fork_refuses(setup):
    from callireader_amd._binding import CalliReaderError
    eng = setup['eng']
    kv = eng.kv_alloc(4, 128)
    eng.prefill(kv, 0, prompt(40, 3).cuda())
    for dsts, n in (([0], 10), ([1, 1], 10), ([4], 10), ([-1], 10), ([1], 0), ([1], 41), ([], 10), ([1, 2, 3, 1], 10)):
        with pytest.raises(CalliReaderError, match=ARG):
            kv.fork(0, dsts, n)
    with pytest.raises(CalliReaderError, match=ARG):
        kv.fork(1, [2], 1)                                            # an empty source
    assert [kv.length(s) for s in range(4)] == [40, 0, 0, 0]          # a refused call changes nothing
    kv.set_beam(2, 2, eos_id=None, max_new=8)
    with pytest.raises(CalliReaderError, match=STATE):
        kv.fork(0, [1, 3], 10)                                        # a destination in a beam group
    eng.prefill(kv, 2, prompt(12, 4).cuda())
    with pytest.raises(CalliReaderError, match=STATE):
        kv.fork(2, [1], 5)                                            # the source in a beam group
    kv.free()
    kv8 = eng.kv_alloc(2, 64, dtype='e4m3')
    eng.prefill(kv8, 0, prompt(16, 5).cuda())
    with pytest.raises(CalliReaderError, match=r'error -1\b.*e4m3'):
        kv8.fork(0, [1], 8)
    kv8.truncate(0, 8)                                                # truncate is state only: any cache format
    assert kv8.length(0) == 8
    kv8.free()


@pytest.mark.parametrize('a,b', [(70, 130), (256, 31)])
def test_a_forked_sequence_computes_what_its_source_computes(setup, a, b):
    """The source keeps the pick it made after A, the branches start without ids: the ids compared are those from B on."""
    eng = setup['eng']
    _, A, B = two_prompts(a, b)
    kv = eng.kv_alloc(3, 512)
    eng.prefill(kv, 0, A.cuda())
    kv.fork(0, [1, 2], a)
    lg = eng.prefill_batch(kv, [0, 1, 2], [B.cuda()] * 3, want_logits=True).clone()
    assert torch.equal(lg[0], lg[1]) and torch.equal(lg[0], lg[2])
    for t in range(3):
        lg = eng.decode(kv, [2, 0, 1], want_logits=True).clone()
        assert torch.equal(lg[0], lg[1]) and torch.equal(lg[0], lg[2]), t
    ids = [kv.generated(s) for s in range(3)]
    assert len(ids[1]) == 4 and ids[1] == ids[2] == ids[0][1:]
    assert [kv.length(s) for s in range(3)] == [a + b + 3] * 3
    kv.free()


def test_truncate_fork_prefill_against_the_oracle(setup):
    """prefill(A), four decode steps, truncate back to A, fork to one branch, prefill(B) on the branch, against the oracle run on A ‖ B: the branch's
    logits and six teacher-forced decode steps under check_step's rule (test_gpu_llm.py::test_continued_prefill_against_the_oracle's walk)."""
    from oracle import generate
    eng, sd = setup['eng'], setup['sd']
    a, b = 200, 300
    whole, A, B = two_prompts(a, b)
    with torch.no_grad():
        ref_ids, ref_logits = generate.greedy_generate(sd, 2, whole, max_new_tokens=7, eos_token_id=-1, repetition_penalty=1.0, return_logits=True)
    ref_ids = ref_ids[0].tolist()
    kv = eng.kv_alloc(2, 640)
    eng.prefill(kv, 0, A.cuda())
    for _ in range(4):
        eng.decode(kv, [0])
    kv.truncate(0, a)
    kv.fork(0, [1], a)
    lg = eng.prefill(kv, 1, B.cuda(), want_logits=True)
    torch.cuda.synchronize()
    diverged = []
    for t in range(7):
        got = lg.float().cpu().reshape(-1)
        print(f'  step {t}: rel-L2 {rel_l2(got, ref_logits[t]):.3e}, max |diff| {float((got - ref_logits[t]).abs().max()):.3e}')
        if check_step(t, got, ref_logits[t], kv.generated(1)[t], ref_ids):
            diverged.append(t)
        if t < 6:
            lg = eng.decode(kv, [1], force_tokens=torch.tensor([ref_ids[t]]), want_logits=True)
            torch.cuda.synchronize()
    assert kv.length(1) == a + b + 6 and kv.length(0) == a
    if diverged:
        print(f'greedy picks differed from the oracle at measured near-ties, steps {diverged}')
    kv.free()


CLEAR_SEQS = (0, 63, 64, 65)       # 66 sequences: past the 64 threads of the truncate kernel's workgroup and the 64 entries of its sequence list
CLEAR_KEEP = 5                     # positions truncate / fork keep of the 8-row prompt
SAMPLING = dict(temperature=100.0, seed=20240229)


@pytest.fixture(scope='module')
def fresh(setup):
    """What a sequence that never had a feature switched on computes for the 8-row prompt at penalty 1.5, with n = 0 and n = CLEAR_KEEP of its positions
    cached already (the cached prefix is the prompt's own: prefill, then truncate): {n: (raw logits, greedy id, the id SAMPLING picks instead)}."""
    eng = setup['eng']
    P = prompt(8, 77).cuda()
    out = {}
    for n in (0, CLEAR_KEEP):
        kv = eng.kv_alloc(2, 64)
        for s in (0, 1):
            if n:
                eng.prefill(kv, s, P)
                kv.truncate(s, n)
            if s:
                kv.set_sampling(s, **SAMPLING)
            lg = eng.prefill(kv, s, P[:, n:], penalty=1.5, want_logits=True).clone()
            if s == 0:
                logits = lg
        out[n] = (logits, kv.generated(0)[0], kv.generated(1)[0])
        kv.free()
    return P, out


@pytest.mark.parametrize('way', ['reset_seq', 'reset_all', 'truncate', 'fork'])
def test_every_way_of_clearing_forgets_everything(setup, fresh, way):
    """Sequences 0, 63, 64 and 65 of a 66-sequence cache carry every per-sequence feature that coexists (a stop budget that has fired, sampling, token
    scores, a constraint that bans the id a fresh sequence picks), sequences 10 and 11 are a prefilled beam group.  After reset(seq), reset(),
    truncate(seq, n > 0) or fork(src, [seq], n) a sequence computes the bits of one that never had a feature on."""
    from callireader_amd._binding import CalliReaderError
    from callireader_amd.constraints import Constraints
    eng = setup['eng']
    P, ref = fresh
    n = CLEAR_KEEP if way in ('truncate', 'fork') else 0
    logits, greedy_id, sampled_id = ref[n]
    for k in ref:
        assert ref[k][2] != ref[k][1], (k, ref[k][1:])              # SAMPLING picks another id than greedy: sampling left on would show
    N = 66
    kv = eng.kv_alloc(N, 64)
    for s in CLEAR_SEQS:
        kv.set_stop(s, max_new=1)
        kv.set_sampling(s, **SAMPLING)
        kv.set_logprobs(s, 3)
        kv.set_constraints(s, Constraints(suppress_tokens=(greedy_id,)))
        eng.prefill(kv, s, P, penalty=1.5)
        eng.decode(kv, [s], penalty=1.5)
    kv.set_beam(10, 2, eos_id=None, max_new=8)
    eng.prefill(kv, 10, P)
    eng.prefill(kv, 20, P)                                           # the fork's source: a plain sequence
    got = poll(kv)
    for s in CLEAR_SEQS:
        assert got[1 + N + s] == 1 and len(kv.generated(s)) == 2 and greedy_id not in kv.generated(s)[:1]
        assert len(kv.logprobs(s)[0]) == 2
    assert got[0] >= len(CLEAR_SEQS)
    with pytest.raises(CalliReaderError, match=STATE):
        kv.truncate(10, 3)
    if way == 'reset_all':
        kv.reset()
        assert poll(kv)[0] == 0                                      # the finished ring starts over
    for s in CLEAR_SEQS:
        if way == 'reset_seq':
            kv.reset(s)
        elif way == 'truncate':
            kv.truncate(s, n)
        elif way == 'fork':
            kv.fork(20, [s], n)
    got = poll(kv)
    for s in CLEAR_SEQS:
        assert kv.length(s) == n and kv.generated(s) == []
        assert got[1 + N + s] == 0, s                                # no stop
        with pytest.raises(CalliReaderError, match=STATE):
            kv.logprobs(s)
        lg = eng.prefill(kv, s, P[:, n:], penalty=1.5, want_logits=True)
        assert torch.equal(lg, logits), (s, float((lg - logits).abs().max()))
        assert kv.generated(s) == [greedy_id], (s, kv.generated(s), greedy_id, sampled_id)
    assert all(v == 0 for v in poll(kv)[1 + N:]), 'a budget outlived the clear'
    if way in ('reset_seq', 'reset_all'):
        if way == 'reset_seq':
            kv.reset(11)                                             # one member: the group goes as a whole
        kv.truncate(10, 3 if way == 'reset_seq' else 0)              # the other member: no STATE error any more
        assert kv.length(10) == (3 if way == 'reset_seq' else 0)
        kv.reset(10)
        assert poll(kv)[1 + N + 10] == 0
        kv.set_beam(10, 2, eos_id=None, max_new=8)                   # accepted again
        eng.prefill(kv, 10, P)
        assert kv.length(11) == 8
    kv.free()

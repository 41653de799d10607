"""cr_llm_score_batch on a real MI355X: a continued prefill that makes no pick and scores given targets (reduced model of tests/test_gpu_llm.py:
2 LLM layers, full width, vocab 8201).

Oracle: oracle.internlm2.model_forward(all_logits=True) on the full rows, oracle.generate.apply_repetition_penalty over the targets before a row, float64
log-softmax.  Bounds, as the issue states them:
  - raw logits of every scored row within decode_checks.ATOL / RTOL_L2 of the oracle's (the project's calibrated bf16 noise floor);
  - lp within 1e-5 of the float64 log-softmax of the RETURNED raw rows after the host penalty (tests/test_gpu_logprobs.py's derivation for |z| <= 32);
  - lp within 2 * max(penalty, 1) * ATOL of the oracle's value: the target entry and the log-sum-exp each move by at most the penalised logit error."""
import ctypes as C

import pytest
import torch

from callireader_amd.config import ModelDims
from callireader_amd import synthetic

from decode_checks import ATOL, RTOL_L2, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
V = 8201


@pytest.fixture(scope='module')
def setup():
    from callireader_amd.engine import Engine
    dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=V)
    sd = synthetic.make_state_dict(dims, parts=('llm',), seed=0)
    eng = Engine(dims, max_pos=2048)
    eng.load_state_dict(sd)
    eng.load_rope()
    eng.finalize()
    return dict(eng=eng, dims=dims, sd=sd, table=sd['language_model.model.tok_embeddings.weight'])


def prompt(S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S, 4096, generator=g) * 0.02).to(torch.bfloat16)


def answer(T, seed):
    """T ids with repeats (a pool of about T / 2 + 1 ids), so that the penalty has something to do"""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randperm(V, generator=g)[:T // 2 + 1]
    return pool[torch.randint(0, len(pool), (T,), generator=g)].tolist()


def rows_of(setup, P, y, seed):
    """(rows [P + T - 1, 4096] bf16 on the CPU, targets): prompt ++ embed(y[:-1]), [-1] * (P - 1) ++ y"""
    e = prompt(P, seed)
    if len(y) > 1:
        e = torch.cat([e, setup['table'][torch.tensor(y[:-1])].to(torch.bfloat16)], dim=0)
    return e, [-1] * (P - 1) + list(y)


def host_penalty(row, hist, penalty):
    from oracle.generate import apply_repetition_penalty
    return apply_repetition_penalty(row, list(hist), penalty)


_oracle = {}


def oracle_logits(setup, P, T, seed):
    """The oracle's logits of the scored rows [T, V] fp32, computed once per case"""
    key = (P, T, seed)
    if key not in _oracle:
        from oracle import internlm2
        y = answer(T, seed)
        e, _ = rows_of(setup, P, y, seed)
        with torch.no_grad():
            lg, _ = internlm2.model_forward(setup['sd'], 2, inputs_embeds=e[None], all_logits=True)
        _oracle[key] = lg[0, P - 1:].float()
    return _oracle[key]


@pytest.mark.parametrize('P,T', [(40, 37), (17, 130), (1, 1)])       # crosses a 32-row wave / a 128-row block / the smallest call
@pytest.mark.parametrize('penalty', [1.0, 1.5])
def test_scores_against_the_oracle(setup, P, T, penalty):
    eng = setup['eng']
    seed = 1000 + P
    y = answer(T, seed)
    e, targets = rows_of(setup, P, y, seed)
    ref = oracle_logits(setup, P, T, seed)
    kv = eng.kv_alloc(1, 512)
    try:
        (ts,), lg = eng.score_batch(kv, [0], [e.cuda()], [targets], penalty=penalty, top_n=5, want_logits=True)
        torch.cuda.synchronize()
        lg = lg.cpu()
        assert lg.shape == (T, V) and len(ts) == T and ts.top_ids.shape == (T, 5)
        assert kv.length(0) == P + T - 1 and kv.generated(0) == []
        worst_abs = worst_rel = worst_own = worst_ref = 0.0
        for j in range(T):
            worst_abs = max(worst_abs, float((lg[j] - ref[j]).abs().max()))
            worst_rel = max(worst_rel, rel_l2(lg[j], ref[j]))
            own = torch.log_softmax(host_penalty(lg[j], y[:j], penalty).double(), -1)
            want = torch.log_softmax(host_penalty(ref[j], y[:j], penalty).double(), -1)
            worst_own = max(worst_own, abs(float(ts.logprobs[j]) - float(own[y[j]])))
            worst_ref = max(worst_ref, abs(float(ts.logprobs[j]) - float(want[y[j]])))
            order = torch.sort(host_penalty(lg[j], y[:j], penalty), descending=True, stable=True).indices[:5]
            assert ts.top_ids[j].tolist() == order.tolist(), j
            assert float((torch.as_tensor(ts.top_logprobs[j]).double() - own[order]).abs().max()) <= TOL, j
        print(f'P={P} T={T} penalty={penalty}: logits max|d| {worst_abs:.4f} rel-L2 {worst_rel:.4f}; lp vs own float64 {worst_own:.2e}, vs oracle {worst_ref:.4f}')
        assert worst_abs <= ATOL and worst_rel <= RTOL_L2
        assert worst_own <= TOL
        assert worst_ref <= 2 * max(penalty, 1.0) * ATOL
    finally:
        kv.free()


def test_head_tiles_do_not_change_a_row(setup):
    """300 scored rows (two head tiles: 256 + 44) alone, and as the first of four sequences (402 scored rows: 256 + 146): the same bits, logits included"""
    eng = setup['eng']
    lens = [300, 5, 64, 33]
    ys = [answer(n, 50 + i) for i, n in enumerate(lens)]
    rows = [rows_of(setup, 1, y, 60 + i) for i, y in enumerate(ys)]
    kv = eng.kv_alloc(4, 512)
    try:
        (a,), la = eng.score_batch(kv, [0], [rows[0][0].cuda()], [rows[0][1]], penalty=1.5, top_n=3, want_logits=True)
        kv.reset()
        many, lb = eng.score_batch(kv, [2, 0, 3, 1], [r[0].cuda() for r in rows], [r[1] for r in rows], penalty=1.5, top_n=3, want_logits=True)
        assert [len(t) for t in many] == lens and [kv.length(s) for s in (2, 0, 3, 1)] == lens
        b = many[0]
        assert (a.logprobs.view('int32') == b.logprobs.view('int32')).all() and (a.top_ids == b.top_ids).all()
        assert (a.top_logprobs.view('int32') == b.top_logprobs.view('int32')).all()
        assert torch.equal(la, lb[:300])
    finally:
        kv.free()


def test_the_cache_is_what_a_prefill_leaves(setup):
    eng = setup['eng']
    y = answer(60, 7)
    e, targets = rows_of(setup, 45, y, 7)
    S = e.shape[0]
    kv, kv2 = eng.kv_alloc(2, 256), eng.kv_alloc(2, 256)
    try:
        eng.score_batch(kv, [1], [e.cuda()], [targets], penalty=1.5, top_n=1)
        eng.prefill_batch(kv2, [1], [e.cuda()], penalty=1.5)
        assert kv.length(1) == kv2.length(1) == S and kv.length(0) == 0
        assert kv.generated(1) == [] and len(kv2.generated(1)) == 1
        for pos in (0, S // 2, S - 1):
            for which in (0, 1):
                assert torch.equal(kv.read(1, 1, pos, which), kv2.read(1, 1, pos, which)), (pos, which)
        ft = torch.tensor([y[-1]])
        l1 = eng.decode(kv, [1], penalty=1.0, force_tokens=ft, want_logits=True)
        l2 = eng.decode(kv2, [1], penalty=1.0, force_tokens=ft, want_logits=True)
        assert torch.equal(l1, l2) and kv.length(1) == S + 1
    finally:
        kv.free(); kv2.free()


def test_forked_prefix_and_batching(setup):
    """A 50-row prefix forked to two sequences, two different answers scored in one call: each equals the same answer scored alone on a fork"""
    eng, table = setup['eng'], setup['table']
    pre = prompt(50, 3)
    ys = [answer(20, 31), answer(33, 32)]

    def tail(y):       # the prefix is cached whole: roll the fork back one row and feed that row again
        return torch.cat([pre[49:], table[torch.tensor(y[:-1])].to(torch.bfloat16)], dim=0).cuda()
    kv = eng.kv_alloc(3, 256)
    try:
        eng.prefill(kv, 0, pre.cuda())
        kv.fork(0, [1, 2], 49)
        both, lb = eng.score_batch(kv, [1, 2], [tail(y) for y in ys], [list(y) for y in ys], penalty=1.5, top_n=2, want_logits=True)
        assert [kv.length(s) for s in (0, 1, 2)] == [50, 49 + 20, 49 + 33]
        r0 = 0
        for i, y in enumerate(ys):
            kv.fork(0, [2 - i], 49)                                   # the other slot, too: a row's bits do not depend on its sequence
            (one,), lo = eng.score_batch(kv, [2 - i], [tail(y)], [list(y)], penalty=1.5, top_n=2, want_logits=True)
            assert (one.logprobs.view('int32') == both[i].logprobs.view('int32')).all() and (one.top_ids == both[i].top_ids).all()
            assert (one.top_logprobs.view('int32') == both[i].top_logprobs.view('int32')).all()
            assert torch.equal(lo, lb[r0:r0 + len(y)])
            r0 += len(y)
    finally:
        kv.free()


def test_refusals_change_nothing(setup):
    from callireader_amd import _binding as B
    from callireader_amd._binding import CalliReaderError
    eng = setup['eng']
    e, targets = rows_of(setup, 4, answer(3, 1), 1)
    e = e.cuda()
    kv, kv8 = eng.kv_alloc(4, 16), eng.kv_alloc(1, 16, dtype='e4m3')
    try:
        eng.prefill(kv, 3, prompt(5, 2).cuda())                      # sequence 3 holds a generated id
        kv.set_beam(1, 2, max_new=4)                                 # sequences 1 and 2 are a beam group
        lens0 = [kv.length(s) for s in range(4)]

        def refused(code, seqs, embeds, tg, kvx=kv, **kw):
            with pytest.raises(CalliReaderError, match=f'error {code}:'):
                eng.score_batch(kvx, seqs, embeds, tg, **kw)
            assert [kv.length(s) for s in range(4)] == lens0 and kv8.length(0) == 0 and kv.generated(0) == []
        refused(-1, [4], [e], [targets])                             # out of range
        refused(-1, [-1], [e], [targets])
        refused(-1, [0, 0], [e, e], [targets, targets])              # listed twice
        refused(-1, [0], [e[:0]], [[]])                              # lens <= 0
        big = torch.cat([e, e, e])
        refused(-1, [0], [big], [[-1] * 17 + [5]])                   # rows exceed the cache (16)
        refused(-1, [0], [e], [[-1] * 6])                            # no scored row
        refused(-1, [0], [e], [targets[:-1] + [V]])                  # target >= vocab
        refused(-1, [0], [e], [targets], kvx=kv8)                    # an e4m3 cache
        refused(-1, [1], [e], [targets])                             # members of a beam group
        refused(-1, [2], [e], [targets])
        refused(-3, [3], [e], [targets])                             # holds generated ids
        refused(-1, [0], [e], [targets], penalty=0.0)
        # top_n outside 0..8: the binding's own check comes first, so ask the library
        lp = torch.empty(8, device='cuda')
        ti, tl = torch.empty(8, 8, dtype=torch.int32, device='cuda'), torch.empty(8, 8, device='cuda')
        for bad in (-1, 9):
            rc = B.lib.cr_llm_score_batch(eng._h, kv._h, (C.c_int32 * 1)(0), 1, C.c_void_p(e.data_ptr()), (C.c_int32 * 1)(6), (C.c_int64 * 6)(*targets), 1.0, bad,
                                          C.c_void_p(lp.data_ptr()), C.c_void_p(ti.data_ptr()), C.c_void_p(tl.data_ptr()), None, None)
            assert rc == -1
        with pytest.raises(ValueError):
            eng.score_batch(kv, [0], [e], [targets], top_n=9)
        assert [kv.length(s) for s in range(4)] == lens0
        # and the same call is accepted once nothing is wrong; a truncate makes sequence 3 scorable
        (ts,) = eng.score_batch(kv, [0], [e], [targets], penalty=1.5)
        assert len(ts) == 3 and ts.top_ids.shape == (3, 0) and kv.length(0) == 6
        kv.truncate(3, 4)
        (t3,) = eng.score_batch(kv, [3], [e], [targets], penalty=1.5)
        assert len(t3) == 3 and kv.length(3) == 10
    finally:
        kv.free(); kv8.free()


def test_fp8_mfma_option(setup):
    """cr_enable_fp8_mfma: the call runs on a >= 256-row input and returns finite values; switching it off restores the bf16 bits"""
    eng = setup['eng']
    y = answer(40, 9)
    e, targets = rows_of(setup, 260, y, 9)
    kv = eng.kv_alloc(1, 512)
    try:
        (a,), la = eng.score_batch(kv, [0], [e.cuda()], [targets], penalty=1.5, top_n=2, want_logits=True)
        eng.enable_fp8_mfma(True)
        try:
            kv.reset()
            (f,), lf = eng.score_batch(kv, [0], [e.cuda()], [targets], penalty=1.5, top_n=2, want_logits=True)
        finally:
            eng.enable_fp8_mfma(False)
        assert torch.isfinite(lf).all() and torch.isfinite(torch.as_tensor(f.logprobs)).all() and torch.isfinite(torch.as_tensor(f.top_logprobs)).all()
        assert not torch.equal(lf, la)                               # the option did take the e4m3 path
        kv.reset()
        (b,), lb = eng.score_batch(kv, [0], [e.cuda()], [targets], penalty=1.5, top_n=2, want_logits=True)
        assert torch.equal(la, lb) and (a.logprobs.view('int32') == b.logprobs.view('int32')).all() and (a.top_ids == b.top_ids).all()
    finally:
        kv.free()

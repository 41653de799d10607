"""CPU checks of the shared attention reference (tests/attn_ref.py) and of the inputs test_gpu_prefill_attention.py builds: what the GPU tests rely on
is confirmed here without a GPU."""
import math

import torch

import test_gpu_prefill_attention as T
from attn_ref import attn_f64, attn_ref, rb, segments_ref


def test_reference_stays_finite_on_the_poisoned_launch():
    """The poisoned launch of test_nothing_outside_a_segments_range_is_read_or_written (4 heads over 1 KV head here: the property is per head): NaN in
    everything a segment must not read.  attn_ref over prefix + page reads positions < pos0 + S of the segment's slot only, so it is finite on these
    inputs -- and equals the reference on the same launch without the poison, bit for bit."""
    segs = T.segments(T.LENS, T.SLOTS, T.POS0, gap=5)
    rows = segs[-1][0] + segs[-1][1] + 64
    q, kc, vc = T.random_launch(4, 1, segs, T.N_SLOTS, T.MAX_TOKENS, seed=44, rows=rows, poison=True)
    assert torch.isnan(q[segs[0][1]:segs[1][0]]).all() and torch.isnan(q[-64:]).all() and torch.isnan(kc[4]).all() and torch.isnan(vc[15]).all()
    for row0, S, pos0, slot in segs:
        assert not torch.isnan(kc[slot, :, :pos0 + S]).any() and torch.isnan(kc[slot, :, pos0 + S:]).all()
    clean = T.random_launch(4, 1, segs, T.N_SLOTS, T.MAX_TOKENS, seed=44, rows=rows)
    ref, ref_clean = segments_ref(q, kc, vc, segs, T.SDIV), segments_ref(*clean, segs, T.SDIV)
    for i in ref:
        assert torch.isfinite(ref[i]).all() and torch.equal(ref[i], ref_clean[i])


def test_segments_ref_is_causal_over_prefix_plus_page():
    """Row r of a page that starts at pos0 attends over positions 0 .. pos0 + r: the row's output is the plain softmax attention of that many keys, and
    the float64 form agrees with the rounded one to bf16 accuracy."""
    segs = [(3, 70, 63, 2), (0, 3, 0, 0)]
    q, kc, vc = T.random_launch(4, 2, segs, 3, 140, seed=1)
    ref, exact = segments_ref(q, kc, vc, segs, T.SDIV), segments_ref(q, kc, vc, segs, T.SDIV, fn=attn_f64)
    for r in (0, 1, 64, 69):
        n = 63 + r + 1
        for h in range(4):
            s = (q[3 + r, h].double() @ kc[2, h // 2, :n].double().T) / T.SDIV
            row = torch.softmax(s, -1) @ vc[2, h // 2, :n].double()
            torch.testing.assert_close(exact[0][r, h], row, rtol=1e-12, atol=1e-12)
    for i in ref:
        torch.testing.assert_close(ref[i].double(), exact[i], rtol=T.RTOL, atol=T.ATOL)
    one = attn_ref(q[:3, :1].float().permute(1, 0, 2)[None], kc[0, :1, :3].float()[None], vc[0, :1, :3].float()[None], True, 0, 1.0, T.SDIV)
    assert torch.equal(one[0, 0], ref[1][:, 0])


def test_peaked_cases_plant_what_they_say():
    """The planted scores of peaked_case, read back through the reference's own rounding (a short page keeps this cheap for `random`; the planted
    keys need the full length)."""
    for pos0 in T.PEAK_POS0:
        q, kc, _, segs = T.peaked_case('late', pos0)
        S = segs[0][1]
        r = torch.arange(S)
        late = r + pos0 >= T.PEAK_KEY
        s = T.rb(T.rb(torch.einsum('nd,kd->nk', q[:, 0].float(), kc[1, 0, :T.PEAK_KEY + 1].float())) / T.SDIV)
        before, at = s[:, :T.PEAK_KEY].amax(-1), s[:, T.PEAK_KEY]
        assert float((at - before)[late & (r % 32 == 3)].min()) > 8 and float((at - before)[late & (r % 32 == 9)].min()) > 100
        assert float((at - before)[late & (r % 32 == 4)].max()) < 8
        q, kc, _, _ = T.peaked_case('sink', pos0)
        s = T.rb(T.rb(q[:, 5].float() @ kc[1, 1, 0].float()) / T.SDIV)
        assert float(s.min()) > 36 and float(s.max()) < 44
        q, kc, _, _ = T.peaked_case('negative', pos0)
        s = T.rb(T.rb(torch.einsum('nd,kd->nk', q[5:7, 0].float(), kc[1, 0, :200].float())) / T.SDIV)
        assert float(s.max()) < -30
    assert set(T.PEAKED_FLOOR) == {(n, p) for n in T.PEAKED for p in T.PEAK_POS0}


# ---- the perceiver attention's reference and cases (test_gpu_calli_ops.py) -------------------------------------------------------------------
import test_gpu_calli_ops as C  # noqa: E402
from attn_ref import perceiver_attn_ref, perceiver_heads  # noqa: E402


def test_perceiver_ref_is_the_oracles_einsum_path():
    """perceiver_attn_ref (fp32 with the rounding points written out) against oracle.calli_align.perceiver_softmax_pv on the bf16 tensors themselves -- the
    einsum path perceiver_attention runs.  Bit for bit where achievable: the oracle's bf16 einsum sums in another order, so one bf16 step of the result is allowed and
    the number of differing elements printed (0 or 1 of 7680 per case)."""
    from oracle import calli_align
    for name in C.DATA_CASES:
        q, kv, ref = C.data_case(name)
        q, kv, ref = *C.first_tiles(q, kv, 5), ref[:15]
        qh, k, v = perceiver_heads(q, kv)
        orc = calli_align.perceiver_softmax_pv(qh, k, v).permute(0, 2, 1, 3).reshape(15, 512)
        assert orc.dtype == torch.bfloat16
        diff = orc.float() != ref
        step = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)
        print(f'perceiver_attn_ref vs the oracle, {name}: {int(diff.sum())} of {diff.numel()} elements differ')
        assert bool(((orc.float() - ref).abs() <= step).all())


PERCEIVER_MISTAKES = {
    'key 258 masked': dict(drop_keys=(258,)),
    'keys 256..258 masked': dict(drop_keys=(256, 257, 258)),
    'sim - amax unrounded': dict(round_sub=False),
    'probabilities unrounded': dict(round_p=False),
}
# Which (case, mistake) the data cases' bound -- assert_close(rtol = RTOL, atol = max(ATOL, 2 x floor)) against perceiver_attn_ref at T = 37 -- sees.
# The key masks show on every case: among 888 rows some give a latent key a large weight (and the exact cases pin every key bit for bit).  The two
# left-out roundings move an ordinary row by ~ 3e-3, and a bound of 2 x the reference's own distance from float64 cannot see that in principle: what
# the rounding moves IS part of that distance.  So `random`, `spread`, `late` and `negative` do not see them; binade_case is built so that the
# reference's roundings cancel and each alone does not (its docstring), and sees both.
_MASKS = ('key 258 masked', 'keys 256..258 masked')
PERCEIVER_SEEN = {
    'random': _MASKS,
    'spread': _MASKS,
    'late': _MASKS,
    'negative': _MASKS,
    'binade': _MASKS + ('sim - amax unrounded', 'probabilities unrounded'),
}


def _passes(got, ref, atol):
    try:
        torch.testing.assert_close(got, ref, rtol=C.RTOL, atol=atol)
        return True
    except AssertionError:
        return False


def test_perceiver_bound_sees_the_mistakes_it_claims_to():
    """Each mistake of PERCEIVER_MISTAKES, made in the reference, against the bound the GPU test uses: it must FAIL on the cases PERCEIVER_SEEN names (and
    every mistake on at least one case), the true reference must pass, and so must its float64 form (that is what the floor means)."""
    seen_somewhere = set()
    for name in C.DATA_CASES:
        q, kv, ref = C.data_case(name)
        atol = C.allowed_atol(name, C.T_MAX)
        assert _passes(perceiver_attn_ref(q, kv), ref, atol)
        assert _passes(perceiver_attn_ref(q, kv, exact=True).float(), ref, atol)
        for what, kw in PERCEIVER_MISTAKES.items():
            got = perceiver_attn_ref(q, kv, **kw)
            excess = float(((got - ref).abs() - C.RTOL * ref.abs()).max())
            fails = not _passes(got, ref, atol)
            print(f'{name:9s} {what:24s}: worst |mistake - ref| - rtol |ref| = {excess:10.3e} against {atol:.3e}: {"FAILS" if fails else "passes (not seen)"}')
            assert fails == (what in PERCEIVER_SEEN[name]), (name, what, excess, atol)
            if fails:
                seen_somewhere.add(what)
    assert seen_somewhere == set(PERCEIVER_MISTAKES)


def test_perceiver_floors_are_the_measured_ones():
    """DATA_FLOOR is what scripts/perceiver_attention_calibrate.py prints for the cases as they are built now (a changed builder must not keep an old floor)."""
    for name in C.DATA_CASES:
        q, kv, ref = C.data_case(name)
        exact = perceiver_attn_ref(q, kv, exact=True)
        for j, T in enumerate(C.TS):
            floor = max(0.0, float(((ref[:T * 3].double() - exact[:T * 3]).abs() - C.RTOL * exact[:T * 3].abs()).max()))
            assert abs(floor - C.DATA_FLOOR[name][j]) <= 1e-3 * floor + 1e-6, (name, T, floor)


def test_perceiver_cases_plant_what_they_say():
    rb = C.rb
    # uniform: the expected output is what the reference gives, and every probability is 253 * 2^-16
    q, kv, exp = C.uniform_case(5)
    assert float(torch.tensor(1 / 259).to(torch.bfloat16)) == 253 * 2.0 ** -16
    assert torch.equal(perceiver_attn_ref(q, kv), exp.float())
    # selection: the reference returns the target's V row; every key is a target, the edges of the kernel's key loops among them
    for per_query in (False, True):
        q, kv, exp, tg = C.selection_case(per_query=per_query)
        assert set(tg.reshape(-1).tolist()) == set(range(259)) and set(C.SELECT_MUST) <= set(tg.reshape(-1).tolist())
        assert torch.equal(perceiver_attn_ref(q, kv), exp.float())
        qh, k, _ = perceiver_heads(q, kv)
        s = rb(rb(qh.float() * 0.125) @ k.float().transpose(-1, -2))
        assert sorted(set(s.reshape(-1).tolist())) == [0.0, 128.0] and bool((s.argmax(-1) == tg).all()) and int((s == 128).sum()) == tg.numel()
        assert float(torch.exp(torch.tensor(-128.0))) == 0.0
        if per_query:
            assert len({int(tg[0, 0, i]) for i in range(3)}) == 3
    # spread / late / negative
    qh, k, _ = perceiver_heads(*C.spread_case(5))
    s = rb(rb(qh.float() * 0.125) @ k.float().transpose(-1, -2))
    assert 2.7 < float(s.std()) < 3.3
    qh, k, _ = perceiver_heads(*C.late_case())
    s = rb(rb(qh.float() * 0.125) @ k.float().transpose(-1, -2))
    keys = torch.tensor([[C.late_key(t, h) for h in range(8)] for t in range(C.T_MAX)])
    assert bool((s[:, :, 1].argmax(-1) == keys).all()) and set(keys.reshape(-1).tolist()) == {256, 257, 258}
    top2 = s[:, :, 1].topk(2, -1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) > 0.5 and float(s[:, :, 1].softmax(-1).amax(-1).median()) > 0.9
    qh, k, _ = perceiver_heads(*C.negative_case(5))
    s = rb(rb(qh.float() * 0.125) @ k.float().transpose(-1, -2))
    assert float(s[:, :, 2].max()) < -28 and float(s[:, :, 2].min()) > -56
    # binade: the roundings its docstring lists
    q, kv = C.binade_case(5)
    qh, k, v = perceiver_heads(q, kv)
    exact = (qh.double() * 0.125) @ k.double().transpose(-1, -2)
    s = rb(exact.float())
    dom = torch.tensor([[C.binade_key(t, h) for h in range(8)] for t in range(5)])
    assert bool((s.argmax(-1) == dom[:, :, None]).all()) and {int(x) for x in dom.reshape(-1)} >= {256, 257, 258} and int(dom.min()) < 256
    assert sorted(set(s.reshape(-1).tolist())) == [-6.0, 0.5234375] and abs(float(exact.min()) + 6.006165) < 1e-6
    d = s - s.amax(-1, keepdim=True)
    assert sorted(set(d.reshape(-1).tolist())) == [-6.5234375, 0.0] and sorted(set(rb(d).reshape(-1).tolist())) == [-6.53125, 0.0]
    p = torch.softmax(rb(d), -1)
    assert sorted(set(rb(p).reshape(-1).tolist())) == [0.00106048583984375, 0.7265625]
    for x in sorted(set(p.reshape(-1).tolist())):                                              # far from a rounding boundary: > 0.2 % either side
        assert float(rb(torch.tensor(x * 1.002))) == float(rb(torch.tensor(x * 0.998)))
    assert float(v.float().abs().min()) >= 32 and float(perceiver_attn_ref(q, kv).abs().max()) < 0.5


# ---- the ViT attention's cases (test_gpu_vit_attention.py) ---------------------------------------------------------------------------------------------------
import test_gpu_vit_attention as W  # noqa: E402


def test_vit_codes_are_the_gold_set():
    c = W.gold_codes()
    assert c.shape == (4095, 63) and set(c.reshape(-1).tolist()) == {-1.0, 1.0}
    gram = c @ c.T
    assert bool((gram.diagonal() == 63).all())
    assert set((gram - 63 * torch.eye(4095)).reshape(-1).tolist()) == {-17.0, -1.0, 0.0, 15.0}      # 0: the diagonal itself


def test_vit_exact_cases_select_what_they_say():
    """Every case of EXACT_CASES, as built: q, k, v survive a bf16 round trip; the reference's bf16 scores ARE the float64 scores; every query's largest score is
    on its permutation's key, 24 or more above the runner-up; it lies the intended delta above the CLS key's score (a query that selects the CLS key: the CLS
    key 30 or more above every patch key); every key is some query's target; attn_ref returns the V rows exactly."""
    for name, kw in W.EXACT_CASES.items():
        c = W.exact_case(**kw)
        S, Bn, H, q, k, v, target, delta = (c[n] for n in ('S', 'Bn', 'H', 'q', 'k', 'v', 'target', 'delta'))
        assert S in (257, 385, 1025) and q.shape == k.shape == v.shape == (Bn, H, S, 64)
        for t in (q, k, v):
            assert torch.equal(rb(t), t)
        assert float(v.abs().min()) >= 1 and float(v.abs().max()) <= 64 and torch.equal(v, v.round())
        s = rb(rb(q * 0.125) @ k.transpose(-1, -2))
        assert torch.equal(s.double(), (q.double() * 0.125) @ k.double().transpose(-1, -2))
        top = s.topk(2, -1)
        assert torch.equal(top.indices[..., 0], target) and float((top.values[..., 0] - top.values[..., 1]).min()) >= 24, name
        assert bool((target.sort(-1).values == torch.arange(S)).all())
        to_cls = target == 0
        assert torch.equal(to_cls, delta.isnan()) and int(to_cls.sum()) == Bn * H
        assert torch.equal((top.values[..., 0] - s[..., 0])[~to_cls], delta[~to_cls])
        assert float((s[..., 0] - s[..., 1:].amax(-1))[to_cls].min()) >= 30
        want = torch.full((Bn, H, S), float(kw.get('delta', 40)))
        for b, h, r0, r1, d in kw.get('flagged', ()):
            want[b, h, r0:r1] = d
            assert not bool(to_cls[b, h, r0:r1].any()) or r1 - r0 > 1, name                        # a single flagged query is flagged
        assert torch.equal(delta[~to_cls], want[~to_cls])
        assert torch.equal(attn_ref(q, k, v, False, 0, 0.125, 1.0), c['expected']), name
        # the CLS query's targets over the (batch, head) pairs: every 32-key half of every block and the CLS key, where the launch has pairs enough
        nch = W.n_cls_choices(S)
        cls_t = target[:, :, 0].reshape(-1)
        choice = torch.where(cls_t == 0, nch - 1, (cls_t - 1) // 32)
        assert len(set(choice.tolist())) == min(nch, Bn * H), name
    for names in (W.ORDINARY, W.CLS_EDGES):
        for name in names:
            c = W.exact_case(**W.EXACT_CASES[name])
            assert c['Bn'] * c['H'] >= W.n_cls_choices(c['S'])
    assert {W.EXACT_CASES[n]['S'] for n in W.ORDINARY} == {257, 385, 1025}
    assert sum(((kw['S'] - 1) // 128 * kw['Bn'] * kw['H']) % 8 != 0 for kw in W.EXACT_CASES.values()) >= 2
    assert len(W.ORDINARY) + len(W.DELTAS) + len(W.PLACED) + len(W.CLS_EDGES) == len(W.EXACT_CASES)


def test_vit_exact_cases_are_exact_on_the_generic_kernel_too():
    """attention.hip sums its fp32 probabilities and multiplies V by their bf16 roundings, so its weights sum to 1 only to bf16 accuracy.  On the delta = 40
    cases its reference point is the first tile's maximum: 63 where the target (or, 93, the CLS key as target) is in that tile -- probability 1 -- and otherwise
    23, the CLS key's score, since no other patch score exceeds 15.  Then the target's probability is bf16(e^40) against a row sum of e^40 (1 + 1e-17): the
    output is V times a factor that rounds every integer |V| <= 64 back to itself."""
    for name in W.ORDINARY:
        c = W.exact_case(**W.EXACT_CASES[name])
        s = rb(rb(c['q'] * 0.125) @ c['k'].transpose(-1, -2))
        first = s[..., :64].amax(-1)
        assert set(first.reshape(-1).tolist()) <= {23.0, 63.0, 93.0}
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    p = torch.exp2(torch.tensor(63.0) * log2e - torch.tensor(23.0) * log2e)                        # fp32, as the kernel forms it
    factor = float(rb(p)) / math.exp(40.0)
    assert abs(factor - 1) < 4e-4
    ints = torch.arange(1, 65).float()
    for f in (factor * (1 - 1e-5), factor * (1 + 1e-5)):                                            # v_exp_f32 and the fp32 roundings: far inside
        assert torch.equal(rb(ints * f), ints)


def test_vit_uniform_case_sees_a_key_dropped_doubled_or_swapped():
    """uniform_case: the float64 expectation per column, and what each mistake does to it -- any one key left out, any one key counted twice, any tile read in
    place of a neighbour (whose tile % 4 differs): some column moves by more than two bf16 steps, the GPU test allows one."""
    for S, Bn, H in W.UNIFORM_SHAPES:
        q, k, v, expect = W.uniform_case(S, Bn, H)
        assert not bool(q.any()) and torch.equal(rb(k), k) and torch.equal(rb(v), v) and bool((v == v[0, 0]).all())
        v0 = v[0, 0].double()
        tot = v0.sum(0)
        assert torch.equal(expect, tot / S) and bool((tot == tot[0]).all())
        torch.testing.assert_close(W._attn_ref(q, k, v, False, 0, 0.125, 1.0).double(), expect.expand(Bn, H, S, 64), rtol=0, atol=float(W.bf16_step(expect).max()))
        step = W.bf16_step(expect)
        dropped = ((tot - v0) / (S - 1) - expect).abs() / step                                      # row j: key j left out
        doubled = ((tot + v0) / (S + 1) - expect).abs() / step
        assert float(dropped.amax(-1).min()) > 2 and float(doubled.amax(-1).min()) > 2
        nt = (S - 1) // 64
        tiles = v0[1:].reshape(nt, 64, 64).sum(1)                                                    # (tile, column)
        for t in range(nt):
            for other in (t - 1, t + 1):
                if 0 <= other < nt:
                    assert t % 4 != other % 4
                    moved = ((tot - tiles[t] + tiles[other]) / S - expect).abs() / step
                    assert float(moved.max()) > 2


def test_vit_strided_case_pads_with_nan_and_shares_no_stride():
    for S, Bn, H in W.STRIDED_SHAPES:
        bufs, lays, ref = W.strided_case(S, Bn, H)
        for i in range(3):                                                                           # batch, head, row strides
            assert len({lays[n][i] for n in 'qkvo'}) == 4
        for n in 'qkv':
            assert all(x % 8 == 0 for x in lays[n][:4])
            inside = torch.zeros(lays[n][4], dtype=torch.bool)
            W.strided_view(inside, lays[n], S, Bn, H).fill_(True)
            assert int(inside.sum()) == Bn * H * S * 64                                              # no two elements share a place
            assert bool(bufs[n][~inside].isnan().all()) and not bool(bufs[n][inside].isnan().any())
            assert not bool(inside[:lays[n][3]].any()) and not bool(inside[-8:].any())               # padding in front of the first and behind the last element
        assert all(x % 4 == 0 for x in lays['o'][:4]) and lays['o'][2] > H * 64
        bs, hs, rs, off, _ = lays['k']                                                               # head-major planes: a NaN row before row 0 and after row S - 1
        for b in range(Bn):
            for h in range(H):
                p0 = off + b * bs + h * hs
                assert bool(bufs['k'][p0 - 64:p0].isnan().all()) and bool(bufs['k'][p0 + S * 64:p0 + S * 64 + 64].isnan().all())
        assert bool(torch.isfinite(ref).all())

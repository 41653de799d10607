"""attention_vit.hip alone, through cr_op_attention, at what its four tests in test_gpu_ops.py cannot see.

A. Exact key selection.  Every query -- the CLS query too -- selects ONE key by integer-valued scores, the map from query to key is a random permutation per
   (batch, head), and the output row must be that key's V row bit for bit (torch.equal).  The scores are exact in any summation order, so nothing about the
   kernel's schedule may show.  How far the winning score lies above the CLS key's (the lean sweep's reference point) is the case's knob DELTA: 40 is
   ordinary, 60 .. 68 is the band just below the flag (row sums up to e^68 ~ 3e29 < 2^100), 72 .. 300 is flagged (finite sums, then overflowing ones).
B. Every key counted once.  Q = 0, so every key weighs 1 / S, and V says which keys were summed: one bf16 step of the float64 value.
C. Four buffers with four layouts, NaN in every gap: a stride taken from the wrong operand, or a row outside [0, S), shows.

Shapes: S = 257 (nb = 2, the smallest the kernel takes), 385 (an odd block count), 1025 (the product's); workgroup counts nb * H * B that are no multiple of
8 among them (the remainder branch of the XCD renumbering).  Every case runs under the four-wave and the two-wave form, and where it says so under the
generic kernel (attention.hip).  Every output is pre-filled with 7.0: a block nobody computed shows.

The builders are plain functions; tests/test_attn_ref_cpu.py confirms on the CPU what they claim.
"""
import functools
import zlib

import pytest
import torch

from attn_ref import attn_ref as _attn_ref

pytestmark = pytest.mark.gpu

RTOL = 1.6e-2
ATOL = 1.5e-2
D = 64
SENTINEL = 7.0
FORMS = {
    'four_waves': {'CR_VIT_ATTN': '1', 'CR_VIT_ATTN_NW': '4'},
    'two_waves': {'CR_VIT_ATTN': '1', 'CR_VIT_ATTN_NW': '2'},
    'generic': {'CR_VIT_ATTN': '0', 'CR_VIT_ATTN_NW': '4'},
}
VIT_FORMS = ('four_waves', 'two_waves')
CLS_SCORE_OF_A_CLS_QUERY = 93                                  # 30 above the largest score a patch key can reach (63)


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def E():
    from callireader_amd import engine
    return engine


def set_form(monkeypatch, form):
    for name, value in FORMS[form].items():                   # both are read per call (attention_vit.hip)
        monkeypatch.setenv(name, value)


# ---- A. exact key selection ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gold_codes():
    """4095 codes in {-1, +1}^63 any two of which have the dot product -17, -1 or 15: the 65 Gold sequences of length 63 (the m-sequence u of x^6 + x + 1, its
    decimation by 5, and u xor every cyclic shift of that) in all 63 cyclic shifts.  A token's code against its own gives 63, so a query built from one
    code selects one key with a gap of 48 to every other patch key whichever S codes a case draws -- no drawing until the gap happens to hold."""
    a = [1, 0, 0, 0, 0, 0]
    for i in range(57):
        a.append(a[i] ^ a[i + 1])
    u = torch.tensor(a)
    v = u[(5 * torch.arange(63)) % 63]
    base = torch.stack([u, v] + [u ^ v.roll(s) for s in range(63)])
    return (1 - 2 * torch.cat([base.roll(s, 1) for s in range(63)])).float()


def n_cls_choices(S):
    return 4 * ((S - 1) // 128) + 1                            # the CLS query's partials: a 32-key half of a block each, and the CLS key


@functools.lru_cache(maxsize=None)
def exact_case(S, Bn, H, delta=40, flagged=(), cls_off=None, rot=0, seed=0):
    """q, k, v (Bn, H, S, 64) fp32 holding bf16 values, target (Bn, H, S): query i of a (batch, head) selects key target[i], a random permutation of the S tokens.

    Token j has a code c_j (gold_codes, drawn and sign-flipped per (batch, head)).  Patch key j = 2 c_j in dims 0 .. 62 and 0 in dim 63; the CLS key is 0 in
    dims 0 .. 62 and 8 in dim 63.  Query i = 4 c_target(i) with q[63] = u_i.  With q_prescale = 0.125 the score against patch key j is the integer
    c_target(i) . c_j -- 63 on the target, <= 15 elsewhere -- and against the CLS key u_i = 63 - delta: the winning score lies delta above the CLS key's.  A
    query whose target IS the CLS key takes the CLS token's code and u_i = 93.  V holds non-zero integers in +-[1, 64].
    delta: the same for every query, except flagged = ((batch, head, first row, end row, delta), ...).
    The CLS query's target: (batch, head) pair i takes choice (i + rot) % (4 nb + 1) -- choice c < 4 nb is a key of the c-th 32-key half (cls_off inside the
    half; None: drawn), choice 4 nb the CLS key -- so the pairs of one launch walk over the partials the combine kernel merges.
    Returns a dict; 'delta' is NaN where the target is the CLS key."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((S, Bn, H, delta, flagged, cls_off, rot, seed)).encode()))
    codes = gold_codes()
    nch = n_cls_choices(S)
    q, k = torch.zeros(Bn, H, S, D), torch.zeros(Bn, H, S, D)
    v = torch.empty(Bn, H, S, D)
    target = torch.empty(Bn, H, S, dtype=torch.long)
    dl = torch.full((Bn, H, S), float(delta))
    for b, h, r0, r1, d in flagged:
        dl[b, h, r0:r1] = float(d)
    for b in range(Bn):
        for h in range(H):
            code = codes[torch.randperm(codes.shape[0], generator=g)[:S]] * (torch.randint(0, 2, (63,), generator=g) * 2 - 1).float()
            perm = torch.randperm(S, generator=g)
            c = (b * H + h + rot) % nch
            off = int(torch.randint(0, 32, (1,), generator=g)) if cls_off is None else cls_off
            t = 0 if c == nch - 1 else 1 + 32 * c + off
            j = int((perm == t).nonzero())
            perm[j], perm[0] = perm[0].clone(), t
            k[b, h, 1:, :63] = 2 * code[1:]
            k[b, h, 0, 63] = 8
            q[b, h, :, :63] = 4 * code[perm]
            q[b, h, :, 63] = torch.where(perm == 0, torch.tensor(float(CLS_SCORE_OF_A_CLS_QUERY)), 63 - dl[b, h])
            dl[b, h][perm == 0] = float('nan')
            v[b, h] = torch.randint(1, 65, (S, D), generator=g).float() * (torch.randint(0, 2, (S, D), generator=g) * 2 - 1).float()
            target[b, h] = perm
    expected = torch.gather(v, 2, target[..., None].expand(-1, -1, -1, D))
    return dict(S=S, Bn=Bn, H=H, q=q, k=k, v=v, target=target, delta=dl, expected=expected)


def _last_row_of_block(qb):
    return 1 + qb * 128 + 127                                  # the last lane of the block's last wave (two-wave form: of its second sub-block)


BAND = (60, 66, 68)                                            # below 2^100 = e^69.3: the lean sweep at its largest magnitudes
FLAGGED = (72, 80, 100, 300)                                   # e^72, e^80: finite row sums >= 2^100; e^100, e^300: not finite in fp32
EXACT_CASES = {
    # A1 (and A4: the pairs of each launch walk over every choice of the CLS query's target): (B, H) with B * H >= 4 nb + 1
    'ordinary-257': dict(S=257, Bn=3, H=5),                    # 30 workgroups
    'ordinary-385': dict(S=385, Bn=1, H=13),                   # 39
    'ordinary-1025': dict(S=1025, Bn=3, H=11),                 # 264
    # A3: one place flagged, everything else in the launch clean
    'one-query-385': dict(S=385, Bn=1, H=3, flagged=((0, 1, _last_row_of_block(2), _last_row_of_block(2) + 1, 80),)),       # 9 workgroups
    'one-query-1025': dict(S=1025, Bn=1, H=2, flagged=((0, 1, _last_row_of_block(5), _last_row_of_block(5) + 1, 80),)),
    'one-block-385': dict(S=385, Bn=2, H=3, flagged=((1, 2, 129, 257, 80),)),                                               # (batch 1, head 2, block 1)
    'one-block-1025': dict(S=1025, Bn=2, H=3, flagged=((1, 2, 129, 257, 80),)),
    'flag-word-263': dict(S=1025, Bn=1, H=33, flagged=((0, 32, 1 + 7 * 128, 1025, 80),)),   # H * nb = 264 flag words: the exact kernel's second trip
}
# ... and the same places 300 above: at 80 the lean sweep's own result is still the V row (e^80 is finite), so only these show that the flagged block WAS redone
for _n in [n for n in EXACT_CASES if n.startswith(('one-', 'flag-'))]:
    EXACT_CASES[_n + '-d300'] = dict(EXACT_CASES[_n], flagged=tuple(f[:4] + (300,) for f in EXACT_CASES[_n]['flagged']))
for _S, _Bn, _H in ((385, 1, 3), (1025, 2, 2)):                 # A2: every query at the same distance; the pairs' CLS targets start elsewhere per delta
    for _d in BAND + FLAGGED:
        EXACT_CASES[f'delta-{_d}-{_S}'] = dict(S=_S, Bn=_Bn, H=_H, delta=_d, rot=_d)
for _S, _Bn, _H in ((257, 3, 3), (385, 1, 13), (1025, 3, 11)):  # A4: the first and the last key of every 32-key half, and the CLS key
    EXACT_CASES[f'cls-first-{_S}'] = dict(S=_S, Bn=_Bn, H=_H, cls_off=0, rot=3)
    EXACT_CASES[f'cls-last-{_S}'] = dict(S=_S, Bn=_Bn, H=_H, cls_off=31, rot=7)
ORDINARY = tuple(n for n in EXACT_CASES if n.startswith('ordinary'))
DELTAS = tuple(n for n in EXACT_CASES if n.startswith('delta'))
PLACED = tuple(n for n in EXACT_CASES if n.startswith(('one-', 'flag-')))
CLS_EDGES = tuple(n for n in EXACT_CASES if n.startswith('cls-'))


def launch(E, q, k, v, q_prescale=0.125):
    """(Bn, H, S, 64) tensors -> the kernel's output in the same layout, run on (Bn, S, H, 64) buffers (one layout for all four: section C has the others)."""
    Bn, H, S, _ = q.shape
    qd, kd, vd = (t.bfloat16().permute(0, 2, 1, 3).contiguous().to(dev()) for t in (q, k, v))
    o = torch.full((Bn, S, H, D), SENTINEL, device=dev(), dtype=torch.bfloat16)
    E.op_attention(qd, kd, vd, o, [S * H * D, H * D, D] * 4, Bn, H, S, S, D, q_prescale=q_prescale)
    torch.cuda.synchronize()
    return o.permute(0, 2, 1, 3).float().cpu()


def check_exact(E, name):
    c = exact_case(**EXACT_CASES[name])
    out = launch(E, c['q'], c['k'], c['v'])
    bad = (out != c['expected']).any(-1)
    if bool(bad.any()):
        where = bad.nonzero()
        b, h, r = (int(x) for x in where[0])
        cols = (out[b, h, r] != c['expected'][b, h, r]).nonzero().reshape(-1)[:8].tolist()
        pytest.fail(f'{name}: {len(where)} of {bad.numel()} rows are not their key\'s V row; (batch, head, row) {where[:12].tolist()}; row ({b}, {h}, {r}) selects '
                    f'key {int(c["target"][b, h, r])}, columns {cols}: got {out[b, h, r, cols].tolist()}, V row {c["expected"][b, h, r, cols].tolist()}')
    assert torch.equal(out, c['expected'])


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('name', ORDINARY)
def test_attention_vit_exact_key_selection(E, monkeypatch, name, form):
    """A1: delta = 40 everywhere.  The generic kernel too: its reference point is the first tile's maximum, the CLS key's 23 (every patch score but the
    target's is <= 15), so a later target's probability is bf16(e^40) = 209 * 2^50 against a row sum of 209.07 * 2^50 -- the output is V * (1 - 3.4e-4), which
    rounds to V for every |V| <= 64 (half a bf16 step is >= 2^-9 relative)."""
    set_form(monkeypatch, form)
    check_exact(E, name)


@pytest.mark.parametrize('form', VIT_FORMS)
@pytest.mark.parametrize('name', DELTAS)
def test_attention_vit_exact_below_and_above_the_flag(E, monkeypatch, name, form):
    """A2: every query 60, 66, 68 above its reference point (the lean sweep, probabilities up to e^68), or 72, 80 (flagged by a finite row sum >= 2^100), 100,
    300 (by a row sum that is not finite): every block of the launch takes the same path, and either path returns the V row."""
    set_form(monkeypatch, form)
    check_exact(E, name)


@pytest.mark.parametrize('form', VIT_FORMS)
@pytest.mark.parametrize('name', PLACED)
def test_attention_vit_exact_where_the_flag_sits(E, monkeypatch, name, form):
    """A3: one flagged place in a clean launch -- a single query in the last lane of its block's last wave; one block of (batch 1, head 2) with head 0 and
    batch 0 clean; flag word 263 of 264, behind the exact kernel's first 256.  Each at 80 above the reference point (a finite row sum; the lean result would
    still be right, so this holds the exact sweep's result to the V row) and at 300 (the lean result is NaN: the block must have been redone)."""
    set_form(monkeypatch, form)
    check_exact(E, name)


@pytest.mark.parametrize('form', VIT_FORMS)
@pytest.mark.parametrize('name', CLS_EDGES)
def test_attention_vit_exact_cls_query_over_every_partial(E, monkeypatch, name, form):
    """A4: the CLS query selects the first (then the last) key of every 32-key half of every block, and the CLS key, over the (batch, head) pairs of one
    launch: each of the 4 nb + 1 partials carries the whole result once, through vit_cls_combine_kernel<33> (S = 1025) and vit_cls_combine_any_kernel."""
    set_form(monkeypatch, form)
    c = exact_case(**EXACT_CASES[name])
    want = {0} | {1 + 32 * half + EXACT_CASES[name]['cls_off'] for half in range(n_cls_choices(c['S']) - 1)}
    assert set(c['target'][:, :, 0].reshape(-1).tolist()) == want
    check_exact(E, name)


# ---- B. every key counted once --------------------------------------------------------------------------------------------------------------------

UNIFORM_SHAPES = ((257, 3, 5), (385, 1, 3), (1025, 2, 2))


@functools.lru_cache(maxsize=None)
def uniform_case(S, Bn, H):
    """Q = 0: every score is 0 whatever K holds (random integers), every key weighs 1 / S.  V[1 + j, j % 64] = 1 + (j // 64) % 4 for patch key j (one entry per
    key: its column says which key of a tile it is, its value which tile, up to 4), the CLS row is 1 in every column.  Returns q, k, v (Bn, H, S, 64)
    and the float64 expectation per column, (64,): the same for every query of every (batch, head)."""
    g = torch.Generator().manual_seed(S)
    k = torch.randint(-8, 9, (Bn, H, S, D), generator=g).float()
    v = torch.zeros(S, D)
    j = torch.arange(S - 1)
    v[1 + j, j % 64] = (1 + (j // 64) % 4).float()
    v[0] = 1.0
    return torch.zeros(Bn, H, S, D), k, v.expand(Bn, H, S, D).contiguous(), v.double().sum(0) / S


def bf16_step(x):
    """The distance between neighbouring bf16 values at |x| (a float64 tensor)."""
    return torch.exp2(torch.floor(torch.log2(x.abs())) - 7)


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('S,Bn,H', UNIFORM_SHAPES)
def test_attention_vit_uniform_weights_count_every_key_once(E, monkeypatch, S, Bn, H, form):
    """B: each output column is (a small integer) / S.  The numerator is exact in fp32 (integers), the kernel then rounds 1 / l and the product in fp32 and the
    result to bf16: one bf16 step of the float64 value.  (The lean sweep's weights sum to exactly 1: it adds nothing.)  A key left out, counted twice or
    taken from a neighbouring tile moves some column by more than two steps (test_attn_ref_cpu.py)."""
    set_form(monkeypatch, form)
    q, k, v, expect = uniform_case(S, Bn, H)
    out = launch(E, q, k, v).double()
    err = (out - expect).abs() / bf16_step(expect)
    worst = float(err.max())
    print(f'uniform S={S} {form}: worst distance from the float64 value {worst:.3f} bf16 steps')
    assert worst <= 1.0, [int(x) for x in (err > 1.0).nonzero()[0]]


# ---- C. distinct strides, and nothing else touched --------------------------------------------------------------------------------------------

STRIDED_SHAPES = ((257, 3, 5), (385, 1, 3), (1025, 2, 2))


def strided_layouts(S, Bn, H):
    """(batch, head, row stride, offset of element 0, buffer elements) of q, k, v, o: every stride a multiple of 8 (o: of 4), no two operands alike in any.
    q: row-major, heads padded to 72; k: head-major planes with one row of padding before, between and after them; v: row-major with padded rows;
    o: row-major, heads padded to 68 and rows padded."""
    lay = {}
    q_rs = H * 72 + 8
    lay['q'] = (S * q_rs + 16, 72, q_rs, 8)
    k_hs = S * 64 + 64
    lay['k'] = (H * k_hs + 128, k_hs, 64, 64)
    v_rs = H * 64 + 40
    lay['v'] = (S * v_rs + 48, 64, v_rs, 24)
    o_rs = H * 68 + 4
    lay['o'] = (S * o_rs + 12, 68, o_rs, 4)
    for i in range(3):
        assert len({lay[n][i] for n in 'qkvo'}) == 4, (i, lay)
    return {n: (bs, hs, rs, off, off + Bn * bs) for n, (bs, hs, rs, off) in lay.items()}


def strided_view(buf, lay, S, Bn, H):
    bs, hs, rs, off, _ = lay
    return buf.as_strided((Bn, H, S, D), (bs, hs, rs, 1), off)


@functools.lru_cache(maxsize=None)
def strided_case(S, Bn, H):
    """Random q, k, v (Bn, H, S, 64) bf16 laid into NaN-filled buffers by strided_layouts, and attn_ref of them.  Returns (buffers, layouts, ref)."""
    g = torch.Generator().manual_seed(100 + S)
    lays = strided_layouts(S, Bn, H)
    bufs, t = {}, {}
    for n in 'qkv':
        t[n] = torch.randn(Bn, H, S, D, generator=g).bfloat16()
        bufs[n] = torch.full((lays[n][4],), float('nan'), dtype=torch.bfloat16)
        strided_view(bufs[n], lays[n], S, Bn, H).copy_(t[n])
    ref = _attn_ref(t['q'].float(), t['k'].float(), t['v'].float(), False, 0, 0.125, 1.0)
    return bufs, lays, ref


@pytest.mark.parametrize('S,Bn,H', STRIDED_SHAPES)
def test_attention_vit_distinct_strides_and_nothing_else_touched(E, monkeypatch, S, Bn, H):
    """C: q, k, v and o in four buffers with four layouts.  Everything around the operands is NaN (q, k, v) or the sentinel (o): the result is finite, within
    the suite's bound of attn_ref and within 2^-7 of the generic kernel on the same buffers; the two ViT forms give the same bits; o's padding and the three
    inputs are bit for bit what they were."""
    bufs, lays, ref = strided_case(S, Bn, H)
    d = {n: bufs[n].to(dev()) for n in 'qkv'}
    view = {n: strided_view(d[n], lays[n], S, Bn, H) for n in 'qkv'}
    strides = [x for n in 'qkvo' for x in (lays[n][0], lays[n][2], lays[n][1])]                     # (batch, row, head) per operand
    valid = torch.zeros(lays['o'][4], dtype=torch.bool)
    strided_view(valid, lays['o'], S, Bn, H).fill_(True)
    assert int(valid.sum()) == Bn * H * S * D and not bool(valid.all())
    out = {}
    for form in FORMS:
        set_form(monkeypatch, form)
        ob = torch.full((lays['o'][4],), SENTINEL, device=dev(), dtype=torch.bfloat16)
        E.op_attention(view['q'], view['k'], view['v'], strided_view(ob, lays['o'], S, Bn, H), strides, Bn, H, S, S, D, q_prescale=0.125)
        torch.cuda.synchronize()
        ob = ob.cpu()
        assert bool((ob[~valid] == SENTINEL).all()), f'{form}: {int((ob[~valid] != SENTINEL).sum())} elements of the output\'s padding were written'
        out[form] = strided_view(ob, lays['o'], S, Bn, H).float()
        assert bool(torch.isfinite(out[form]).all()), f'{form}: {int((~torch.isfinite(out[form])).sum())} elements are not finite'
    for n in 'qkv':
        assert torch.equal(d[n].cpu().view(torch.int16), bufs[n].view(torch.int16)), n
    for form in FORMS:
        print(f'strided S={S} {form}: largest difference from attn_ref {float((out[form] - ref).abs().max()):.4f}, '
              f'from the generic kernel {float((out[form] - out["generic"]).abs().max()):.4f}')
    for form in FORMS:
        torch.testing.assert_close(out[form], ref, rtol=RTOL, atol=ATOL)
        assert float((out[form] - out['generic']).abs().max()) <= 2 ** -7
    assert torch.equal(out['two_waves'], out['four_waves'])

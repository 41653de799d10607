"""The CalliAlign stage's own kernels, each alone, on a real MI355X (csrc/calli.hip): the perceiver attention (cr_op_perceiver_attention: the launch
cr_resample makes, both kernels), the LayerNorm's output-row regrouping (cr_op_layernorm_regroup: the fill cr_resample uses), vq_pick_kernel's merge of
the per-block arg-max partials over more blocks than it has threads, and cr_vq's row chunking.  The case builders run on the CPU: tests/test_attn_ref_cpu.py
checks there what the cases plant and which mistakes the bounds below can see; scripts/perceiver_attention_calibrate.py prints the floors."""
import math

import pytest
import torch

from attn_ref import P_DH, P_HEADS, P_NKV, P_NQ, perceiver_attn_ref, rb

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1.6e-2, 1.5e-2
TS = (1, 5, 37)                       # tiles per launch; the cases are built for 37, a smaller launch takes the first tiles
T_MAX = TS[-1]
SENTINEL = 0x7BCD                     # bf16 bit pattern (2.13e36): no case's expected output holds it


def assemble(qh, k, v):
    """q (T, 8, 3, 64), k / v (T, 8, 259, 64) -> the entry's operands: q (T * 3, 512), kv (T * 259, 1024) [K | V] bf16."""
    T = qh.shape[0]
    q = qh.permute(0, 2, 1, 3).reshape(T * P_NQ, P_HEADS * P_DH)
    kv = torch.stack((k, v)).permute(1, 3, 0, 2, 4).reshape(T * P_NKV, 2 * P_HEADS * P_DH)
    return q.to(torch.bfloat16).contiguous(), kv.to(torch.bfloat16).contiguous()


def first_tiles(q, kv, T):
    return q[:T * P_NQ].contiguous(), kv[:T * P_NKV].contiguous()


def one_tile(q, kv, t):
    return q[t * P_NQ:(t + 1) * P_NQ].contiguous(), kv[t * P_NKV:(t + 1) * P_NKV].contiguous()


def _randn(shape, g, std):
    return rb(torch.randn(shape, generator=g) * std)


# ---- exact cases -------------------------------------------------------------------------------------------------------------------------
def uniform_case(T=T_MAX, seed=1):
    """q = 0: every score is 0, every probability bf16(1 / 259) = 253 * 2^-16.  V holds integers |v| <= 64, so every fp32 partial sum of p * v is an integer
    multiple of 2^-16 below 2^24 of them (253 * 64 * 259 < 2^23): exact in any order.  K is random (nothing of it may reach the output).  Returns q, kv and
    the expected output bf16(bf16(1 / 259) * sum over the keys of v), computed in float64."""
    g = torch.Generator().manual_seed(seed)
    qh = torch.zeros(T, P_HEADS, P_NQ, P_DH)
    k = _randn((T, P_HEADS, P_NKV, P_DH), g, 1.3)
    v = torch.randint(-64, 65, (T, P_HEADS, P_NKV, P_DH), generator=g).float()
    p = torch.tensor(1.0 / P_NKV).to(torch.bfloat16).double()
    exp = (p * v.double().sum(2, keepdim=True)).expand(-1, -1, P_NQ, -1)                    # (T, 8, 3, 64)
    exp = exp.permute(0, 2, 1, 3).reshape(T * P_NQ, P_HEADS * P_DH).to(torch.bfloat16)
    return assemble(qh, k, v) + (exp,)


SELECT_MUST = (0, 63, 64, 127, 128, 255, 256, 257, 258)


def selection_targets(T=T_MAX, per_query=False):
    """The key each (tile, head, query) selects, (T, 8, 3): 100 is coprime to 259, so any 259 consecutive rows of the launch cover every key."""
    if per_query:
        return ((torch.arange(T * P_HEADS * P_NQ) * 100 + 58) % P_NKV).reshape(T, P_HEADS, P_NQ)
    return ((torch.arange(T * P_HEADS) * 100 + 58) % P_NKV).reshape(T, P_HEADS, 1).expand(-1, -1, P_NQ)      # a (tile, head)'s three queries share a target


def selection_case(T=T_MAX, per_query=False, seed=2):
    """One key takes the whole weight: its score is 128, every other score 0, and exp(-128) is 0 in fp32 -- the output is the target's V row for that
    head, bit for bit.  per_query = False: the query rows are all 4.0 (0.5 after the scale) and the target's K row of that head is all 4.0 (64 * 0.5 * 4);
    the three queries of a (tile, head) meet the same keys, so they share the target.  per_query = True: query i is 16.0 on dims 16 i .. 16 i + 15 only
    and ITS target is 4.0 on those dims (16 * 2 * 4 = 128; a query scores 0 on the other queries' targets), so a swapped query row shows too.
    Other heads' K columns and other tiles' rows hold other targets.  Returns q, kv, the expected output and the targets."""
    g = torch.Generator().manual_seed(seed)
    tg = selection_targets(T, per_query)
    qh = torch.zeros(T, P_HEADS, P_NQ, P_DH)
    k = torch.zeros(T, P_HEADS, P_NKV, P_DH)
    v = _randn((T, P_HEADS, P_NKV, P_DH), g, 1.3)
    t_i, h_i = torch.meshgrid(torch.arange(T), torch.arange(P_HEADS), indexing='ij')
    for i in range(P_NQ):
        dims = slice(16 * i, 16 * i + 16) if per_query else slice(0, P_DH)
        qh[:, :, i, dims] = 16.0 if per_query else 4.0
        k[t_i, h_i, tg[:, :, i], dims] = 4.0
    exp = torch.stack([v[t_i, h_i, tg[:, :, i]] for i in range(P_NQ)], 2)                    # (T, 8, 3, 64)
    exp = exp.permute(0, 2, 1, 3).reshape(T * P_NQ, P_HEADS * P_DH).to(torch.bfloat16)
    return assemble(qh, k, v) + (exp, tg)


# ---- data cases --------------------------------------------------------------------------------------------------------------------------
# q, k and v of layer 0 as the oracle computes them on test_gpu_calli.py's features (N(0, 0.7), synthetic weights, seed 0) all have standard deviation
# 1.28-1.29; the scores' is 1.65, the largest softmax weight of a row 0.04 .. 0.45, the three latent keys carry 1.1 % of the mass
# (scripts/perceiver_attention_calibrate.py prints these)
STAGE_STD = 1.28

# binade_case: the constants of its construction (derived in its docstring, confirmed by test_attn_ref_cpu.py)
BIN_K_LOW = (-6.0, -101 * 2.0 ** -14)       # a low key's K: exact score -6 - 101 * 2^-14, which bf16 rounds to -6 (+ 6.165e-3)
BIN_K_DOM = (0.5, 3 * 2.0 ** -7)            # the dominant key's K: score 0.5234375, a bf16 value
BIN_RHO = 0.7265625 / (258 * 0.00106048583984375)      # bf16(p_dom) / (258 * bf16(p_low)): v_low = -BIN_RHO * v_dom makes the row's output cancel


def random_case(T=T_MAX, seed=3):
    g = torch.Generator().manual_seed(seed)
    return assemble(_randn((T, P_HEADS, P_NQ, P_DH), g, STAGE_STD), _randn((T, P_HEADS, P_NKV, P_DH), g, STAGE_STD), _randn((T, P_HEADS, P_NKV, P_DH), g, STAGE_STD))


def _spread(T, seed):
    g = torch.Generator().manual_seed(seed)
    s = math.sqrt(3.0)                                                                         # scores 0.125 * q . k: standard deviation 3
    return _randn((T, P_HEADS, P_NQ, P_DH), g, s), _randn((T, P_HEADS, P_NKV, P_DH), g, s), _randn((T, P_HEADS, P_NKV, P_DH), g, STAGE_STD)


def spread_case(T=T_MAX, seed=4):
    """Scores with standard deviation 3: a row's largest weight is 0.1 .. 0.9, a handful of keys carry it."""
    return assemble(*_spread(T, seed))


def late_key(t, h):
    return 256 + (t + h) % 3


def late_case(T=T_MAX, seed=5):
    """spread_case with one late dominant key among the latents: in every (tile, head) the K row of latent key 256 + (tile + head) % 3 is 0.6 x the head's
    query 1, whose score there is 0.125 * 0.6 * |q|^2 ~ 14 against a largest other score of ~ 9; queries 0 and 2 see one more ordinary key."""
    qh, k, v = _spread(T, seed)
    for t in range(T):
        for h in range(P_HEADS):
            k[t, h, late_key(t, h)] = rb(0.6 * qh[t, h, 1])
    return assemble(qh, k, v)


def negative_case(T=T_MAX, seed=6):
    """spread_case with every score of query 2 near -40 in every (tile, head): dims 0..7 of every K row are -6.5 and of query 2 +6.5 (0.125 * 8 * -42.25);
    near -40 a bf16 score moves in steps of 0.25.  Queries 0 and 1 get a shift common to all their keys."""
    qh, k, v = _spread(T, seed)
    k[..., :8] = -6.5
    qh[:, :, 2, :8] = 6.5
    return assemble(qh, k, v)


def binade_key(t, h):
    return (256 + (t + h) % 3) if (t + h) % 2 == 0 else (37 * t + 11 * h) % 256


def binade_case(T=T_MAX, seed=7):
    """Rows built so that the reference's roundings of sim - amax and of the probabilities each MATTER and the reference still equals exact arithmetic --
    the only kind of row on which a bound of 2 x (the reference's own distance from float64) can tell a kernel that leaves one of them out.
    Every query is (8, 8, 0, ...) (1, 1 after the scale).  258 low keys have K = BIN_K_LOW: exact score -6.006165, which bf16 rounds to -6 (+6.165e-3).
    One dominant key (binade_key: a latent or a media key) has K = BIN_K_DOM: score m = 0.5234375.  sim - amax = -6.5234375 is no bf16 value: it rounds
    to -6.53125 (-7.8125e-3).  So the reference's exponent is 1.648e-3 below the exact one, -6.529602, and that makes up for what its bf16 probabilities
    do: p_dom = 0.72677 -> 0.7265625 (-2.84e-4), p_low = 1.05903e-3 -> 1.06049e-3 (+1.370e-3), whose ratio is exp(6.529602 + 5e-6).
    V is v_dom (|v| in 32..64, random per tile, head and dim) at the dominant key and -BIN_RHO * v_dom at the others: the output cancels to ~ 0 in
    the reference and in float64 alike, while leaving sim - amax unrounded moves it by 5.7e-3 * v_dom and leaving the probabilities unrounded by
    1.2e-3 * v_dom.  Both probabilities lie 0.3 % and more from a bf16 rounding boundary, far outside what another exp or summation order moves them."""
    g = torch.Generator().manual_seed(seed)
    qh = torch.zeros(T, P_HEADS, P_NQ, P_DH)
    qh[..., :2] = 8.0
    k = torch.zeros(T, P_HEADS, P_NKV, P_DH)
    k[..., 0], k[..., 1] = BIN_K_LOW
    vd = (32 + 32 * torch.rand(T, P_HEADS, P_DH, generator=g)) * (torch.randint(0, 2, (T, P_HEADS, P_DH), generator=g) * 2 - 1)
    v = (-BIN_RHO * vd)[:, :, None, :].repeat(1, 1, P_NKV, 1)
    for t in range(T):
        for h in range(P_HEADS):
            k[t, h, binade_key(t, h), 0], k[t, h, binade_key(t, h), 1] = BIN_K_DOM
            v[t, h, binade_key(t, h)] = vd[t, h]
    return assemble(qh, k, v)


DATA_CASES = {'random': random_case, 'spread': spread_case, 'late': late_case, 'negative': negative_case, 'binade': binade_case}

# The smallest atol at which perceiver_attn_ref passes assert_close(rtol = RTOL) against its float64 form on each case's first 1 / 5 / 37 tiles
# (scripts/perceiver_attention_calibrate.py prints this table); a case allows max(ATOL, 2 x floor), the rule of test_gpu_prefill_attention.py.
DATA_FLOOR = {
    'random': (5.599e-03, 6.453e-03, 8.474e-03),        # T = 37: max |ref - f64| 2.886e-02, max |f64| 3.08
    'spread': (3.545e-02, 3.545e-02, 4.234e-02),        # T = 37: max |ref - f64| 5.294e-02, max |f64| 4.17
    'late': (1.663e-02, 1.787e-02, 3.698e-02),          # T = 37: max |ref - f64| 5.155e-02, max |f64| 5.22
    'negative': (1.254e-01, 1.363e-01, 1.758e-01),      # T = 37: max |ref - f64| 1.832e-01, max |f64| 4.77
    'binade': (1.859e-04, 1.859e-04, 1.859e-04),        # T = 37: max |ref - f64| 7.238e-04, max |f64| 0.22
}


def allowed_atol(name, T):
    return max(ATOL, 2 * DATA_FLOOR[name][TS.index(T)])


_cache = {}


def data_case(name):
    """(q, kv, reference) of a data case at T_MAX, built once per process and never modified."""
    if name not in _cache:
        q, kv = DATA_CASES[name]()
        _cache[name] = (q, kv, perceiver_attn_ref(q, kv))
    return _cache[name]


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def E():
    from callireader_amd import engine
    return engine


def bits(t):
    return t.contiguous().view(torch.int16)


def launch(E, q, kv, which):
    """The entry on device copies, the output pre-filled with the sentinel; returns the output on the CPU."""
    out = torch.full((q.shape[0], q.shape[1]), SENTINEL, dtype=torch.int16, device='cuda').view(torch.bfloat16)
    E.op_perceiver_attention(q.cuda(), kv.cuda(), which=which, out=out)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('which', (0, 1))
def test_perceiver_uniform_weights_sum_every_key_once(E, which):
    q, kv, exp = uniform_case()
    assert not (bits(exp) == SENTINEL).any()
    for T in TS:
        got = launch(E, *first_tiles(q, kv, T), which)
        assert torch.equal(bits(got), bits(exp[:T * P_NQ])), f'which={which} T={T}: {int((bits(got) != bits(exp[:T * P_NQ])).sum())} elements differ'


@pytest.mark.parametrize('per_query', (False, True))
@pytest.mark.parametrize('which', (0, 1))
def test_perceiver_selects_each_key(E, which, per_query):
    q, kv, exp, tg = selection_case(per_query=per_query)
    assert set(tg.reshape(-1).tolist()) == set(range(P_NKV)) and set(SELECT_MUST) <= set(tg.reshape(-1).tolist())
    assert not (bits(exp) == SENTINEL).any()
    for T in TS:
        got = launch(E, *first_tiles(q, kv, T), which)
        bad = (bits(got) != bits(exp[:T * P_NQ])).reshape(T, P_NQ, P_HEADS, P_DH).any(-1).nonzero().tolist()
        assert not bad, f'which={which} T={T}: wrong V row at (tile, query, head) {bad[:8]}, targets {[int(tg[t, h, i]) for t, i, h in bad[:8]]}'


@pytest.mark.parametrize('name', list(DATA_CASES))
def test_perceiver_data_cases(E, name):
    q, kv, ref = data_case(name)
    whole = {w: launch(E, q, kv, w) for w in (0, 1)}
    assert torch.equal(bits(whole[0]), bits(whole[1])), 'the two kernels differ at T = 37'
    for T in TS:
        got = whole[0][:T * P_NQ] if T == T_MAX else launch(E, *first_tiles(q, kv, T), 0)
        if T != T_MAX:
            assert torch.equal(bits(got), bits(launch(E, *first_tiles(q, kv, T), 1))), f'the two kernels differ at T = {T}'
        r = ref[:T * P_NQ]
        excess = float(((got.float() - r).abs() - RTOL * r.abs()).max())
        print(f'perceiver {name} T={T}: worst |o - ref| - {RTOL} |ref| = {excess:.3e} (allowed {allowed_atol(name, T):.3e})')
        assert not (bits(got) == SENTINEL).any()
        torch.testing.assert_close(got.float(), r, rtol=RTOL, atol=allowed_atol(name, T))
    one = {w: launch(E, *first_tiles(q, kv, 1), w) for w in (0, 1)}
    assert torch.equal(bits(one[0]), bits(one[1])), 'the two kernels differ at T = 1'
    # a tile alone == the same tile inside the launch of 37
    for t in (0, 17, 36):
        alone = one[0] if t == 0 else launch(E, *one_tile(q, kv, t), 0)
        assert torch.equal(bits(alone), bits(whole[0][t * P_NQ:(t + 1) * P_NQ])), f'tile {t} alone differs from tile {t} of 37'


def test_perceiver_entry_rejects_bad_arguments(E):
    from callireader_amd import _binding as B
    q, kv = first_tiles(*random_case(1), 1)
    q, kv = q.cuda(), kv.cuda()
    out = torch.empty_like(q)
    for which, qq, kk, oo, T in ((2, q, kv, out, 1), (-1, q, kv, out, 1), (0, None, kv, out, 1), (0, q, None, out, 1), (0, q, kv, None, 1), (0, q, kv, out, 0)):
        ptr = [None if x is None else x.data_ptr() for x in (qq, kk, oo)]
        assert B.lib.cr_op_perceiver_attention(which, ptr[0], ptr[1], ptr[2], T, None) == -1
        assert b'cr_op_perceiver_attention' in B.lib.cr_last_error()


# ---- LayerNorm regrouping ----------------------------------------------------------------------------------------------------------------
def test_layernorm_regroup_writes_the_resamplers_cat(E):
    """The two launches with which cr_resample writes cat(norm_media(x), norm_learns(learns)) in place, T = 3: 768 media rows in groups 256 -> 259 at
    offset 0, 9 latent rows in groups 3 -> 259 at offset 256, into one buffer with 4 guard rows."""
    T, n = 3, 4096
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(T * 256, n, generator=g) * 2 + 0.3).to(torch.bfloat16).cuda()
    lat = (torch.randn(T * 3, n, generator=g) * 0.5 - 0.2).to(torch.bfloat16).cuda()
    gm, bm, gl, bl = [(torch.randn(n, generator=g) * 0.1 + o).to(torch.bfloat16).cuda() for o in (1, 0, 1, 0)]
    buf = torch.full((T * 259 + 4, n), SENTINEL, dtype=torch.int16, device='cuda').view(torch.bfloat16)
    E.op_layernorm_regroup(x, buf, gm, bm, 1e-5, 256, 259, 0)
    E.op_layernorm_regroup(lat, buf, gl, bl, 1e-5, 3, 259, 256)
    plain_m, plain_l = E.op_layernorm(x, gm, bm, 1e-5), E.op_layernorm(lat, gl, bl, 1e-5)
    torch.cuda.synchronize()
    want = torch.cat((plain_m.reshape(T, 256, n), plain_l.reshape(T, 3, n)), 1).reshape(T * 259, n)
    assert not (bits(want) == SENTINEL).any()
    assert torch.equal(bits(buf[:T * 259]), bits(want)), f'rows {sorted(set((bits(buf[:T * 259]) != bits(want)).any(1).nonzero().reshape(-1).tolist()))[:12]} differ'
    assert (bits(buf[T * 259:]) == SENTINEL).all(), 'a guard row was written'
    assert not (bits(buf[:T * 259]) == SENTINEL).any()
    # test_gpu_ops.py::test_layernorm's bound against fp32 layer_norm
    F = torch.nn.functional
    ref = torch.cat((rb(F.layer_norm(x.float(), (n,), gm.float(), bm.float(), 1e-5)).reshape(T, 256, n),
                     rb(F.layer_norm(lat.float(), (n,), gl.float(), bl.float(), 1e-5)).reshape(T, 3, n)), 1).reshape(T * 259, n)
    torch.testing.assert_close(buf[:T * 259].float(), ref, rtol=RTOL, atol=1e-2)
    # out_group = 0 is cr_op_layernorm
    same = E.op_layernorm_regroup(x, torch.empty_like(x), gm, bm, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(bits(same), bits(plain_m))


def test_layernorm_regroup_rejects_overlapping_groups(E):
    from callireader_amd import _binding as B
    x = torch.zeros(6, 4096, dtype=torch.bfloat16, device='cuda')
    out = torch.zeros(600, 4096, dtype=torch.bfloat16, device='cuda')
    w = torch.ones(4096, dtype=torch.bfloat16, device='cuda')
    for in_group, out_group, out_off in ((0, 259, 0), (-1, 259, 0), (3, 259, 257), (256, 255, 0), (3, 259, -1)):
        with pytest.raises(B.CalliReaderError, match='cr_op_layernorm_regroup'):
            E.op_layernorm_regroup(x, out, w, w, 1e-5, in_group, out_group, out_off)
    E.op_layernorm_regroup(x, out, w, w, 1e-5, 3, 259, 256)                                   # the largest offset that fits
    with pytest.raises(ValueError):
        E.op_layernorm_regroup(x, out[:300], w, w, 1e-5, 3, 259, 256)                         # the wrapper: row 517 is outside 300 rows
    torch.cuda.synchronize()


# ---- VQ ----------------------------------------------------------------------------------------------------------------------------------
VQ_PAIRS = ((10, 40), (70, 130), (255, 256), (300, 9000), (100, 16484))      # the same 64-column block; adjacent blocks; across the GEMM's 256-column tile;
VQ_LAST = 16499                                                              # different vq_pick threads; blocks 1 and 257 = ONE thread's two blocks, the second ragged


def test_vq_pick_merges_more_blocks_than_threads():
    """Vocabulary 16 500 = 258 blocks of 64 columns (the last one 52 wide): threads 0 and 1 of vq_pick_kernel hold two blocks each.  Row j of the table is
    a copy of row i for each pair, so a query along that row meets two bit-identical similarities, in any arithmetic: the first maximal index must win."""
    from callireader_amd import synthetic
    from callireader_amd.config import ModelDims
    from callireader_amd.engine import Engine
    from oracle import calli_align
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=1, vocab=16500)
    assert (dims.vocab + 63) // 64 == 258 and dims.vocab % 64 == 52 and VQ_LAST == dims.vocab - 1
    table = synthetic.make_state_dict(dims, parts=('vq',), seed=0)['normed_emb.weight'].clone()
    for i, j in VQ_PAIRS:
        assert i < j
        table[j] = table[i]
    eng = Engine(dims)
    eng.load_weight('normed_emb.weight', table)
    eng.finalize()
    rows = [i for i, _ in VQ_PAIRS] + [VQ_LAST]
    x = (3 * table[rows].float()).to(torch.bfloat16)
    ridx, _ = calli_align.vq_cos_sim(table, x[None], use_dynamic_p=True)
    assert ridx.tolist() == rows, 'the oracle itself does not return the first of two equal maxima'
    idx, cos = eng.vq(x.cuda(), with_cos=True)
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == rows
    assert float((cos.float().cpu() - 1).abs().max()) <= 8e-3
    eng.close()


def test_vq_second_row_chunk():
    """cr_vq works through its rows in chunks of 18 432: 18 432 + 70 rows make it take the offsets of a second chunk (idx + r0, cos + r0, in + r0 * D).  One
    call == the two calls on either side of the boundary, bit for bit, and rows planted around the boundary return what was planted."""
    from callireader_amd import synthetic
    from callireader_amd.config import ModelDims
    from callireader_amd.engine import Engine
    CH, D = 18432, 4096
    n = CH + 70
    dims = ModelDims.reduced(vit_layers=1, llm_layers=1, rs_depth=2, vocab=5003)
    table = synthetic.make_state_dict(dims, parts=('vq',), seed=0)['normed_emb.weight']
    eng = Engine(dims)
    eng.load_weight('normed_emb.weight', table)
    eng.finalize()
    g = torch.Generator(device='cuda').manual_seed(13)
    base = torch.randn(257, D, generator=g, device='cuda').to(torch.bfloat16)                 # 257 distinct rows: a row's period is coprime to every tile size
    x = base.repeat((n + 256) // 257, 1)[:n].contiguous()
    planted = {CH - 1: 4321, CH: 17, CH + 1: 5002, n - 1: 2500}
    for r, i in planted.items():
        x[r] = (table[i].float() * 2).to(torch.bfloat16).cuda()
    idx, cos = eng.vq(x, with_cos=True)
    i0, c0 = eng.vq(x[:CH], with_cos=True)
    i1, c1 = eng.vq(x[CH:], with_cos=True)
    torch.cuda.synchronize()
    assert torch.equal(idx, torch.cat((i0, i1))) and torch.equal(bits(cos), bits(torch.cat((c0, c1))))
    assert {r: int(idx[r]) for r in planted} == planted
    assert int(idx.min()) >= 0 and int(idx.max()) < dims.vocab
    # the tiled rows repeat with period 257 wherever nothing was planted: a chunk offset that is off by a row would break this too
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(planted)] = False
    rep = idx[:257].repeat((n + 256) // 257)[:n].cpu()
    assert torch.equal(idx.cpu()[keep], rep[keep])
    eng.close()

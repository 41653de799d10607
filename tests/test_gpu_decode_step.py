"""The batched decode step (9..64 rows; with e4m3 weights 1..64 rows) pinned at the 256-key split boundaries, and the generated-id buffer past 4096 ids.

A bf16 decode step of 9..64 rows runs wqkv as K-sliced fp32 partial sums (gemm_skinny.hip) and decode_attn_kernel<DIV, FOLD = true> (attention_decode.hip),
which sums the slices, rounds, rotates, writes the new token's K / V row into the cache and patches that row into the registers of the lanes that would have
loaded it.  Three kinds of check, all on rows whose NEW position passes 254..259, 510..515 and 766..771 next to rows of 1..65 cached tokens (whose upper
splits are empty while the longest row fixes the split count):

1. the fold, the separate kernels (CR_DECODE_FOLD_ROPE=0) and a row decoded alone (gemm_decode.hip's fused small-batch kernels) give the same bits: logits
   of every row and step, ids, and the K / V cache rows of every new position in both layers; again with e4m3 weights, where batches of 1..64 rows fold;
2. against code that shares nothing with the step: logits and picks of rows inside the batch against the CPU oracle (tests/decode_checks.py: the calibrated
   bounds of test_gpu_llm.py, a differing pick only as a measured near-tie), and the layer-0 K / V rows of every row and step against a closed form in float64;
3. more than 4096 generated ids: a free run and a teacher-forced run over the same ids give the same logits at every step.
"""
import os

import pytest
import torch

from callireader_amd.config import ModelDims
from callireader_amd import synthetic

from decode_checks import check_step

pytestmark = pytest.mark.gpu
STEPS = 6
PENALTY = 1.3
L0 = 'language_model.model.layers.0.'


@pytest.fixture(scope='module')
def setup():
    from callireader_amd.engine import Engine
    dims = ModelDims.reduced(vit_layers=1, llm_layers=2, rs_depth=1, vocab=8201)
    sd = synthetic.make_state_dict(dims, parts=('llm',), seed=0)
    eng = Engine(dims, max_pos=2048)
    eng.load_state_dict(sd)
    eng.load_rope()
    eng.finalize()
    os.environ['CR_DECODE_FOLD_ROPE'] = '0'
    try:
        nofold = Engine(dims, max_pos=2048)
    finally:
        del os.environ['CR_DECODE_FOLD_ROPE']
    nofold.share_weights_from(eng)
    yield dict(eng=eng, nofold=nofold, dims=dims, sd=sd, alone={})
    nofold.close()
    eng.close()


def prompt(S):
    """One prompt per length: a row is the same page in every batch, so its single-row run and its oracle run are made once."""
    g = torch.Generator().manual_seed(3000 + S)
    return (torch.randn(1, S, 4096, generator=g) * 0.02).to(torch.bfloat16)


# Cached tokens before the first step.  Step t appends position len + t: 254 -> 254..259, 510 -> 510..515, 766 -> 766..771 (the new position enters split 1, 2, 3
# at t = 2); 255 / 511 / 767 and 253 / 509 shift the crossing by a step.  The short rows end in split 0: with a long row in the batch their splits 1.. are empty.
BOUNDARY = [254, 510, 766]
SHORT = [1, 2, 3, 15, 16, 17, 62, 63, 64, 65]
FILL = [255, 511, 767, 253, 509, 256, 512, 768, 100, 129, 200, 300, 333, 400, 447, 600, 640, 700, 31, 32, 33, 127, 128, 191, 192, 193, 257, 319, 320, 383,
        384, 385, 448, 449, 513, 575, 576, 577, 639, 641, 703, 704, 705, 765, 769, 5, 8, 48, 90, 150]
BATCHES = {
    9: BOUNDARY + [1, 2, 3, 15, 16, 17],                                          # the longest row (766) is on a boundary
    13: [900] + BOUNDARY[:2] + [62, 63, 64, 65, 1, 16, 17, 255, 511, 3],          # the longest row (900 -> 4 splits) is NOT; 254 and 510 cross under it
    33: BOUNDARY + SHORT + FILL[:20],
    64: [1000] + BOUNDARY + SHORT + FILL[:50],                                    # 1000..1005: no boundary
}
assert all(len(v) == k and len(set(v)) == k for k, v in BATCHES.items())


def slots_and_order(rows):
    """Row i lives in cache slot i + 1 (slot 0 stays empty); the batch lists the rows reversed with the two halves interleaved."""
    rev = list(range(rows - 1, -1, -1))
    order = rev[::2] + rev[1::2]
    return [i + 1 for i in range(rows)], order


def fill(eng, kv, lens):
    for i, S in enumerate(lens):
        eng.prefill(kv, i + 1, prompt(S).cuda(), penalty=PENALTY)


def new_rows(kv, slot, S):
    """K and V of both layers at the STEPS new positions of a row: (STEPS, 2 layers, 2, 8, 128)"""
    return torch.stack([torch.stack([torch.stack([kv.read(layer, slot, S + t, which) for which in (0, 1)]) for layer in (0, 1)]) for t in range(STEPS)])


def run_batch(eng, lens):
    """Free-running decode of the batch with the penalty on: per step logits in ROW order, then ids and the new cache rows of every row."""
    rows = len(lens)
    slots, order = slots_and_order(rows)
    kv = eng.kv_alloc(rows + 1, 1024)
    fill(eng, kv, lens)
    logits = []
    for _ in range(STEPS):
        lg = eng.decode(kv, [slots[i] for i in order], penalty=PENALTY, want_logits=True)
        byrow = torch.empty_like(lg)
        byrow[torch.tensor(order, device=lg.device)] = lg
        logits.append(byrow)
    torch.cuda.synchronize()
    ids = [kv.generated(slots[i]) for i in range(rows)]
    cache = torch.stack([new_rows(kv, slots[i], lens[i]) for i in range(rows)])
    assert [kv.length(s) for s in slots] == [S + STEPS for S in lens] and kv.length(0) == 0
    kv.free()
    return torch.stack(logits), ids, cache


def same_bits(a, b, lens, what):
    """(logits (STEPS, rows, V), ids, cache (rows, STEPS, 2, 2, 8, 128)) of two runs: every row, every step"""
    for t in range(STEPS):
        for i, S in enumerate(lens):
            assert torch.equal(a[0][t, i], b[0][t, i]), (what, 'logits', f'row of {S} tokens', f'step {t}', float((a[0][t, i] - b[0][t, i]).abs().max()))
    for i, S in enumerate(lens):
        assert a[1][i] == b[1][i] and len(a[1][i]) == STEPS + 1, (what, 'ids', f'row of {S} tokens', a[1][i], b[1][i])
        for t in range(STEPS):
            for layer in (0, 1):
                for which in (0, 1):
                    assert torch.equal(a[2][i, t, layer, which], b[2][i, t, layer, which]), \
                        (what, 'VK'[1 - which], f'layer {layer}', f'row of {S} tokens', f'position {S + t}')


def run_alone(setup, S):
    """The row as the only one of its step: the <= 8-row fused kernels of gemm_decode.hip."""
    if S not in setup['alone']:
        eng = setup['eng']
        kv = eng.kv_alloc(2, 1024)
        eng.prefill(kv, 1, prompt(S).cuda(), penalty=PENALTY)
        logits = torch.stack([eng.decode(kv, [1], penalty=PENALTY, want_logits=True)[0] for _ in range(STEPS)])
        torch.cuda.synchronize()
        setup['alone'][S] = (logits, kv.generated(1), new_rows(kv, 1, S))
        kv.free()
    return setup['alone'][S]


@pytest.mark.parametrize('rows', sorted(BATCHES))
def test_fold_separate_and_single_row_give_the_same_bits(setup, rows):
    lens = BATCHES[rows]
    fold = run_batch(setup['eng'], lens)
    sep = run_batch(setup['nofold'], lens)
    same_bits(fold, sep, lens, f'{rows} rows, fold vs separate kernels')
    assert float(fold[0].abs().max()) > 0 and float(fold[2].abs().max()) > 0
    for S in [S for S in lens if S in BOUNDARY] + [S for S in lens if S in SHORT][:1] + [S for S in lens if S in SHORT][-1:]:
        i = lens.index(S)
        lg, ids, cache = run_alone(setup, S)
        one = (fold[0][:, i:i + 1], [fold[1][i]], fold[2][i:i + 1])
        same_bits(one, (lg[:, None], [ids], cache[None]), [S], f'{rows} rows, inside the batch vs alone')


@pytest.mark.parametrize('rows', [1, 5, 8, 9, 13, 64])
def test_fold_and_separate_kernels_give_the_same_bits_with_e4m3_weights(setup, rows):
    """cr_enable_fp8_decode: the fused small-batch kernels are off, so every batch of 1..64 rows takes the K-sliced partial sums (gemm8) and the fold."""
    eng, nofold = setup['eng'], setup['nofold']
    lens = BATCHES[rows] if rows in BATCHES else (BOUNDARY + [1, 17, 255, 511, 64])[:rows]
    plain = run_batch(eng, lens) if rows in (1, 9) else None
    eng.enable_fp8_decode(True)
    nofold.share_weights_from(eng)
    try:
        fold = run_batch(eng, lens)
        sep = run_batch(nofold, lens)
    finally:
        eng.enable_fp8_decode(False)
        nofold.share_weights_from(eng)
    same_bits(fold, sep, lens, f'{rows} rows, e4m3 weights, fold vs separate kernels')
    if plain is not None:
        assert not torch.equal(plain[0], fold[0])                    # the option was on: other weights, other logits


# ---- part 2: references that share no code with the step ----

def rbf(x):
    return x.to(torch.bfloat16).double()


def kv_rows_f64(sd, cos, sin, tokens, positions, eps=1e-5):
    """Layer 0's new K (after RoPE) and V rows for `tokens` fed at `positions`, in float64 with the reference's bf16 rounding points
    (modeling_internlm2.py:138-143 RMSNorm: bf16 before * weight; :359-371 wqkv and its [groups][4 q | k | v][128] view; :233-247 RoPE): (n, 2, 8, 128).
    With forced tokens the input of layer 0 is the token's embedding row, so these rows are a function of the state dict alone."""
    x = sd['language_model.model.tok_embeddings.weight'][tokens].double()
    h = rbf(x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    h = rbf(sd[L0 + 'attention_norm.weight'].double() * h)
    qkv = rbf(h @ sd[L0 + 'attention.wqkv.weight'].double().T).view(-1, 8, 6, 128)
    k, v = qkv[:, :, 4], qkv[:, :, 5]
    c, s = cos[positions].double()[:, None], sin[positions].double()[:, None]
    rot = torch.cat((-k[..., 64:], k[..., :64]), dim=-1)
    k = rbf(rbf(k * c) + rbf(rot * s))
    return torch.stack((k, v), dim=1)


def kv_rows_oracle(sd, tokens, positions):
    """The same rows as the CPU oracle caches them (oracle/internlm2.py, bf16 on the CPU): its attention layer run on the token over a past of the right length."""
    from oracle import internlm2
    cos_t, sin_t = internlm2.rope_tables(128, seq_len=2048)
    out = []
    with torch.no_grad():
        for tok, pos in zip(tokens.tolist(), positions.tolist()):
            x = sd['language_model.model.tok_embeddings.weight'][tok][None, None]
            past = (torch.zeros(1, 8, pos, 128, dtype=x.dtype), torch.zeros(1, 8, pos, 128, dtype=x.dtype))
            _, (k, v) = internlm2.attention(sd, L0, internlm2.rms_norm(x, sd[L0 + 'attention_norm.weight']), torch.tensor([[pos]]), past, cos_t, sin_t)
            out.append(torch.stack((k[0, :, -1], v[0, :, -1])))
    return torch.stack(out)


def bf16_steps(got, ref):
    """|got - ref| in units of the bf16 spacing at the reference element (8 significand bits: 2^(exponent - 7)), per element"""
    ref = ref.double()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)
    return (got.double() - ref).abs() / ulp


# Worst deviation of the ORACLE's bf16 rows (kv_rows_oracle) from kv_rows_f64 over exactly the (token, position) pairs the two batches below feed (462 pairs x
# 8 x 128 elements, CPU; scripts/decode_step_calibrate.py prints them): K 64 bf16 steps of the element, V 19.  Both are single elements some 2^-7 of the
# typical magnitude, where one step of the element is a small fraction of the fp32 sum's rounding error; 12 (K) and 6 (V) of 393 216 elements are off by more
# than one step, none of the others by more than one.  A second bf16 implementation with another summation order cannot be asked to be closer to exact
# arithmetic than the reference is: the bound is twice the oracle's worst.
ORACLE_K_STEPS = 64.0
ORACLE_V_STEPS = 19.0

ORACLE_ROWS = [254, 510, 17]        # crosses 256, crosses 512, a short row: each checked from inside the batch


def forced_tokens(lens, oracle_ids):
    """(STEPS, rows) ids fed at the decode steps: the oracle's own ids for the rows it checks, seeded random ids for the others"""
    g = torch.Generator().manual_seed(len(lens))
    f = torch.randint(0, 8201, (STEPS, len(lens)), generator=g)
    for S, ids in oracle_ids.items():
        if S in lens:
            f[:, lens.index(S)] = torch.tensor(ids[:STEPS])
    return f


@pytest.fixture(scope='module')
def oracle(setup):
    from oracle import generate
    out = {}
    with torch.no_grad():
        for S in ORACLE_ROWS:
            ids, logits = generate.greedy_generate(setup['sd'], 2, prompt(S), max_new_tokens=STEPS + 1, eos_token_id=-1, repetition_penalty=PENALTY,
                                                   return_logits=True)
            out[S] = (ids[0].tolist(), logits)
    return out


@pytest.mark.parametrize('rows', [13, 64])
def test_rows_inside_the_batch_against_the_oracle_and_float64(setup, oracle, rows):
    """Teacher-forced batch.  Logits and picks of the rows of 254, 510 and 17 cached tokens against the CPU oracle's run of the same prompt alone (check_step:
    |diff| <= 0.12, rel-L2 <= 2.5e-2, a differing pick only as a measured near-tie).  Layer-0 K / V rows of EVERY row and step against kv_rows_f64.

    Tolerance of the K / V rows, measured, not guessed: over the (token, position) pairs of these two batches the oracle's own bf16 rows deviate from
    kv_rows_f64 by at most 64 (K) / 19 (V) bf16 steps of the element (ORACLE_K_STEPS / ORACLE_V_STEPS above, with their source); twice that is allowed:
    128 steps for K, 38 for V.  (Measured on an MI355X: K 1 / V 31 steps in the 13-row batch, K 32 / V 17 in the 64-row one; 3 (K) and 6 (V) of 393 216
    elements off by more than one step.)"""
    from callireader_amd.engine import rope_tables
    eng, sd, lens = setup['eng'], setup['sd'], BATCHES[rows]
    assert all(S in lens for S in ORACLE_ROWS)
    slots, order = slots_and_order(rows)
    forced = forced_tokens(lens, {S: ids for S, (ids, _) in oracle.items()})
    kv = eng.kv_alloc(rows + 1, 1024)
    first = {}
    for i, S in enumerate(lens):
        lg = eng.prefill(kv, i + 1, prompt(S).cuda(), penalty=PENALTY, want_logits=S in ORACLE_ROWS)
        if S in ORACLE_ROWS:
            first[S] = lg.float().cpu()
    steps = []
    for t in range(STEPS):
        lg = eng.decode(kv, [slots[i] for i in order], penalty=PENALTY, force_tokens=forced[t][order], want_logits=True)
        steps.append(lg.float().cpu())
    torch.cuda.synchronize()
    for S in ORACLE_ROWS:
        i = lens.index(S)
        ref_ids, ref_logits = oracle[S]
        picked = kv.generated(slots[i])
        assert len(picked) == STEPS + 1
        div = []
        for t in range(STEPS + 1):
            got = first[S] if t == 0 else steps[t - 1][order.index(i)]
            if check_step(t, got.reshape(-1), ref_logits[t], picked[t], ref_ids, PENALTY):
                div.append(t)
        if div:
            print(f'{rows} rows, row of {S} tokens: picks differed from the oracle at measured near-ties, steps {div}')
    # layer 0's new rows of every row and step
    cos, sin = rope_tables(setup['dims'], 2048)
    tokens = forced.T.reshape(-1)                                                     # row-major: (row, step)
    positions = torch.tensor([S + t for S in lens for t in range(STEPS)])
    want = kv_rows_f64(sd, cos, sin, tokens, positions).view(rows, STEPS, 2, 8, 128)
    got = torch.stack([torch.stack([torch.stack([kv.read(0, slots[i], lens[i] + t, which) for which in (0, 1)]) for t in range(STEPS)])
                       for i in range(rows)]).cpu()
    kv.free()
    assert {255, 256, 257, 511, 512} <= set(positions.tolist())
    dev = bf16_steps(got, want)
    dk, dv = dev[:, :, 0], dev[:, :, 1]
    print(f'{rows} rows: layer-0 rows vs float64, worst deviation in bf16 steps of the element: K {float(dk.max()):.3f}, V {float(dv.max()):.3f} '
          f'(oracle {ORACLE_K_STEPS} / {ORACLE_V_STEPS}); elements off by more than one step: K {int((dk > 1).sum())}, V {int((dv > 1).sum())} of {dk.numel()}')
    for name, d, bound in (('V', dv, 2 * ORACLE_V_STEPS), ('K', dk, 2 * ORACLE_K_STEPS)):
        i, t = [int(x) for x in (d.amax(dim=(2, 3)) == d.max()).nonzero()[0]]
        assert float(d.max()) <= bound, (name, f'row of {lens[i]} tokens', f'position {lens[i] + t}', float(d.max()), bound)


# ---- part 3: more ids than the old 4096-id buffer ----

LONG_STEPS = 4200


@pytest.fixture(scope='module')
def long_engine(setup):
    eng = setup['eng'].__class__(setup['dims'], max_pos=4352)
    eng.load_state_dict(setup['sd'])
    eng.load_rope()
    eng.finalize()
    yield eng
    eng.close()


@pytest.mark.parametrize('rows', [1, 9])
def test_more_than_4096_generated_ids(long_engine, rows):
    """The id buffer is sized by the cache (one id per cached token at most), not 4096: past it the step must go on feeding the id it has just picked.
    An 8-token prompt, LONG_STEPS free-running greedy steps (no EOS, penalty 1.0), then the same steps teacher-forced with the first run's ids on a second
    cache (force_tokens never reads the id buffer).  Same kernels, same inputs: the logits of every step are the same bits.  1 row: the fused small-batch
    kernels; 9 rows: the K-sliced step.  (With the 4096-id buffer the free run fed id number 4095 again and again: the runs differ from decode step 4097.)"""
    eng = long_engine
    seqs = list(range(rows))
    embs = [(torch.randn(1, 8, 4096, generator=torch.Generator().manual_seed(50 + i)) * 0.02).to(torch.bfloat16).cuda() for i in range(rows)]
    free, forced = eng.kv_alloc(rows, 8 + LONG_STEPS), eng.kv_alloc(rows, 8 + LONG_STEPS)
    free.set_logprobs(0, 2)
    first = torch.stack([eng.prefill(free, i, embs[i], want_logits=True) for i in seqs])
    for i in seqs:
        eng.prefill(forced, i, embs[i])
    keep = [eng.decode(free, seqs, want_logits=True) for _ in range(LONG_STEPS)]
    torch.cuda.synchronize()
    # penalty 1.0: the id a step appends is the first maximum of its logits, so the ids to force are known without reading the id buffer
    feed = torch.stack([first.argmax(-1)] + [lg.argmax(-1) for lg in keep])           # (steps + 1, rows)
    first_diff = None
    for t in range(LONG_STEPS):
        lg = eng.decode(forced, seqs, force_tokens=feed[t], want_logits=True)
        if first_diff is None and not torch.equal(lg, keep[t]):
            first_diff = t
    assert first_diff is None, f'free-running and teacher-forced logits differ from decode step {first_diff + 1} on (the first to feed generated id number {first_diff})'
    ids = [free.generated(i) for i in seqs]
    for i in seqs:
        assert len(ids[i]) == LONG_STEPS + 1 and free.length(i) == 8 + LONG_STEPS, (i, len(ids[i]), free.length(i))
    assert ids == feed.T.tolist()
    lp, top_ids, _ = free.logprobs(0)
    assert len(lp) == LONG_STEPS + 1 and top_ids[:, 0].tolist() == ids[0]
    assert [forced.length(i) for i in seqs] == [8 + LONG_STEPS] * rows
    free.free(); forced.free()


def test_the_repetition_penalty_sees_a_history_of_more_than_4096_ids(long_engine):
    """The pick's penalty gathers up to 4096 ids in registers; a longer history takes the path that reads an untouched copy of the row (pick.hpp).  Past
    4096 ids every pick must still be the first maximum of the penalised row, computed here from the step's raw logits and the ids so far."""
    eng = long_engine
    emb = (torch.randn(1, 8, 4096, generator=torch.Generator().manual_seed(60)) * 0.02).to(torch.bfloat16).cuda()
    kv = eng.kv_alloc(1, 8 + LONG_STEPS)
    eng.prefill(kv, 0, emb, penalty=1.3)
    keep = {}
    for t in range(LONG_STEPS):
        lg = eng.decode(kv, [0], penalty=1.3, want_logits=t >= 4000)
        if lg is not None:
            keep[t] = lg[0]
    torch.cuda.synchronize()
    ids = kv.generated(0)
    assert len(ids) == LONG_STEPS + 1
    pen = torch.tensor(1.3, dtype=torch.float32)
    for t, lg in keep.items():
        lg = lg.cpu()                                                                 # on the CPU: a true fp32 division, as the kernel's
        hist = torch.tensor(sorted(set(ids[:t + 1])))
        s = lg[hist]
        lg[hist] = torch.where(s < 0, s * pen, s / pen)
        assert int(lg.argmax()) == ids[t + 1] or (float(lg[ids[t + 1]]) == float(lg.max()) and ids[t + 1] <= int(lg.argmax())), (t, ids[t + 1], int(lg.argmax()))
    kv.free()

"""cr_op_span_mass on a real MI355X: the span-mass kernels of cr_llm_ground_batch alone, one layer (csrc/ground.hip).

Data: q and k entries are multiples of 1/4 in [-3, 3], so every product is a multiple of 1/16 below 9 and every 128-term dot product (< 1152, 15 bits) is
exact in fp32 whatever the summation order: the two bf16 roundings of a score are then deterministic, and the reference's scores are the kernel's, bit for
bit.  Scores have a standard deviation of about 3 (they span about +-8): the softmax is peaked.

Reference: the score arithmetic of the prefill attention's DIV path in torch on the CPU (fp32 dot, bf16, * fp32(1 / s_div), bf16), then softmax and span
sums in float64.  Bound: |mass - ref| <= 2 (Sk + 32) 2^-24 ref + 1e-9 with Sk = the row's own key count -- the worst case of fp32 sums of Sk non-negative
terms with 32 ulp allowed per term for the exponent's multiply and v_exp_f32, applied to numerator and denominator."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, NKV, HD, T, SLOTS = 32, 8, 128, 512, 3
S_DIV = 11.313708498984761
# (cached, rows, slot): the queries of the second cross key 256 and a 64-key tile edge; the third crosses a 32-row wave and a 128-row block
SEGS = [(70, 37, 1), (250, 9, 2), (3, 130, 0)]
NOT_GROUNDED = {0: (0, 5)}      # rows 0 and 5 of the first segment


# one span from key 0, fourteen 3-wide runs, one 1-wide, one across the 64-key tile edge (62..66), one empty; then per segment spans inside the rows' own
# region (zero for the earlier queries): (80, 90) behind 70 cached keys, (254, 258) across key 256 behind 250, (126, 131) across a 128-key edge
BASE = [(0, 2)] + [(5 + 3 * i, 8 + 3 * i) for i in range(14)] + [(50, 51), (62, 66), (68, 68)]
SPANS = [BASE + [(80, 90)], BASE + [(100, 130), (254, 258)], BASE + [(80, 90), (126, 131)]]


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(20)
    rows = sum(s[1] for s in SEGS)
    q = (torch.randint(-12, 13, (rows, H, HD), generator=g).float() / 4).to(torch.bfloat16)
    k = (torch.randint(-12, 13, (SLOTS, NKV, T, HD), generator=g).float() / 4).to(torch.bfloat16)
    segs, r0 = [], 0
    for cached, S, slot in SEGS:
        segs.append((r0, S, cached, slot))
        r0 += S
    grounded = [True] * rows
    for i, rr in NOT_GROUNDED.items():
        for r in rr:
            grounded[segs[i][0] + r] = False
    return dict(q=q, k=k, qd=q.cuda(), kd=k.cuda(), segs=segs, grounded=grounded, probs={})


def probs_of(data, i):
    """[H, S, Sk] float64 softmax of segment i, computed once"""
    if i not in data['probs']:
        r0, S, pos0, slot = data['segs'][i]
        Sk = pos0 + S
        qs = data['q'][r0:r0 + S].float().permute(1, 0, 2)                                  # [H, S, d]
        ks = data['k'][slot, :, :Sk].float().repeat_interleave(H // NKV, dim=0)             # [H, Sk, d]
        s = torch.bmm(qs, ks.transpose(1, 2))                                               # exact in fp32
        inv = torch.tensor(np.float32(1.0) / np.float32(S_DIV))
        s = (s.to(torch.bfloat16).float() * inv).to(torch.bfloat16).double()
        mask = torch.arange(Sk)[None, :] > (pos0 + torch.arange(S))[:, None]
        data['probs'][i] = torch.softmax(s.masked_fill(mask[None], float('-inf')), dim=-1)
    return data['probs'][i]


def reference(data, i, spans, rows=None):
    """[rows, len(spans)] float64 head-mean span mass of segment i's grounded rows"""
    r0, S, pos0, _ = data['segs'][i]
    P = probs_of(data, i)
    keep = [r for r in range(S) if data['grounded'][r0 + r]] if rows is None else rows
    out = torch.zeros(len(keep), len(spans), dtype=torch.float64)
    for b, (s, e) in enumerate(spans):
        if e > s:
            out[:, b] = P[:, keep, s:e].sum(-1).mean(0)
    return out, torch.tensor([pos0 + r + 1 for r in keep], dtype=torch.float64)


def check(got, ref, keys, what):
    bound = 2 * (keys[:, None] + 32) * 2.0 ** -24 * ref + 1e-9
    err = (got.double() - ref).abs()
    rel = float((err / ref.clamp_min(1e-30))[ref > 1e-6].max()) if bool((ref > 1e-6).any()) else 0.0
    print(f'{what}: max |mass - ref| {float(err.max()):.3e}, max relative (ref > 1e-6) {rel:.3e}, mass up to {float(ref.max()):.3f}')
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    return rel


def test_mass_against_the_reference(data):
    from callireader_amd.engine import op_span_mass
    mass = op_span_mass(data['qd'], data['kd'], data['segs'], SPANS, grounded=data['grounded'], s_div=S_DIV).cpu()
    ld = max(len(s) for s in SPANS)
    assert mass.shape == (sum(data['grounded']), ld)
    r = 0
    for i in range(len(SEGS)):
        ref, keys = reference(data, i, SPANS[i])
        n = ref.shape[0]
        check(mass[r:r + n, :len(SPANS[i])], ref, keys, f'segment {i}')
        assert bool((mass[r:r + n, len(SPANS[i]):] == 0).all())                  # columns past a sequence's own span count are written 0
        r += n
    # a span entirely behind a row gets exactly 0: rows at positions 70..79 of the first segment and its span (80, 90)
    first = mass[:35, len(SPANS[0]) - 1]
    assert SPANS[0][-1] == (80, 90) and bool((first[:8] == 0).all()) and bool((first[8:] > 0).all())
    assert bool((mass[:35, SPANS[0].index((68, 68))] == 0).all())                # the empty span


def test_spans_that_partition_the_keys_sum_to_one(data):
    from callireader_amd.engine import op_span_mass
    parts = [[(s, min(s + 7, c + S)) for s in range(0, c + S, 7)] for c, S, _ in SEGS]
    mass = op_span_mass(data['qd'], data['kd'], data['segs'], parts, grounded=data['grounded'], s_div=S_DIV).cpu()
    r = 0
    for i in range(len(SEGS)):
        ref, keys = reference(data, i, parts[i])
        n = ref.shape[0]
        check(mass[r:r + n, :len(parts[i])], ref, keys, f'partition of segment {i}')
        tot = mass[r:r + n, :len(parts[i])].double().sum(-1)
        worst = float((tot - 1).abs().max())
        print(f'partition of segment {i}: max |sum - 1| {worst:.3e}')
        assert bool(((tot - 1).abs() <= 2 * (keys + 32) * 2.0 ** -24 + len(parts[i]) * 1e-9).all())
        r += n


def test_a_segment_alone_and_among_the_three(data):
    from callireader_amd.engine import op_span_mass
    three = op_span_mass(data['qd'], data['kd'], data['segs'], SPANS, grounded=data['grounded'], s_div=S_DIV)
    r = 0
    for i in range(len(SEGS)):
        alone = op_span_mass(data['qd'], data['kd'], [data['segs'][i]], [SPANS[i]], grounded=data['grounded'], s_div=S_DIV)
        n = alone.shape[0]
        assert torch.equal(alone, three[r:r + n, :len(SPANS[i])]), i
        r += n
    # one row of the 130-row segment by itself (another workgroup shape, another lane): the same bits
    r0, S, pos0, slot = data['segs'][2]
    one = op_span_mass(data['qd'], data['kd'], [(r0 + 77, 1, pos0 + 77, slot)], [BASE], s_div=S_DIV)      # (a 1-row segment ends at key 80: the spans before it)
    assert one.shape == (1, len(BASE)) and torch.equal(one[0], three[35 + 9 + 77, :len(BASE)])
    # a slot with no span at all: its rows are 0, the others keep their bits
    none = op_span_mass(data['qd'], data['kd'], data['segs'], [SPANS[0], [], SPANS[2]], grounded=data['grounded'], s_div=S_DIV)
    assert bool((none[35:44] == 0).all()) and torch.equal(none[:35], three[:35, :none.shape[1]]) and torch.equal(none[44:], three[44:, :none.shape[1]])


def test_refusals(data):
    from callireader_amd.engine import op_span_mass
    from callireader_amd._binding import CalliReaderError
    seg = data['segs'][0]
    for bad in ([(5, 8), (7, 9)], [(8, 5)], [(10, 12), (2, 4)], [(100, 108)], [(-1, 3)]):      # overlapping, reversed, unsorted, outside [0, 107)
        with pytest.raises(CalliReaderError, match='error -1:'):
            op_span_mass(data['qd'], data['kd'], [seg], [bad], s_div=S_DIV)
    with pytest.raises(CalliReaderError, match='error -1:'):
        op_span_mass(data['qd'], data['kd'], [(0, 37, 500, 1)], [[(0, 1)]], s_div=S_DIV)      # rows past the cache
    with pytest.raises(CalliReaderError, match='error -1:'):
        op_span_mass(data['qd'], data['kd'], [seg], [[(0, 1), (1, 2)]], s_div=S_DIV, mass_ld=1)
    with pytest.raises(CalliReaderError, match='error -1:'):
        op_span_mass(data['qd'], data['kd'], [seg], [[(0, 1)]], grounded=[False] * data['q'].shape[0], s_div=S_DIV)

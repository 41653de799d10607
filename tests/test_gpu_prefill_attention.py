"""The prefill attention's segment launch on a real MI355X, through cr_op_attention_segments: flash_attn_kernel<128, causal, divisor> driven with
AttnParams::seg exactly as cr_llm_prefill_batch drives it (both fill their launch in attention.hpp's segment_attn_params).

Reference: attn_ref (tests/attn_ref.py), the reference model's rounding points in plain PyTorch, evaluated per KV head on the device over each
segment's prefix + page with its first position.  Bound for ordinary random data: test_attention_llm_causal_gqa's, rtol 1.6e-2 (two bf16 steps
of the output) + atol 1.5e-2.

Peaked scores (a sink, a late dominant key, a key that grows the row maximum by 6..8, rows whose scores are all near -40): the bound is measured,
not guessed.  scripts/prefill_attention_calibrate.py evaluates, on the CPU and on these very inputs, how far attn_ref itself lies from a float64
softmax attention without any rounding, as the smallest atol at which attn_ref would pass `assert_close(rtol = 1.6e-2)` against float64
(PEAKED_FLOOR below).  A second bf16 implementation with another summation order cannot be asked to be closer to exact arithmetic than the
reference is, so twice the floor is allowed (the margin test_gpu_decode_step.py set for its K / V rows) -- and where 1.5e-2 already exceeds
twice the floor, 1.5e-2 stays.  Measured (floor -> allowed; the kernel's worst excess over rtol * |ref| on an MI355X):

    case       pos0 = 0                               pos0 = 1000
    random     9.3e-3 -> 1.5e-2 (kept)   2.8e-3       2.5e-3 -> 1.5e-2 (kept)   5.1e-4
    sink       0      -> 1.5e-2 (kept)   < 0          0      -> 1.5e-2 (kept)   < 0
    late       9.3e-3 -> 1.86e-2         2.8e-3       2.5e-3 -> 1.5e-2 (kept)   5.1e-4
    grow       9.3e-3 -> 1.86e-2         2.8e-3       5.1e-3 -> 1.5e-2 (kept)   5.1e-4
    negative   1.30e-1 -> 2.60e-1        2.8e-3       1.81e-2 -> 3.62e-2        1.1e-3

(`random` is ordinary data and keeps 1.5e-2 whatever its floor.  The pos0 = 0 floors come from the page's first rows, which attend over a handful of keys
and return outputs up to |2.6|; `negative` is the reference's coarsest case: near -40 a bf16 score moves in steps of 0.25, so a weight differs from
exact arithmetic by up to 13 % -- the kernel rounds at the same points and stays within 3e-3 of the reference all the same.)
"""
import math

import pytest
import torch

from attn_ref import rb, segments_ref

pytestmark = pytest.mark.gpu

RTOL = 1.6e-2                 # test_gpu_ops.py's: two bf16 steps of the output
ATOL = 1.5e-2                 # test_attention_llm_causal_gqa's
SDIV = math.sqrt(128)
HD = 128
SENTINEL = -1232.0            # a bf16 value no attention over N(0, 1) values produces

# the page lengths of test_final_layer_on_the_last_rows_only_gives_the_same_bits: both sides of the kernel's 32-row waves, 64-key tiles and 128-row blocks
LENS = [300, 77, 130, 1500, 33, 32, 64, 65, 1, 129, 128, 97]
SLOTS = [7, 2, 11, 0, 14, 5, 9, 1, 12, 3, 10, 6]                        # arbitrary and non-monotonic, of 16
POS0 = [0, 1, 63, 1000, 64, 70, 0, 127, 128, 200, 0, 1000]              # first positions: three pages start empty, the 1500-row page at 1000
N_SLOTS, MAX_TOKENS = 16, 2560


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def E():
    from callireader_amd import engine
    return engine


def segments(lens, slots, pos0s, gap=0):
    """[(first row, rows, first position, slot)] with the row offsets as the running sum (+ `gap` unused rows after every page)."""
    segs, row = [], 0
    for S, slot, p in zip(lens, slots, pos0s):
        segs.append((row, S, p, slot))
        row += S + gap
    return segs


def random_launch(H, n_kv, segs, n_slots, max_tokens, seed, rows=None, poison=False):
    """q (rows, H, 128), kc / vc (n_slots, n_kv, max_tokens, 128) bf16 ~ N(0, 1).  poison: everything a segment launch must not read is NaN -- cache
    rows at or past a segment's pos0 + S, slots no segment names, q rows of no segment."""
    g = torch.Generator().manual_seed(seed)
    rows = rows or max(r + S for r, S, _, _ in segs)
    q = torch.randn(rows, H, HD, generator=g).bfloat16()
    kc = torch.randn(n_slots, n_kv, max_tokens, HD, generator=g).bfloat16()
    vc = torch.randn(n_slots, n_kv, max_tokens, HD, generator=g).bfloat16()
    if poison:
        live_kv = torch.zeros(n_slots, max_tokens, dtype=torch.bool)
        live_q = torch.zeros(rows, dtype=torch.bool)
        for row0, S, pos0, slot in segs:
            live_kv[slot, :pos0 + S] = True
            live_q[row0:row0 + S] = True
        dead = ~live_kv[:, None, :, None].expand_as(kc)
        kc[dead] = float('nan')
        vc[dead] = float('nan')
        q[~live_q] = float('nan')
    return q, kc, vc


def launch(E, q, kc, vc, segs, Sq=None):
    o = torch.full_like(q, SENTINEL)
    E.op_attention_segments(q, kc, vc, o, segs, s_div=SDIV, Sq=Sq)
    torch.cuda.synchronize()
    return o


def check(o, q, kc, vc, segs, atol=ATOL, label=''):
    """Every segment's rows finite and within rtol * |ref| + atol of attn_ref; every other row of o untouched.  Returns the worst excess
    |o - ref| - rtol * |ref| (what atol has to cover), printed per launch before anything is asserted."""
    ref = segments_ref(q, kc, vc, segs, SDIV)
    inside = torch.zeros(q.shape[0], dtype=torch.bool, device=o.device)
    worst, finite = -1.0, True
    for i, (row0, S, _, _) in enumerate(segs):
        got = o[row0:row0 + S].float()
        assert torch.isfinite(ref[i]).all(), ('the reference itself is not finite', i)
        finite = finite and bool(torch.isfinite(got).all())
        worst = max(worst, float(torch.nan_to_num((got - ref[i]).abs() - RTOL * ref[i].abs(), nan=float('inf')).max()))
        inside[row0:row0 + S] = True
    print(f'  {label}: {len(segs)} segments, worst excess over rtol {worst:.3e} (allowed {atol:.3e}), finite {finite}')
    for i, (row0, S, pos0, slot) in enumerate(segs):
        got = o[row0:row0 + S].float()
        assert torch.isfinite(got).all(), f'segment {i} (rows {row0}+{S}, pos0 {pos0}, slot {slot}): output not finite'
        torch.testing.assert_close(got, ref[i], rtol=RTOL, atol=atol, msg=lambda m, i=i, s=(row0, S, pos0, slot): f'segment {i} {s}: {m}')
    outside = o[~inside]
    assert torch.equal(outside, torch.full_like(outside, SENTINEL)), 'rows of o that belong to no segment were written'
    return worst


def to_dev(*ts):
    return [t.to(dev()) for t in ts]


def test_production_shape(E):
    """One page as the bench prefills it: 3 164 rows, 32 query heads over 8 KV heads -- 25 query blocks, up to 50 key tiles; all rows, all heads."""
    S = 3164
    segs = [(0, S, 0, 0)]
    q, kc, vc = to_dev(*random_launch(32, 8, segs, 1, S, seed=41))
    check(launch(E, q, kc, vc, segs), q, kc, vc, segs, label='production shape')


def test_ragged_pages_in_one_launch(E):
    """Twelve pages of 1..1500 rows in one launch of Sq = 1500, slots in arbitrary order: the short pages' surplus query blocks return early."""
    segs = segments(LENS, SLOTS, [0] * len(LENS))
    q, kc, vc = to_dev(*random_launch(32, 8, segs, N_SLOTS, MAX_TOKENS, seed=42))
    check(launch(E, q, kc, vc, segs), q, kc, vc, segs, label='ragged pages')


def test_nonzero_first_positions(E):
    """The same pages continuing sequences that already hold 1, 63, 64, 70, 127, 128, 200 and 1000 tokens (three start empty): the cache holds the
    prefix keys / values, the reference attends over prefix + page with q_pos0.  Pins kmax, need_mask, Sk = q_pos0 + Sq and the ragged tile's clamp."""
    segs = segments(LENS, SLOTS, POS0)
    assert {p for _, _, p, _ in segs} == {0, 1, 63, 64, 70, 127, 128, 200, 1000}
    q, kc, vc = to_dev(*random_launch(32, 8, segs, N_SLOTS, MAX_TOKENS, seed=43))
    check(launch(E, q, kc, vc, segs), q, kc, vc, segs, label='non-zero first positions')


def test_nothing_outside_a_segments_range_is_read_or_written(E):
    """NaN in every cache row at or past a segment's pos0 + S, in every slot no segment names and in every q row of no segment (five unused rows after
    every page, 64 at the end); o starts as a sentinel.  The kernel clamps a ragged tile's loads to key Sk - 1 and a ragged block's to row Sq - 1, so
    nothing of that is data it may read: outputs finite and within the bound, rows of no segment keep the sentinel's bits.  (The reference reads
    positions < pos0 + S only and is asserted finite in check(); tests/test_attn_ref_cpu.py confirms that on the CPU with these inputs.)"""
    segs = segments(LENS, SLOTS, POS0, gap=5)
    rows = segs[-1][0] + segs[-1][1] + 64
    q, kc, vc = random_launch(32, 8, segs, N_SLOTS, MAX_TOKENS, seed=44, rows=rows, poison=True)
    assert torch.isnan(kc[4]).all() and torch.isnan(kc[SLOTS[8], :, POS0[8] + 1:]).all() and not torch.isnan(kc[SLOTS[8], :, :POS0[8] + 1]).any()
    q, kc, vc = to_dev(q, kc, vc)
    check(launch(E, q, kc, vc, segs), q, kc, vc, segs, label='poisoned surroundings')


SHORT = [150 if S == 1500 else S for S in LENS]       # longest 300 rows: three query blocks, an odd count


@pytest.mark.parametrize('H,n_kv,lens,total', [
    (32, 8, LENS, 4608), (32, 8, LENS + [200], 4992),                     # 12 blocks x 32 heads x 12 / 13 pages: multiples of 8 whatever the page count
    (4, 1, SHORT, 144), (4, 1, SHORT + [200], 156), (1, 1, SHORT + [200], 39)])      # 3 blocks: 144 = 8 x 18; 156 = 8 x 19 + 4; 39 = 8 x 4 + 7
def test_workgroup_id_remap(E, H, n_kv, lens, total):
    """The kernel remaps its linear workgroup id so that each XCD gets a contiguous run of (page, head, block); with total % 8 != 0 the first
    total % 8 XCDs get one more.  A wrong remap computes some (page, head, block) twice and another never: the sentinel survives in o."""
    n = len(lens)
    segs = segments(lens, (SLOTS + [15])[:n], (POS0 + [5])[:n])
    Sq = max(lens)
    got_total = (Sq + 127) // 128 * H * n
    assert got_total == total and (total & 7 != 0) == (total in (156, 39)), (got_total, total)
    q, kc, vc = to_dev(*random_launch(H, n_kv, segs, N_SLOTS, MAX_TOKENS, seed=45, rows=sum(LENS) + 200))      # the same data for every page count of a head count
    check(launch(E, q, kc, vc, segs), q, kc, vc, segs, label=f'remap H={H} n={n} total={total}')


def test_last_rows_form_gives_the_full_launchs_bits(E):
    """The final layer's launch: per page the segment {row0 + w0, S - w0, pos0 + w0, slot}, w0 = (S - 1) / 32 * 32, Sq = 32 -- the rows that share
    a wave with the page's last row.  That last row must be the full launch's, bit for bit (what prefill_layers relies on); pages with non-zero
    first positions, S on both sides of 32, 64 and 128."""
    segs = segments(LENS, SLOTS, POS0)
    assert {32, 33, 64, 65, 128, 129, 1} <= set(LENS)
    q, kc, vc = to_dev(*random_launch(32, 8, segs, N_SLOTS, MAX_TOKENS, seed=46))
    full = launch(E, q, kc, vc, segs)
    last = [(row0 + (S - 1) // 32 * 32, S - (S - 1) // 32 * 32, pos0 + (S - 1) // 32 * 32, slot) for row0, S, pos0, slot in segs]
    assert all(1 <= s[1] <= 32 for s in last)
    part = launch(E, q, kc, vc, last, Sq=32)
    check(full, q, kc, vc, segs, label='full launch')
    for i, (row0, S, _, _) in enumerate(segs):
        r = row0 + S - 1
        assert torch.equal(part[r], full[r]), (i, S, float((part[r].float() - full[r].float()).abs().max()))
        assert not torch.equal(full[r], torch.full_like(full[r], SENTINEL))
    written = torch.zeros(q.shape[0], dtype=torch.bool, device=dev())
    for row0, S, _, _ in last:
        written[row0:row0 + S] = True
    assert torch.equal(part[~written], torch.full_like(part[~written], SENTINEL))


# ---- peaked scores ----
PEAK_T, PEAK_H, PEAK_KV, PEAK_KEY = 3164, 8, 2, 2000
PEAKED = ['random', 'sink', 'late', 'grow', 'negative']
PEAK_POS0 = [0, 1000]
# scripts/prefill_attention_calibrate.py (CPU): the smallest atol at which attn_ref passes assert_close(rtol = RTOL) against float64 softmax attention
PEAKED_FLOOR = {
    ('random', 0): 9.285e-03,         # max |ref - f64| 1.795e-02 (the first rows: few keys, |o| up to 2.6)
    ('random', 1000): 2.528e-03,      # max |ref - f64| 4.978e-03
    ('sink', 0): 0.0,                 # max |ref - f64| 3.4e-12: every row is key 0's value in both
    ('sink', 1000): 0.0,
    ('late', 0): 9.285e-03,           # max |ref - f64| 1.795e-02
    ('late', 1000): 2.528e-03,        # max |ref - f64| 4.978e-03
    ('grow', 0): 9.285e-03,           # max |ref - f64| 2.668e-02
    ('grow', 1000): 5.061e-03,        # max |ref - f64| 2.777e-02
    ('negative', 0): 1.300e-01,       # max |ref - f64| 1.386e-01: near -40 a bf16 score moves in steps of 0.25, a weight by up to 13 %
    ('negative', 1000): 1.809e-02,    # max |ref - f64| 1.937e-02
}


def peaked_atol(name, pos0):
    if name == 'random':
        return ATOL               # ordinary random data keeps test_attention_llm_causal_gqa's bound whatever its floor: the case is here for comparison
    return max(ATOL, 2.0 * PEAKED_FLOOR[(name, pos0)])


def peaked_case(name, pos0):
    """One page of PEAK_T - pos0 rows continuing pos0 cached tokens of slot 1 (CPU tensors); q / k / v ~ N(0, 1) except that dimensions 0..3 of q and k
    are zero and carry the planted scores (query value x key value / sqrt(128), on top of the random part where the key keeps it):
      sink      key 0 scores ~ +40 for every query of every head;
      late      key 2000 scores ~ +20 for the queries at positions >= 2000 whose row % 32 is 3, 17 or 20 and ~ +113 where it is 9 -- far more than 8 above
                everything before it, for a few lanes of every wave (the rescale vote is wave-wide: the other lanes rescale with them);
      grow      key 2000 scores the row's reference point (its maximum over the first key tile) + 6.5..7.5 for ALL 32 rows of every second wave at
                positions >= 2000: no lane votes for a rescale, the deferred form carries P ~ e^7;
      negative  every score of the rows whose row % 32 is 5, 6 or 30 is shifted by ~ -40.
    Returns q (S, H, 128), kc, vc (2, KV, PEAK_T, 128) bf16 and the one segment."""
    g = torch.Generator().manual_seed(47)
    S, H, n_kv, grp = PEAK_T - pos0, PEAK_H, PEAK_KV, PEAK_H // PEAK_KV
    q = torch.randn(PEAK_T, H, HD, generator=g)[pos0:].bfloat16()                     # the same rows at the same positions for both first positions
    kc = torch.randn(2, n_kv, PEAK_T, HD, generator=g).bfloat16()
    vc = torch.randn(2, n_kv, PEAK_T, HD, generator=g).bfloat16()
    q[:, :, :4] = 0
    kc[:, :, :, :4] = 0
    r = torch.arange(S)
    late_rows = r + pos0 >= PEAK_KEY
    if name == 'sink':
        kc[1, :, 0, 0] = 16.0
        q[:, :, 0] = 28.25                                                           # 452 / sqrt(128) = 39.95
    elif name == 'late':
        kc[1, :, PEAK_KEY, 1] = 16.0
        q[late_rows & ((r % 32 == 3) | (r % 32 == 17) | (r % 32 == 20)), :, 1] = 14.125      # 226 / sqrt(128) = 19.98
        q[late_rows & (r % 32 == 9), :, 1] = 80.0                                            # 1280 / sqrt(128) = 113.1
    elif name == 'grow':
        kc[1, :, PEAK_KEY] = 0
        kc[1, :, PEAK_KEY, 2] = 16.0
        rows = late_rows & ((r // 32) % 2 == 0)
        qf = q[rows].float()                                                         # (n, H, 128)
        k0 = kc[1, :, :64].float().repeat_interleave(grp, 0)                         # (H, 64, 128): the first key tile
        m_first = rb(rb(torch.einsum('nhd,hkd->nhk', qf, k0)) / SDIV).amax(-1)       # the kernel's reference point after tile 0
        q[rows, :, 2] = ((m_first + 7.0) * SDIV / 16.0).bfloat16()
        grown = rb(rb(q[rows, :, 2].float() * 16.0) / SDIV) - m_first
        assert float(grown.min()) > 6.0 and float(grown.max()) < 8.0, (float(grown.min()), float(grown.max()))
    elif name == 'negative':
        kc[1, :, :, 3] = 16.0
        q[(r % 32 == 5) | (r % 32 == 6) | (r % 32 == 30), :, 3] = -28.25
    else:
        assert name == 'random'
    return q, kc, vc, [(0, S, pos0, 1)]


@pytest.mark.parametrize('pos0', PEAK_POS0)
@pytest.mark.parametrize('name', PEAKED)
def test_peaked_scores(E, name, pos0):
    """See the module docstring for the bound and peaked_case for the inputs.  Outputs finite and within rtol * |ref| + max(1.5e-2, 2 x floor)."""
    q, kc, vc, segs = peaked_case(name, pos0)
    q, kc, vc = to_dev(q, kc, vc)
    check(launch(E, q, kc, vc, segs), q, kc, vc, segs, atol=peaked_atol(name, pos0), label=f'peaked {name} pos0={pos0}')

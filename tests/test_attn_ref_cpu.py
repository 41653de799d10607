"""CPU checks of the shared attention reference (tests/attn_ref.py) and of the inputs test_gpu_prefill_attention.py builds: what the GPU tests rely on
is confirmed here without a GPU."""
import torch

import test_gpu_prefill_attention as T
from attn_ref import attn_f64, attn_ref, segments_ref


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

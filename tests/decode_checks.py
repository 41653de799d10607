"""The rule by which a HIP logits row and its greedy pick are held against the CPU oracle's, shared by test_gpu_llm.py (check_stream: one sequence
alone) and test_gpu_decode_step.py (rows inside a 9..64-row batch).  The bounds are test_gpu_llm.py's calibrated ones (its docstring): the bf16
oracle's own distance from an fp32 evaluation of the same network."""
ATOL = 0.12
RTOL_L2 = 2.5e-2


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def check_step(t, got, ref, picked, ref_ids, penalty=1.0):
    """Step t of a teacher-forced walk along the oracle's ids: got / ref = the raw fp32 logits rows (CPU), picked = the HIP pick.  Returns True when
    the pick differed (acceptable only as a measured near-tie)."""
    assert rel_l2(got, ref) <= RTOL_L2, (t, rel_l2(got, ref))
    assert float((got - ref).abs().max()) <= ATOL, (t, float((got - ref).abs().max()))
    if picked == ref_ids[t]:
        return False
    # only acceptable as a MEASURED near-tie of the (penalised) scores: the oracle's gap between its pick and ours must be
    # covered by the logit differences measured at exactly those two ids (the HIP scores straddle), and stay inside the
    # calibrated tolerance; nothing is excused by a row-wide bound and there is no allowance per stream
    from oracle.generate import near_tie_straddles
    ok, gap, d_ref, d_hip = near_tie_straddles(ref, got, ref_ids[t], picked, ref_ids[:t], penalty, ATOL)
    print(f'  step {t}: pick differs: oracle gap {gap:.4f}, measured d(ref id) {d_ref:+.4f}, d(hip id) {d_hip:+.4f}')
    assert ok, (t, picked, ref_ids[t], gap, d_ref, d_hip)
    return True

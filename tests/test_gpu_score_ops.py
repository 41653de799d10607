"""The score kernels of cr_llm_score_batch alone (csrc/score.hip through cr_op_score_rows): the repetition penalty applied in registers from a
first-occurrence table, then csrc/logprobs.hip's chunk reduction and chunk-order merge.

Three checks per case.  (1) Bit-equality with cr_op_logprobs on a copy of the rows that the HOST penalised (the same fp32 multiply / divide, IEEE on both
sides): the two kernel pairs share their placement and summation order.  (2) float64 log_softmax of the penalised row within TOL = 1e-5 absolute, the bound
tests/test_gpu_logprobs.py derives for |z| <= 32 (the data stays inside it; a penalty of 1.5 only shrinks or, for negative scores, grows |z| to at most
1.5 * 20).  (3) A row's result does not depend on the launch size or on the row's position.

Histories: row r belongs to history row_seq[r] with ordinal hist_index[r]; it is penalised at the targets of the rows of its history with a smaller ordinal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
VOCABS = [8201, 92553]            # both ragged: the last chunk is partial and row starts are not 16-byte aligned


def make_case(V, n, seed):
    """n raw rows, their targets and histories.  Two interleaved histories (rows r % 3 == 2 belong to the second); targets drawn from a pool of 6 ids so that
    ids repeat inside a history and a target is usually in its own history; the first pool id is negative in every row, the second positive, so a target is
    penalised on both sides; rows with -inf entries; one NaN row (n >= 13)."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(n, V, generator=g) * 3.0).clamp(-20, 20)
    pool = torch.randperm(V, generator=g)[:6].tolist()
    z[:, pool[0]] = -torch.rand(n, generator=g) * 5 - 0.5
    z[:, pool[1]] = torch.rand(n, generator=g) * 5 + 0.5
    z[:, V - 1] = 4.0                                        # the ragged tail's last id is a contender
    targets, row_seq, hist_index, count = [], [], [], [0, 0]
    fixed = {0: pool[0], 1: pool[1], 3: pool[0], 4: pool[1]}      # rows 3 and 4 (first history, like rows 0 and 1) score an id their history holds
    for r in range(n):
        h = 1 if r % 3 == 2 else 0
        targets.append(fixed[r] if r in fixed else pool[int(torch.randint(0, 6, (1,), generator=g))])
        row_seq.append(h)
        hist_index.append(count[h])
        count[h] += 1
    for r in range(1, n, 4):                                 # rows with -inf entries (never at a pool id: the targets stay finite)
        idx = torch.randperm(V, generator=g)[:V // 3]
        keep = z[r, pool].clone()
        z[r, idx] = -float('inf')
        z[r, pool] = keep
    nan_row = 7 if n >= 13 else None
    if nan_row is not None:
        z[nan_row, (pool[2] + 1) % V] = float('nan')
    return z, targets, row_seq, hist_index, nan_row


def host_penalised(z, targets, row_seq, hist_index, penalty):
    out = z.clone()
    for r in range(z.shape[0]):
        hist = sorted({targets[q] for q in range(z.shape[0]) if row_seq[q] == row_seq[r] and hist_index[q] < hist_index[r]})
        if penalty != 1.0 and hist:
            ids = torch.tensor(hist, dtype=torch.long)
            s = z[r, ids]
            out[r, ids] = torch.where(s < 0, s * np.float32(penalty), s / np.float32(penalty))
    return out


@pytest.mark.parametrize('V', VOCABS)
@pytest.mark.parametrize('n', [1, 13, 70])
@pytest.mark.parametrize('penalty', [1.0, 1.5])
def test_score_rows_equal_logprobs_on_the_host_penalised_rows(V, n, penalty):
    from callireader_amd.engine import op_logprobs, op_score_rows
    z, targets, row_seq, hist_index, nan_row = make_case(V, n, seed=V + n)
    zp = host_penalised(z, targets, row_seq, hist_index, penalty)
    if penalty != 1.0 and n > 1:
        moved = [r for r in range(n) if r != nan_row and zp[r, targets[r]] != z[r, targets[r]]]
        assert any(z[r, targets[r]] < 0 for r in moved) and any(z[r, targets[r]] > 0 for r in moved)      # a target penalised on either side
    top_n = 8 if n != 13 else 3
    zc = z.cuda()
    before = zc.clone()
    got = [t.cpu() for t in op_score_rows(zc, targets, row_seq, hist_index, penalty, top_n)]
    assert torch.equal(zc.cpu().view(torch.int32), before.cpu().view(torch.int32))              # the logits are never modified
    want = [t.cpu() for t in op_logprobs(zp.cuda(), targets, top_n)]
    ok = [r for r in range(n) if r != nan_row]
    if nan_row is not None:
        assert torch.isnan(got[0][nan_row]) and torch.isnan(want[0][nan_row])
    for a, b, what in zip(got, want, ('lp', 'top_ids', 'top_lp')):
        assert torch.equal(a[ok], b[ok]), what
    # float64 reference on the penalised rows
    ls = torch.log_softmax(zp[ok].double(), -1)
    lp64 = ls.gather(1, torch.tensor([targets[r] for r in ok]).reshape(-1, 1))[:, 0]
    order = torch.sort(zp[ok], dim=-1, descending=True, stable=True).indices[:, :top_n]
    e1 = float((got[0][ok].double() - lp64).abs().max())
    e2 = float((got[2][ok].double() - ls.gather(1, order)).abs().max())
    print(f'V={V} n={n} penalty={penalty}: max |logprob err| {e1:.3e}, max |top logprob err| {e2:.3e}')
    assert torch.equal(got[1][ok].long(), order)
    assert e1 <= TOL and e2 <= TOL, (e1, e2)


@pytest.mark.parametrize('V', VOCABS)
def test_a_rows_result_does_not_depend_on_the_launch(V):
    """Row X with a history of three earlier targets (one of them X's own): in a launch of those four rows, and inside a 70-row launch at other positions,
    as another history, with other ordinals in between."""
    from callireader_amd.engine import op_score_rows
    z, targets, row_seq, hist_index, _ = make_case(V, 70, seed=5)
    z[7] = z[8]                                              # no NaN row here
    g = torch.Generator().manual_seed(1)
    four = (torch.randn(4, V, generator=g) * 3.0).clamp(-20, 20)
    ids = [11, V - 1, 11, V - 1]
    four[3, V - 1] = 2.5
    four[3, 11] = -1.5
    small = [t.cpu() for t in op_score_rows(four.cuda(), ids, [0, 0, 0, 0], [0, 1, 2, 3], 1.5, 8)]
    for at in ((0, 1, 2, 3), (66, 67, 68, 69), (5, 30, 31, 64), (64, 20, 3, 1)):      # (also: row order need not follow the ordinals)
        zz, tg, rs, hi = z.clone(), list(targets), list(row_seq), list(hist_index)
        for k, r in enumerate(at):
            zz[r] = four[k]
            tg[r], rs[r], hi[r] = ids[k], 2, 10 * k + 1
        big = [t.cpu() for t in op_score_rows(zz.cuda(), tg, rs, hi, 1.5, 8)]
        for a, b in zip(small, big):
            assert torch.equal(a[3], b[at[3]]), at
    one = [t.cpu() for t in op_score_rows(four[:1].cuda(), ids[:1], [0], [0], 1.5, 8)]
    for a, b in zip(small, one):
        assert torch.equal(a[0], b[0])


def test_score_rows_without_alternatives_and_refusals():
    from callireader_amd.engine import op_score_rows
    from callireader_amd._binding import CalliReaderError
    z, targets, row_seq, hist_index, _ = make_case(8201, 5, seed=2)
    zc = z.cuda()
    lp0, ti, tl = op_score_rows(zc, targets, row_seq, hist_index, 1.5, 0)
    assert ti is None and tl is None
    assert torch.equal(lp0.cpu(), op_score_rows(zc, targets, row_seq, hist_index, 1.5, 4)[0].cpu())
    for bad in (dict(targets=[8201] + targets[1:]), dict(targets=[-1] + targets[1:]), dict(row_seq=[5] + row_seq[1:]), dict(hist_index=[-1] + hist_index[1:]),
                dict(penalty=0.0)):
        kw = dict(targets=targets, row_seq=row_seq, hist_index=hist_index, penalty=1.5)
        kw.update(bad)
        with pytest.raises(CalliReaderError, match='error -1'):
            op_score_rows(zc, kw['targets'], kw['row_seq'], kw['hist_index'], kw['penalty'], 1)

"""cr_kv_fanout (csrc/kv.hip, ABI v13): several sampled first picks from ONE prefill.

`src` is prefilled once with sampling on; every destination must then be, bit for bit, what a lone prefill of the same prompt with its seed leaves:
  - its first id is cr_op_sample's on the prefill's raw last row with that seed at step 0, and the numpy replica's (sampling.gumbel over the kept set);
  - cache rows [0, S) of every layer, K and V are the source's, rows >= S (a sentinel written beforehand) are not touched, the source is unchanged;
  - length, ids, stop state and the token-score record equal a lone sequence's in a second cache, and so do the ids and the raw logits of 16 further decode
    steps (the fanned-out rows decode as one batch, the lone one alone);
  - a first id that is the EOS id finishes its sequence at once and leaves its siblings alone;
  - every refusal leaves every sequence as it was.
Prompt lengths 1, 63, 64, 65 (both sides of the copy kernel's 64-position tile) and 250 (16 decode steps cross the decode attention's 256-key split);
1, 7 and 63 destinations."""
import ctypes as C

import numpy as np
import pytest
import torch

from callireader_amd import sampling as S
from callireader_amd import synthetic
from callireader_amd.config import ModelDims

pytestmark = pytest.mark.gpu

V, PEN, LAYERS, STEPS = 9000, 1.5, 2, 16
SETTINGS = {'warped': S.SamplingParams(0.7, 5, 0.8), 'plain': S.SamplingParams(1.0, 0, 1.0)}
CASES = [(1, 1), (1, 7), (63, 7), (64, 1), (64, 7), (65, 7), (65, 63), (250, 7)]
SENTINEL = 3                  # rows behind the prompt that the destinations hold beforehand


@pytest.fixture(scope='module')
def llm():
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    dims = ModelDims.reduced(vit_layers=1, llm_layers=LAYERS, rs_depth=1, vocab=V)
    m = InternVLChatModel.from_state_dict(synthetic.make_state_dict(dims, seed=3), dims, max_tokens=512, max_pages=64)
    g = torch.Generator().manual_seed(7)
    prompts = {s: m.engine.embed_splice(torch.randint(0, V, (s,), generator=g)) for s in (1, 63, 64, 65, 250)}
    other = m.engine.embed_splice(torch.randint(0, V, (250 + SENTINEL,), generator=g))
    lone = m._kv_alloc(1, 512)
    yield m, prompts, other, lone
    lone.free()
    m.close()


def poll(kv):
    out = torch.zeros(1 + 2 * kv.n_seqs, dtype=torch.int32).pin_memory()
    kv.poll_finished(out)
    torch.cuda.synchronize()
    return out.tolist()


def rows_of(kv, seq, lo, hi):
    """cache rows [lo, hi) of a sequence: [layer, K|V, position, 8, 128] bf16"""
    return torch.stack([torch.stack([torch.stack([kv.read(l, seq, p, w) for p in range(lo, hi)]) for w in (0, 1)]) for l in range(LAYERS)])


def state_of(kv, seqs):
    p = poll(kv)
    N = kv.n_seqs
    return [(kv.length(s), kv.generated(s), p[1 + N + s]) for s in seqs], p[0]


def seeds_for(n, src_seed):
    """n destination seeds: distinct ones, except that the second repeats the first and the last is the source's own"""
    sd = [S.splitmix64(1000 + j) for j in range(n)]
    if n > 2:
        sd[1] = sd[0]
        sd[-1] = src_seed
    return sd


def kept_set(row, sp):
    """The device's kept set of an fp32 row (numpy, its documented rules): z = row / T in fp32; top-k keeps z >= the k-th largest; top-p removes the
    ascending fp32 softmax cumsum <= fp32(1 - top_p) of the survivors, keeps the maximum, and every id tied with the smallest kept score."""
    z = row.astype(np.float32)
    if sp.temperature != 1.0:
        z = z / np.float32(sp.temperature)
    keep = np.ones(len(z), dtype=bool)
    if 0 < sp.top_k < len(z):
        keep = z >= np.sort(z)[-sp.top_k]
    if sp.top_p < 1.0:
        idx = np.nonzero(keep)[0]
        o = idx[np.argsort(z[idx], kind='stable')]
        zz = z[o].astype(np.float64)
        pr = np.exp(zz - zz.max())
        cum = np.cumsum(pr / pr.sum())
        rem = cum <= float(np.float32(1.0 - sp.top_p))
        rem[-1] = False
        thr = z[o[~rem]].min()
        keep = keep & (z >= thr)
    return z, np.nonzero(keep)[0]


def replica_draw(row, sp, seed, step=0):
    z, kept = kept_set(row, sp)
    sc = z[kept].astype(np.float64) + S.gumbel(seed, step, kept)
    o = np.argsort(-sc, kind='stable')
    return int(kept[o[0]]), (sc[o[0]] - sc[o[1]] if len(o) > 1 else np.inf), len(kept)


def prefill_src(m, kv, emb, sp, seed, lpn=0, eos=None, budget=0, seq=0):
    """reset(seq), its sampling / score / stop state, its prefill; returns the raw last row"""
    kv.reset(seq)
    kv.set_sampling(seq, sp.temperature, sp.top_k, sp.top_p, seed)
    if lpn:
        kv.set_logprobs(seq, lpn)
    if eos is not None or budget:
        kv.set_stop(seq, eos, budget)
    return m.engine.prefill(kv, seq, emb, penalty=PEN, want_logits=True)


@pytest.mark.parametrize('S_len,n_dst', CASES)
@pytest.mark.parametrize('setting', sorted(SETTINGS))
def test_fanout_equals_lone_prefills(llm, S_len, n_dst, setting):
    from callireader_amd.engine import op_sample
    m, prompts, other, lone = llm
    sp, emb = SETTINGS[setting], prompts[S_len]
    kv = m.kv(64)
    dsts = list(range(1, n_dst + 1))
    src_seed = S.splitmix64(5)
    seeds = seeds_for(n_dst, src_seed)
    lpn = 3 if setting == 'warped' else 0                 # token scores on in one setting, off in the other
    budget = 10                                           # a stop inside the 16 steps: the stop state is compared after it, too
    # the sentinel: every destination holds another, longer prompt's rows
    kv.reset()
    m.engine.prefill_batch(kv, dsts, [other[:S_len + SENTINEL]] * n_dst, penalty=PEN)
    sentinel = {d: rows_of(kv, d, S_len, S_len + SENTINEL) for d in (dsts[0], dsts[-1])}
    kv.reset()
    row = prefill_src(m, kv, emb, sp, src_seed, lpn, budget=budget)
    src_rows, (src_state, _) = rows_of(kv, 0, 0, S_len), state_of(kv, [0])
    src_lp = kv.logprobs(0) if lpn else None
    row_before = row.clone()
    kv.fanout(0, dsts, seeds, row)
    assert torch.equal(row, row_before)                                            # nobody writes the row
    # --- first pick: cr_op_sample on the raw row, and the numpy replica
    first = [kv.generated(d) for d in dsts]
    assert all(len(f) == 1 for f in first)
    ids, kept = op_sample(m.engine, row[None].expand(n_dst, V), sp.temperature, sp.top_k, sp.top_p, seeds, 0)
    assert [f[0] for f in first] == ids.cpu().tolist()
    row_h, near = row.cpu().numpy(), 0
    for f, sd, k in zip(first, seeds, kept.cpu().tolist()):
        wid, gap, nk = replica_draw(row_h, sp, sd)
        assert nk == k, (nk, k)
        if gap < 1e-4:                                                              # the double-precision logs of two libraries: no verdict on a near tie
            near += 1
            continue
        assert f[0] == wid, (f[0], wid, gap)
    assert near <= 1
    if n_dst > 2:
        assert first[1] == first[0] and first[-1] == kv.generated(0)               # the same seed draws the same id: the source's seed the source's id
    # --- cache contents: the prefix is the source's, the sentinel is intact, the source is unchanged
    for d in dsts:
        assert torch.equal(rows_of(kv, d, 0, S_len), src_rows), d
    for d, want in sentinel.items():
        assert torch.equal(rows_of(kv, d, S_len, S_len + SENTINEL), want), d
    assert torch.equal(rows_of(kv, 0, 0, S_len), src_rows) and state_of(kv, [0])[0] == src_state
    if lpn:
        assert all(np.array_equal(a, b) for a, b in zip(kv.logprobs(0), src_lp))
    # --- equality with a lone sequence, state and 16 decode steps (the fanned-out rows as ONE batch, the source among them)
    batch = [0] + dsts
    lg_batch = [m.engine.decode(kv, batch, penalty=PEN, want_logits=True).clone() for _ in range(STEPS)]
    after, _ = state_of(kv, batch)
    for r, (s, sd) in enumerate(zip(batch, [src_seed] + seeds)):
        lrow = prefill_src(m, lone, emb, sp, sd, lpn, budget=budget)
        assert torch.equal(lrow, row)
        st0, _ = state_of(lone, [0])
        assert st0[0] == (S_len, first[r - 1] if r else kv.generated(0)[:1], 0)
        for t in range(STEPS):
            lg = m.engine.decode(lone, [0], penalty=PEN, want_logits=True)
            assert torch.equal(lg[0], lg_batch[t][r]), (s, t)
        st1, _ = state_of(lone, [0])
        assert st1[0] == after[r], (s, st1[0], after[r])                            # lengths, all 17 ids, the stop count (the budget of 10)
        assert after[r][2] == budget
        if lpn:
            a, b = kv.logprobs(s), lone.logprobs(0)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].shape == (STEPS + 1, 3), s


def test_first_id_that_is_eos_finishes_its_sequence(llm):
    m, prompts, other, lone = llm
    sp, emb = SETTINGS['warped'], prompts[65]
    kv = m.kv(64)
    kv.reset()
    row = prefill_src(m, kv, emb, sp, 1).cpu().numpy()
    draws = {sd: replica_draw(row, sp, sd) for sd in (S.splitmix64(j) for j in range(40))}
    draws = {sd: d[0] for sd, d in draws.items() if d[1] >= 1e-4}
    src_id = kv.generated(0)[0]
    eos = next(i for i in draws.values() if i != src_id)                           # the EOS id lowered into the kept set: an id some seed draws first
    hit = [sd for sd, i in draws.items() if i == eos][:2]
    miss = [sd for sd, i in draws.items() if i != eos][:5]
    seeds = miss[:2] + hit[:1] + miss[2:] + hit[1:]
    dsts = list(range(3, 3 + len(seeds)))
    kv.reset()
    lg = prefill_src(m, kv, emb, sp, 1, eos=eos)
    kv.fanout(0, dsts, seeds, lg)
    p, N = poll(kv), kv.n_seqs
    want_done = [d for d, sd in zip(dsts, seeds) if sd in hit]
    assert p[0] == len(want_done) and sorted(p[1:1 + p[0]]) == want_done            # finished and queued like any other
    for d, sd in zip(dsts, seeds):
        assert p[1 + N + d] == (1 if sd in hit else 0) and kv.generated(d) == [draws[sd]]
    assert p[1 + N + 0] == 0
    # the siblings run on, with the ids of their lone runs
    for _ in range(4):
        m.engine.decode(kv, [0] + dsts, penalty=PEN)
    for d, sd in zip(dsts, seeds):
        prefill_src(m, lone, emb, sp, sd, eos=eos)
        for _ in range(4):
            m.engine.decode(lone, [0], penalty=PEN)
        assert kv.generated(d) == lone.generated(0) and poll(lone)[1 + 1 + 0] == poll(kv)[1 + N + d], d


def test_refusals_change_nothing(llm):
    from callireader_amd import _binding as B
    from callireader_amd.constraints import Constraints
    from callireader_amd.engine import _p, _stream
    m, prompts, other, lone = llm
    sp, emb = SETTINGS['warped'], prompts[63]
    kv = m.kv(64)
    kv.reset()
    row = prefill_src(m, kv, emb, sp, 9)
    prefill_src(m, kv, other[:20], sp, 4, seq=5)                                   # a bystander that holds something
    watch = [0, 1, 2, 5, 10, 11, 20, 21, 63]

    def snapshot():
        return state_of(kv, watch), rows_of(kv, 1, 0, 4), rows_of(kv, 5, 0, 4)

    def refused(code, src, dsts, seeds=None, logits=row, cache=kv):
        before = snapshot()
        with pytest.raises(B.CalliReaderError, match=f'error {code}:'):
            cache.fanout(src, dsts, [7] * len(dsts) if seeds is None else seeds, logits)
        after = snapshot()
        assert before[0] == after[0] and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])
    ARG, STATE = -1, -3
    refused(ARG, 0, [])                                                            # n_dst outside 1..63
    refused(ARG, 0, list(range(1, 64)) + [1])                                      # 64 destinations
    refused(ARG, 0, [0])                                                           # the source
    refused(ARG, 0, [1, 2, 1])                                                     # repeated
    refused(ARG, 0, [64])
    refused(ARG, 0, [-1])
    refused(ARG, 64, [1])
    refused(ARG, 0, [1], logits=None)                                              # null last_logits
    before = snapshot()
    assert B.lib.cr_kv_fanout(kv._h, 0, (C.c_int32 * 1)(1), 1, None, _p(row), _stream()) == ARG      # null seeds
    assert B.lib.cr_kv_fanout(None, 0, (C.c_int32 * 1)(1), 1, (C.c_uint64 * 1)(7), _p(row), _stream()) == ARG
    assert snapshot()[0] == before[0]
    kv.set_beam(10, 2, eos_id=None, max_new=8)                                     # sequences 10 and 11: a beam group
    refused(STATE, 0, [11])
    refused(STATE, 10, [1])
    m.engine.prefill(kv, 20, emb, penalty=PEN)                                     # a greedy source
    refused(STATE, 20, [1])
    kv.set_sampling(21, sp.temperature, sp.top_k, sp.top_p, 3)
    refused(STATE, 21, [1])                                                        # a source that samples but has not been prefilled: no id
    kv.set_constraints(5, Constraints(no_repeat_ngram_size=2))                     # a source that carries constraints
    refused(STATE, 5, [1])
    kv.set_constraints(5, None)
    m.engine.decode(kv, [5], penalty=PEN)                                          # ... and one that holds two ids
    refused(STATE, 5, [1])
    e4 = m.engine.kv_alloc(2, 128, dtype='e4m3')
    try:
        lg = prefill_src(m, e4, emb, sp, 9)
        with pytest.raises(B.CalliReaderError, match=f'error {ARG}:'):
            e4.fanout(0, [1], [7], lg)
        assert e4.length(1) == 0 and e4.generated(1) == [] and len(e4.generated(0)) == 1
    finally:
        e4.free()
    kv.fanout(0, [1], [7], row)                                                    # and the same call with good arguments goes through
    assert kv.length(1) == 63 and len(kv.generated(1)) == 1

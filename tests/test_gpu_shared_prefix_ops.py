"""The decode attention over shared prompts alone (cr_op_decode_attention_shared; csrc/attention_decode_group.hip), on a real MI355X.

Two caches with the same contents as far as a reader may see them:
  - the MATERIALISED one, in which every sharer holds a copy of its source's rows [0, pfx_len): what cr_kv_fork leaves;
  - the SHARED one, in which those rows of a sharer are NaN: what cr_kv_fork_shared leaves, with poison where it writes nothing.
op_decode_attention_shared on the shared cache must equal op_decode_attention on the materialised one BIT FOR BIT (torch.equal), and no NaN may come out: the
poison shows that the source was read.  There is no tolerance anywhere: the group form runs the per-row kernel's own device function for each row.

Shapes: 12 slots, max_tokens 1 104, 8 KV heads x 4 query heads x 128.  pfx_len 256 / 512 / 768 (1, 2, 3 shared splits); own lengths pfx_len + {0, 1, 255, 256, 300}
mixed inside a group (the first unshared split empty but for the new token, one key, full, full plus one, two more splits); groups of 1, 2, 3, 8 and 9 rows (9: the
cut into chunks of 8), the source inside the launch and outside it; two groups plus unshared rows in one launch, members not adjacent and in permuted order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SLOTS, MAX_TOKENS, H, G, D = 12, 1104, 8, 4, 128
DELTAS = [0, 1, 255, 256, 300]


def dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def E():
    from callireader_amd import engine
    return engine


@pytest.fixture(scope='module')
def base():
    """Random K / V for every slot and 12 query rows: made once, never written (every case clones what it changes)"""
    g = torch.Generator().manual_seed(33)
    kc = torch.randn((N_SLOTS, H, MAX_TOKENS, D), generator=g).to(torch.bfloat16).to(dev())
    vc = torch.randn((N_SLOTS, H, MAX_TOKENS, D), generator=g).to(torch.bfloat16).to(dev())
    q = (torch.randn((N_SLOTS, H * G * D), generator=g) * 0.7).to(torch.bfloat16).to(dev())
    return kc, vc, q


def caches(base, rows):
    """rows: (slot, own length, pfx_src, pfx_len) per launch row.  Returns the materialised and the shared K / V and the lengths by slot."""
    kc, vc, _ = base
    mk, mv, sk, sv = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    lens = torch.zeros(N_SLOTS, dtype=torch.int32)
    for slot, length, src, plen in rows:
        lens[slot] = length
        if src >= 0:
            mk[slot, :, :plen] = kc[src, :, :plen]
            mv[slot, :, :plen] = vc[src, :, :plen]
            sk[slot, :, :plen] = float('nan')
            sv[slot, :, :plen] = float('nan')
    return (mk, mv), (sk, sv), lens.to(dev())


def run_both(E, base, rows, q_rows=None):
    """(shared result, materialised result) of one launch"""
    (mk, mv), (sk, sv), lens = caches(base, rows)
    q = base[2][:len(rows)].contiguous() if q_rows is None else q_rows
    seqs = torch.tensor([r[0] for r in rows], dtype=torch.int32, device=dev())
    max_keys = max(r[1] for r in rows) + 1
    want = E.op_decode_attention(q, mk, mv, seqs, lens, max_keys=max_keys)
    got = E.op_decode_attention_shared(q, sk, sv, seqs, lens, [r[2] for r in rows], [r[3] for r in rows], max_keys=max_keys)
    torch.cuda.synchronize()
    return got, want


@pytest.mark.parametrize('source_in_launch', [False, True])
@pytest.mark.parametrize('size', [1, 2, 3, 8, 9])
@pytest.mark.parametrize('plen', [256, 512, 768])
def test_one_group_equals_the_materialised_cache(E, base, plen, size, source_in_launch):
    src = 11
    rows = [(j, plen + DELTAS[(j + size) % len(DELTAS)], src, plen) for j in range(size)]
    if source_in_launch:
        rows.insert(size // 2, (src, plen + 37, -1, 0))                     # the source's own row, in the middle of its sharers
    got, want = run_both(E, base, rows)
    assert not torch.isnan(got.float()).any() and not torch.isnan(want.float()).any()
    assert torch.equal(got, want)


def test_two_groups_and_unshared_rows_in_permuted_order(E, base):
    """Group A: source 10 (outside the launch), 512 shared, members 0, 3, 7.  Group B: source 5 (inside), 256 shared, members 1, 8.  Unshared: 2, 6, 9.  Group A's
    members sit at rows 0, 4 and 8, B's at 2 and 6, B's source at row 7."""
    A, B_ = (10, 512), (5, 256)
    rows = [(0, 512 + 300, *A), (2, 40, -1, 0), (1, 256 + 0, *B_), (6, 700, -1, 0), (3, 512 + 1, *A), (9, 256, -1, 0), (8, 256 + 255, *B_), (5, 256 + 256, -1, 0),
            (7, 512 + 255, *A)]
    got, want = run_both(E, base, rows)
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got, want)
    # the same rows in another order: a row's bits follow the row
    perm = [4, 7, 0, 8, 2, 5, 1, 6, 3]
    q = base[2][:len(rows)][perm].contiguous()
    got2, want2 = run_both(E, base, [rows[i] for i in perm], q_rows=q)
    assert torch.equal(got2, want2) and torch.equal(got2, got[perm])


def test_a_launch_without_shares_is_the_plain_launch(E, base):
    rows = [(j, 100 + 190 * j, -1, 0) for j in range(5)]
    got, want = run_both(E, base, rows)
    assert torch.equal(got, want)


def test_a_member_gives_the_same_bits_alone_in_two_and_in_eight(E, base):
    src, plen = 11, 512
    member = (4, plen + 300, src, plen)
    q = base[2]
    outs = []
    for size in (1, 2, 8):
        others = [(j, plen + DELTAS[j % len(DELTAS)], src, plen) for j in (0, 1, 2, 3, 5, 6, 7)][:size - 1]
        rows = others + [member]                                            # the member last: its row index differs from launch to launch
        qr = torch.cat([q[:len(others)], q[4:5]]).contiguous()
        got, want = run_both(E, base, rows, q_rows=qr)
        assert torch.equal(got, want)
        outs.append(got[-1].clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_bad_shares_are_refused(E, base):
    from callireader_amd import _binding as B
    rows = [(0, 600, 11, 512), (1, 600, 11, 512)]
    (mk, mv), (sk, sv), lens = caches(base, rows)
    seqs = torch.tensor([0, 1], dtype=torch.int32, device=dev())
    q = base[2][:2].contiguous()
    for bad in (100, 257, 768):                                             # no multiple of 256; past max_keys = 601
        with pytest.raises(B.CalliReaderError, match='error -1:'):
            E.op_decode_attention_shared(q, sk, sv, seqs, lens, [11, 11], [512, bad], max_keys=601)
    with pytest.raises(ValueError):
        E.op_decode_attention_shared(q, sk, sv, seqs, lens, [11], [512], max_keys=601)

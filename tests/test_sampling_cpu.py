"""Sampled generation, host side (callireader_amd/sampling.py): the generation-config parsing of _gen_args, the numpy Philox-4x32-10 replica
the GPU tests compare the device's draws with (Random123 known answers), and the per-page seed derivation."""
import numpy as np
import pytest
import torch

from callireader_amd import sampling as S


def gen_args(**kw):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    return InternVLChatModel._gen_args(kw)


def test_do_sample_alone_is_top50():
    max_new, eos, sp = gen_args(do_sample=True, max_new_tokens=7)
    assert max_new == 7
    assert (sp.temperature, sp.top_k, sp.top_p) == (1.0, 50, 1.0)


def test_explicit_values_and_greedy():
    _, _, sp = gen_args(do_sample=True, temperature=0.8, top_p=0.8, top_k=0)
    assert (sp.temperature, sp.top_k, sp.top_p) == (0.8, 0, 0.8)
    assert gen_args(do_sample=False, top_k=5, temperature=0.3)[2] is None         # do_sample=False ignores the warpers, as transformers does
    assert gen_args(max_new_tokens=3)[2] is None


@pytest.mark.parametrize('kw', [dict(temperature=0), dict(temperature=-1.0), dict(top_p=1.5), dict(top_p=-0.1), dict(top_k=-1),
                                dict(temperature=float('inf')), dict(temperature=float('nan')), dict(temperature=1e-50), dict(temperature=1e300),
                                dict(top_p=float('nan'))])
def test_invalid_values_raise_value_error(kw):
    with pytest.raises(ValueError):
        gen_args(do_sample=True, **kw)


@pytest.mark.parametrize('kw', [dict(typical_p=0.5), dict(min_p=0.1), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=1e-3), dict(no_repeat_ngram_size=3)])
def test_unsupported_knobs_raise(kw):
    with pytest.raises(NotImplementedError):
        gen_args(do_sample=True, **kw)


def test_tiny_finite_temperature_is_accepted():
    assert gen_args(do_sample=True, temperature=1e-30)[2].temperature == 1e-30      # a positive fp32 value: scores may overflow to inf (documented)


@pytest.mark.parametrize('t,k,p', [(float('inf'), 50, 1.0), (float('nan'), 50, 1.0), (-0.5, 50, 1.0), (1.0, -1, 1.0), (1.0, 50, 1.5),
                                   (1.0, 50, float('nan')), (float('-inf'), 0, 1.0)])
def test_abi_refuses_bad_sampling_state(t, k, p):
    """cr_kv_set_sampling checks its values before anything else: no device, no cache needed."""
    from callireader_amd import _binding as B
    assert B.lib.cr_kv_set_sampling(None, 0, t, k, p, 0, None) == B.lib.cr_kv_set_sampling(None, 0, t, k, p, 1, None) == -1
    assert b'temperature' in B.lib.cr_last_error()
    assert B.lib.cr_kv_set_sampling(None, 0, 0.7, 50, 0.9, 0, None) == -1
    assert b'bad sequence' in B.lib.cr_last_error()                  # good values: it is the missing cache that is refused


def test_beams_still_raise():
    with pytest.raises(NotImplementedError):
        gen_args(num_beams=2)
    with pytest.raises(NotImplementedError):
        gen_args(num_beams=2, do_sample=True)


# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, expected output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers(ctr, key, want):
    got = S.philox4x32_10(np.array(ctr, dtype=np.uint32), key)
    assert [int(v) for v in got] == list(want)


def test_uniforms_layout():
    seed, step = 0x0123456789ABCDEF, 9
    ids = np.arange(10)
    u = S.uniforms(seed, step, ids)
    assert np.all((u > 0) & (u < 1))
    # id i reads word i % 4 of the block at counter (i // 4, step, 0, 0), key (low, high) of the seed
    blk = S.philox4x32_10(np.array([[i, step, 0, 0] for i in range(3)], dtype=np.uint32), (seed & 0xFFFFFFFF, seed >> 32))
    want = ((blk.reshape(-1)[:10] >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    assert np.array_equal(u, want)
    assert not np.array_equal(u, S.uniforms(seed, step + 1, ids))


def test_seed_derivation():
    torch.manual_seed(3)
    a = S.page_seeds(5)
    torch.manual_seed(3)
    b = S.page_seeds(5)
    assert a == b and len(set(a)) == 5 and all(0 <= s < 1 << 64 for s in a)
    torch.manual_seed(4)
    assert S.page_seeds(5) != a
    assert S.page_seeds(3, base=10) == [S.splitmix64(10 + j) for j in range(3)]
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF                  # the first output of SplitMix64 seeded with 0

"""Sampled generation on the host side: the parameters (transformers' semantics and defaults), the per-page seeds, and an exact numpy
replica of the device's random numbers (include/callireader_hip.h, cr_kv_set_sampling) for tests and offline checks.

The token choice itself runs on the device (csrc/sample.hip).  The distribution is transformers 4.45.2's
(RepetitionPenalty -> Temperature -> TopK -> TopP -> softmax draw); the draws are not torch.multinomial's: a page's ids depend only on
(seed, step, logits, history), so they do not change with the batch a page decodes in."""
import math
from dataclasses import dataclass

import numpy as np
import torch

# GenerationConfig defaults for this model (transformers' _get_default_generation_params; the reference's config.json carries the same)
DEFAULT_TEMPERATURE, DEFAULT_TOP_K, DEFAULT_TOP_P = 1.0, 50, 1.0

# sampling knobs the device does not implement: a non-default value raises NotImplementedError (name -> the value that means "off")
UNSUPPORTED = {'min_p': None, 'typical_p': 1.0, 'epsilon_cutoff': 0.0, 'eta_cutoff': 0.0, 'no_repeat_ngram_size': 0,
               'encoder_no_repeat_ngram_size': 0, 'bad_words_ids': None, 'sequence_bias': None, 'suppress_tokens': None,
               'begin_suppress_tokens': None, 'diversity_penalty': 0.0, 'num_beam_groups': 1, 'penalty_alpha': None, 'guidance_scale': None,
               'renormalize_logits': False}

# rows of one batched decode step (the decode kernels' limit): pages x returned sequences of one call
MAX_ROWS = 64


@dataclass(frozen=True)
class SamplingParams:
    """do_sample=True as transformers applies it: temperature > 0, top_k >= 0 (0: off), 0 <= top_p <= 1 (1: off)."""
    temperature: float = DEFAULT_TEMPERATURE
    top_k: int = DEFAULT_TOP_K
    top_p: float = DEFAULT_TOP_P

    def __post_init__(self):
        t, k, p = self.temperature, self.top_k, self.top_p
        if not (isinstance(t, (int, float)) and t > 0):
            raise ValueError(f'`temperature` (={t}) has to be a strictly positive float, otherwise your next token scores will be invalid.')
        # the device divides in fp32: a temperature must stay a positive finite fp32 number (inf would make every score 0, 1e-50 would become 0 = greedy)
        with np.errstate(over='ignore'):
            t32 = float(np.float32(t))
        if not (math.isfinite(t32) and t32 > 0):
            raise ValueError(f'`temperature` (={t}) has to be a finite positive float32 value (about 1.2e-38 .. 3.4e38)')
        if not isinstance(k, int) or isinstance(k, bool) or k < 0:
            raise ValueError(f'`top_k` has to be a non-negative integer, but is {k}')
        if not (isinstance(p, (int, float)) and 0.0 <= p <= 1.0):
            raise ValueError(f'`top_p` has to be a float >= 0 and <= 1, but is {p}')


MAX_BEAMS = 8

# beam knobs the device does not implement (name -> the value that means "off")
BEAM_UNSUPPORTED = {'num_return_sequences': 1, 'num_beam_groups': 1, 'diversity_penalty': 0.0, 'constraints': None, 'force_words_ids': None,
                    'penalty_alpha': None, 'low_memory': None, 'custom_generate': None}


@dataclass(frozen=True)
class BeamParams:
    """num_beams > 1 as transformers' deterministic beam search takes it: length_penalty (exponent of the hypothesis length a finished score is divided
    by), early_stopping False | True | 'never'."""
    num_beams: int
    length_penalty: float = 1.0
    early_stopping: object = False

    def __post_init__(self):
        b, lp, es = self.num_beams, self.length_penalty, self.early_stopping
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 2:
            raise ValueError(f'`num_beams` has to be an integer strictly greater than 1, but is {b!r}')
        if b > MAX_BEAMS:
            raise NotImplementedError(f'num_beams={b}: the device keeps at most {MAX_BEAMS} beams per page')
        if isinstance(lp, bool) or not isinstance(lp, (int, float)) or not math.isfinite(lp):
            raise ValueError(f'`length_penalty` has to be a finite float, but is {lp!r}')
        if not (es is True or es is False or es == 'never'):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es!r}.")       # transformers' GenerationConfig.validate

    @property
    def early_code(self):
        return early_code(self.early_stopping)


def early_code(early_stopping):
    """cr_kv_set_beam's early_stopping: 0 False, 1 True, 2 'never'."""
    return 2 if early_stopping == 'never' else 1 if early_stopping else 0


def parse_beams(kwargs):
    """BeamParams for num_beams > 1, None for num_beams=1 (length_penalty and early_stopping are then ignored, as transformers does).
    ValueError for a num_beams that is no integer >= 1; NotImplementedError for num_beams above 8, beam sampling (do_sample=True), more than one
    returned sequence, group / diverse / constrained beams, and token scores together with beams."""
    b = kwargs.get('num_beams', 1)
    if b is None:
        b = 1
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
        raise ValueError(f'`num_beams` has to be a positive integer, but is {b!r}')
    if b == 1:
        return None
    if kwargs.get('do_sample', False):
        raise NotImplementedError(f'num_beams={b} with do_sample=True (beam sampling) is not implemented: beam search is deterministic here')
    for k, off in BEAM_UNSUPPORTED.items():
        v = kwargs.get(k, off)
        if v is not None and v != off:
            raise NotImplementedError(f'{k}={v!r} is not implemented with num_beams={b} (beam search returns its one best sequence; no group, diverse '
                                      'or constrained beams)')
    if kwargs.get('output_scores') or kwargs.get('return_scores') or kwargs.get('output_logits'):
        raise NotImplementedError(f'token scores (output_scores / return_scores) are not implemented with num_beams={b}: '
                                  'return_dict_in_generate=True gives sequences_scores')
    lp, es = kwargs.get('length_penalty'), kwargs.get('early_stopping')
    return BeamParams(int(b), 1.0 if lp is None else lp, False if es is None else es)


def parse_returns(kwargs):
    """num_return_sequences of a generation config: n >= 1 sampled answers per page (1, the default: today's single answer).  ValueError for a value
    that is no integer >= 1, and -- transformers 4.45.2's GenerationConfig.validate, in its words -- for n > 1 with do_sample=False and num_beams=1.
    With num_beams > 1 it is parse_beams that speaks (n > 1 is not implemented there)."""
    n = kwargs.get('num_return_sequences', 1)
    if n is None:
        n = 1
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f'`num_return_sequences` has to be a positive integer, but is {n!r}')
    n = int(n)
    if n > 1 and parse_beams(kwargs) is None and not kwargs.get('do_sample', False):
        raise ValueError(f'Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {n}).')
    return n


def parse_share(kwargs):
    """share_prompt of a generation config (not one of transformers' keywords): False (the default), or True -- a page's beams or sampled answers read ONE
    cached copy of its prompt in decode instead of one each (KVCache.set_prefix_sharing; the same ids, bit for bit).  ValueError for anything but a bool."""
    v = kwargs.get('share_prompt', False)
    if v is None:
        return False
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f'`share_prompt` has to be True or False, but is {v!r}')
    return bool(v)


SHARE_ENTRY_POINTS = 'generate / generate_ocr / generate_origin, chat_ocr, dynamic_chat, chat_ocr_pages and generate_pages'


def refuse_share(what):
    """The NotImplementedError of an entry point or a feature that does not take share_prompt=True, naming the alternative."""
    raise NotImplementedError(f'share_prompt=True is not implemented with {what}: leave it off there (the copying fan-out gives the same ids), or use '
                              f'{SHARE_ENTRY_POINTS} on a bf16 cache')


def check_rows(P, n):
    """P pages x n returned sequences have to fit one batched decode step."""
    if P * n > MAX_ROWS:
        raise ValueError(f'{P} pages x {n} returned sequences = {P * n} decode rows: at most {MAX_ROWS} (the batched decode kernels)')


def fan_seeds(P, n, base=None):
    """Seeds of one call over P pages with n returned sequences each, [P][n]: sample j of page i has page_seeds(P * n, base)[i * n + j] -- the row order
    of transformers' repeat_interleave expansion.  With n = 1 these are page_seeds(P, base)."""
    flat = page_seeds(P * n, base)
    return [flat[i * n:(i + 1) * n] for i in range(P)]


def parse(kwargs):
    """SamplingParams for do_sample=True, None for greedy or beam search (do_sample=False ignores temperature, top_k and top_p, as transformers does).
    Raises what parse_beams raises for num_beams, what parse_returns raises for num_return_sequences (the count itself is parse_returns'), and
    NotImplementedError for any other sampling knob set to a non-default value."""
    parse_beams(kwargs)
    parse_returns(kwargs)
    if not kwargs.get('do_sample', False):
        return None
    for k, off in UNSUPPORTED.items():
        v = kwargs.get(k, off)
        if v is not None and v != off:
            raise NotImplementedError(f'{k}={v!r} is not implemented (sampling supports temperature, top_k, top_p and repetition_penalty)')
    t = kwargs.get('temperature')
    k = kwargs.get('top_k')
    p = kwargs.get('top_p')
    return SamplingParams(DEFAULT_TEMPERATURE if t is None else float(t), DEFAULT_TOP_K if k is None else int(k),
                          DEFAULT_TOP_P if p is None else float(p))


MASK64 = (1 << 64) - 1


def splitmix64(x):
    """SplitMix64 (Steele, Lea, Flood 2014) finaliser of x + golden gamma."""
    z = (int(x) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def base_seed():
    """One 62-bit base seed per sampling call, drawn from torch's default CPU generator: torch.manual_seed(n) makes a call reproducible."""
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())


def page_seeds(n, base=None):
    """Seeds of pages 0 .. n-1 of one call (input order): splitmix64(base + j)."""
    base = base_seed() if base is None else int(base)
    return [splitmix64(base + j) for j in range(n)]


# ---- host replica of the device's random numbers -----------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Philox-4x32-10 over arrays: ctr uint32 [..., 4], key = (k0, k1) uint32 scalars -> uint32 [..., 4]."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(seed, step, ids):
    """u_i in (0, 1) (float64) of token ids `ids` at (seed, step): ((x >> 8) + 0.5) * 2^-24, x = word i % 4 of Philox(counter (i/4, step, 0, 0))."""
    ids = np.asarray(ids, dtype=np.int64)
    ctr = np.zeros(ids.shape + (4,), dtype=np.uint32)
    ctr[..., 0] = (ids // 4).astype(np.uint32)
    ctr[..., 1] = np.uint32(step)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.take_along_axis(x, (ids % 4)[..., None], axis=-1)[..., 0]
    return ((w >> 8).astype(np.float64) + 0.5) * 2.0 ** -24


def gumbel(seed, step, ids):
    """The noise g_i = -log(-log u_i) (float64) the device adds to the kept scores."""
    return -np.log(-np.log(uniforms(seed, step, ids)))

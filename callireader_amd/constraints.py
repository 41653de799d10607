"""Logits constraints of greedy generation on the host side: the parameters (transformers' keys, semantics and error texts) and their per-page
form.  The masks themselves are applied on the device, per sequence, in front of the pick (csrc/constrain.hip, cr_kv_set_constraints).

    no_repeat_ngram_size   NoRepeatNGramLogitsProcessor
    bad_words_ids          NoBadWordsLogitsProcessor (a sequence_bias whose biases are all -inf is the same thing and is taken as such)
    suppress_tokens        SuppressTokensLogitsProcessor
    begin_suppress_tokens  SuppressTokensAtBeginLogitsProcessor (the first generated id: generation starts from inputs_embeds)
    min_new_tokens / min_length   MinNewTokensLength / MinLengthLogitsProcessor -- the same thing here (the processors see the generated ids only):
                           the larger of the two holds
    allowed_token_ids      this project's key: a whitelist, i.e. suppress_tokens over its complement.  The call's EOS id is ALWAYS kept permitted
                           (a documented difference: a whitelist that cannot stop is never wanted)

Greedy decoding only: with do_sample=True or num_beams > 1 any constraint raises NotImplementedError."""
import math
from dataclasses import dataclass

import numpy as np

# constraint-like knobs the device does not implement (name -> the value that means "off")
CONSTRAINTS_UNSUPPORTED = {'prefix_allowed_tokens_fn': None, 'encoder_no_repeat_ngram_size': 0, 'force_words_ids': None}

_UNSET = object()


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _id_tuple(name, v):
    if v is None:
        return ()
    if _is_int(v):
        v = [v]
    v = list(v)
    if any(not _is_int(t) or t < 0 for t in v):
        raise ValueError(f'`{name}` has to be a list of non-negative integers, but is {v}')
    return tuple(int(t) for t in v)


@dataclass(frozen=True)
class Constraints:
    """The constraints of one page.  min_new_tokens is the larger of the call's min_new_tokens / min_length; eos_token_id is the id it bans (None: none)."""
    no_repeat_ngram_size: int = 0
    bad_words_ids: tuple = ()
    suppress_tokens: tuple = ()
    begin_suppress_tokens: tuple = ()
    min_new_tokens: int = 0
    allowed_token_ids: tuple = None
    eos_token_id: int = None

    def __post_init__(self):
        n, m = self.no_repeat_ngram_size, self.min_new_tokens
        if not _is_int(n) or n < 0:
            raise ValueError(f'`ngram_size` has to be a strictly positive integer, but is {n}')
        if not _is_int(m) or m < 0:
            raise ValueError(f'`min_new_tokens` has to be a positive integer, but is {m}')
        for w in self.bad_words_ids:
            if len(w) == 0:
                raise ValueError(f'Each list in `bad_words_ids` has to be a list of positive integers, but is {[list(x) for x in self.bad_words_ids]}.')
        if self.allowed_token_ids is not None and len(self.allowed_token_ids) == 0:
            raise ValueError('`allowed_token_ids` has to be a non-empty list of token ids')

    @property
    def active(self):
        return bool(self.no_repeat_ngram_size or self.bad_words_ids or self.suppress_tokens or self.begin_suppress_tokens or
                    (self.min_new_tokens and self.eos_token_id is not None) or self.allowed_token_ids is not None)

    def banned_static(self, vocab):
        """The ids banned at every step (sorted): suppress_tokens, one-id bad words, the whitelist's complement."""
        s = set(self.suppress_tokens) | {w[0] for w in self.bad_words_ids if len(w) == 1}
        if self.allowed_token_ids is not None:
            s |= set(range(vocab)) - set(self.allowed_token_ids)
        return sorted(s)


def _bad_words(v):
    """transformers' NoBadWordsLogitsProcessor validation, its texts."""
    if not isinstance(v, (list, tuple)) or len(v) == 0:
        raise ValueError(f'`bad_words_ids` has to be a non-empty list, but is {v}.')
    if any(not isinstance(w, (list, tuple)) for w in v):
        raise ValueError(f'`bad_words_ids` has to be a list of lists, but is {v}.')
    if any(len(w) == 0 or any(not _is_int(t) or t < 0 for t in w) for w in v):
        raise ValueError(f'Each list in `bad_words_ids` has to be a list of positive integers, but is {v}.')
    return tuple(tuple(int(t) for t in w) for w in v)


def parse(kwargs, eos_token_id=_UNSET):
    """Constraints for the generation keywords `kwargs`, or None when none is set.  eos_token_id: the call's EOS id (default: kwargs' own; a list's first).
    ValueError (transformers' texts) for invalid values; NotImplementedError for a constraint together with do_sample=True or num_beams > 1, and for
    the knobs of CONSTRAINTS_UNSUPPORTED and a sequence_bias with finite biases."""
    for k, off in CONSTRAINTS_UNSUPPORTED.items():
        v = kwargs.get(k, off)
        if v is not None and v != off:
            raise NotImplementedError(f'{k} is not implemented (the device applies no_repeat_ngram_size, bad_words_ids, suppress_tokens, '
                                      'begin_suppress_tokens, min_new_tokens / min_length and allowed_token_ids; callable and forcing constraints are not among them)')
    eos = kwargs.get('eos_token_id') if eos_token_id is _UNSET else eos_token_id
    if isinstance(eos, (list, tuple)):
        if len(eos) > 1:
            raise NotImplementedError(f'eos_token_id={eos!r}: one EOS id per call')
        eos = eos[0] if eos else None
    n = kwargs.get('no_repeat_ngram_size')
    n = 0 if n is None else n
    if not _is_int(n) or n < 0:
        raise ValueError(f'`ngram_size` has to be a strictly positive integer, but is {n}')
    mn, ml = kwargs.get('min_new_tokens'), kwargs.get('min_length')
    mn, ml = 0 if mn is None else mn, 0 if ml is None else ml
    if not _is_int(mn) or mn < 0:
        raise ValueError(f'`min_new_tokens` has to be a positive integer, but is {mn}')
    if not _is_int(ml) or ml < 0:
        raise ValueError(f'`min_length` has to be a non-negative integer, but is {ml}')
    bw = kwargs.get('bad_words_ids')
    bw = () if bw is None else _bad_words(bw)
    sb = kwargs.get('sequence_bias')
    if sb:
        items = list(sb.items()) if isinstance(sb, dict) else [tuple(e) for e in sb]
        if any(not (isinstance(b, (int, float)) and math.isinf(b) and b < 0) for _, b in items):
            raise NotImplementedError('sequence_bias with finite biases is not implemented (the device masks; a bias of -inf is taken as a bad word)')
        bw = bw + _bad_words([list(w) for w, _ in items])
    allowed = kwargs.get('allowed_token_ids')
    if allowed is not None:
        allowed = _id_tuple('allowed_token_ids', allowed)
        if not allowed:
            raise ValueError('`allowed_token_ids` has to be a non-empty list of token ids')
        if eos is not None and int(eos) not in allowed:
            allowed = allowed + (int(eos),)                # the whitelist rule: the call can always stop
    c = Constraints(int(n), bw, _id_tuple('suppress_tokens', kwargs.get('suppress_tokens')),
                    _id_tuple('begin_suppress_tokens', kwargs.get('begin_suppress_tokens')), int(max(mn, ml)), allowed, None if eos is None else int(eos))
    if not c.active:
        return None
    if kwargs.get('do_sample', False):
        raise NotImplementedError('logits constraints with do_sample=True are not implemented (greedy decoding only)')
    b = kwargs.get('num_beams', 1)
    if b is not None and b != 1:
        raise NotImplementedError(f'logits constraints with num_beams={b} are not implemented: transformers masks the log-probabilities there, which changes '
                                  "the beam scores' normalisation (greedy decoding only)")
    return c


def per_page(constraints, P):
    """[Constraints or None] per page from generate_pages' `constraints` argument: None, one for every page, or a list with one entry per page."""
    if constraints is None:
        return [None] * P
    cs = list(constraints) if isinstance(constraints, (list, tuple)) else [constraints] * P
    if len(cs) != P:
        raise ValueError(f'constraints: {len(cs)} entries for {P} pages')
    if any(c is not None and not isinstance(c, Constraints) for c in cs):
        raise TypeError('constraints: Constraints objects (constraints.parse) or None')
    return [c if c is not None and c.active else None for c in cs]

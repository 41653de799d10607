"""Token scores on the host side: the keyword arguments, and the containers the generation and chat entry points return.

The numbers come from the device (csrc/logprobs.hip, cr_kv_set_logprobs in include/callireader_hip.h): for the t-th generated id, the
log-softmax of the fp32 score row the pick chose from -- the LM-head logits after the repetition penalty and BEFORE temperature / top-k /
top-p -- at that id, and the n best entries of the row (descending, the lower id first on an exact tie).  For greedy generation this is
transformers' compute_transition_scores(sequences, scores, normalize_logits=True).  This module needs no GPU."""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

MAX_TOP = 8


def check_top_n(n, name='top_logprobs', allow_zero=False):
    """An int in 1..8 (0..8 with allow_zero); ValueError otherwise."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (0 if allow_zero else 1) <= int(n) <= MAX_TOP:
        raise ValueError(f'`{name}` has to be an integer in {0 if allow_zero else 1}..{MAX_TOP}, but is {n!r}')
    return int(n)


def per_page(logprobs, P):
    """`logprobs` of generate_pages / PagePipeline.start / ContinuousPipeline.submit as one int per page: an int for every page, or one per page."""
    if logprobs is None:
        return [0] * P
    if isinstance(logprobs, (list, tuple, np.ndarray)):
        if len(logprobs) != P:
            raise ValueError(f'`logprobs` lists {len(logprobs)} values for {P} pages')
        return [check_top_n(n, 'logprobs', True) for n in logprobs]
    return [check_top_n(logprobs, 'logprobs', True)] * P


def parse(kwargs):
    """The number of alternatives a generate call asked for (0: none, the call returns what it always did).

    return_dict_in_generate=True with output_scores=True asks for scores, `top_logprobs` (default 1) for that many alternatives per id.
    output_logits / output_attentions / output_hidden_states with return_dict_in_generate raise NotImplementedError;
    return_dict_in_generate without output_scores gives 0 (the caller wraps the ids in a GenerateOutput without scores)."""
    if not kwargs.get('return_dict_in_generate', False):
        return 0                                          # (`top_logprobs` may sit in a generation_config that chat(..., return_scores=True) reads)
    for k in ('output_logits', 'output_attentions', 'output_hidden_states'):
        if kwargs.get(k):
            raise NotImplementedError(f'{k}=True is not implemented: the generation loop keeps no per-step tensors on the host '
                                      '(output_scores=True returns per-token log-probabilities and top_logprobs alternatives)')
    if not kwargs.get('output_scores', False):
        return 0                                          # a GenerateOutput with `sequences` alone
    n = kwargs.get('top_logprobs')
    return 1 if n is None else check_top_n(n)


@dataclass
class TokenScores:
    """Scores of one sequence's generated ids, cut to the ids that are returned (EOS kept, speculative ids past the stop dropped):
    logprobs float32 [T], top_ids int32 [T, n], top_logprobs float32 [T, n]."""
    logprobs: np.ndarray
    top_ids: np.ndarray
    top_logprobs: np.ndarray

    def __post_init__(self):
        self.logprobs = np.asarray(self.logprobs, dtype=np.float32).reshape(-1)
        T = len(self.logprobs)
        self.top_ids = np.asarray(self.top_ids, dtype=np.int32).reshape(T, -1)
        self.top_logprobs = np.asarray(self.top_logprobs, dtype=np.float32).reshape(T, -1)
        if self.top_ids.shape != self.top_logprobs.shape:
            raise ValueError(f'top_ids {self.top_ids.shape} and top_logprobs {self.top_logprobs.shape} differ')

    def __len__(self):
        return len(self.logprobs)

    def cut(self, T):
        """The first T steps (the returned ids' count); ValueError when fewer were recorded."""
        if T > len(self):
            raise ValueError(f'{T} ids but only {len(self)} scored steps')
        return TokenScores(self.logprobs[:T].copy(), self.top_ids[:T].copy(), self.top_logprobs[:T].copy())

    @classmethod
    def read(cls, kv, seq, T):
        """The first T steps of KVCache.logprobs(seq) (synchronises the current stream)."""
        lp, ti, tl = kv.logprobs(seq)
        return cls(lp, ti, tl).cut(T)


@dataclass
class GenerateOutput:
    """What generate / generate_ocr / generate_origin return under return_dict_in_generate=True, output_scores=True: `sequences` is the tensor
    returned otherwise ([1, T] new ids, EOS included); token_logprobs [1, T], top_ids [1, T, n], top_logprobs [1, T, n] are torch tensors on the CPU."""
    sequences: object
    token_logprobs: object
    top_ids: object
    top_logprobs: object
    scores: Optional[TokenScores] = None          # the same numbers as numpy arrays
    sequences_scores: object = None               # beam search (num_beams > 1): [1] float32, the returned hypothesis' length-penalised score

    def __getitem__(self, k):
        return getattr(self, k)


def generate_output(sequences, ts=None):
    import torch
    if ts is None:
        return GenerateOutput(sequences, None, None, None, None)
    return GenerateOutput(sequences, torch.from_numpy(ts.logprobs)[None], torch.from_numpy(ts.top_ids)[None], torch.from_numpy(ts.top_logprobs)[None], ts)


def generate_outputs(sequences, tss=None):
    """The GenerateOutput of num_return_sequences = n > 1: `sequences` [n, L] (right-padded), and with scores the per-sequence fields as LISTS of n --
    token_logprobs[j] [T_j], top_ids[j] / top_logprobs[j] [T_j, k] for sample j's own T_j ids, `scores` the n TokenScores."""
    import torch
    if tss is None:
        return GenerateOutput(sequences, None, None, None, None)
    return GenerateOutput(sequences, [torch.from_numpy(t.logprobs) for t in tss], [torch.from_numpy(t.top_ids) for t in tss],
                          [torch.from_numpy(t.top_logprobs) for t in tss], list(tss))


@dataclass
class TokenScore:
    id: int
    piece: str
    logprob: float
    top: List[tuple] = field(default_factory=list)        # [(id, piece, logprob)] descending


@dataclass
class ResponseScores:
    """Chat-level scores: one TokenScore per generated id (EOS included), and the aggregates over the tokens that survive
    skip_special_tokens (the ones the response text is made of): mean_logprob, min_logprob, min_index (into `tokens`), confidence = exp(mean)."""
    tokens: List[TokenScore]
    kept: List[int]                     # indices into tokens of the non-special ones
    mean_logprob: float
    min_logprob: float
    min_index: int
    confidence: float
    total_logprob: float = float('nan')     # sum over the kept tokens: log P(text) up to the special ids (scoring.py ranks candidates by it)

    @classmethod
    def build(cls, tokenizer, ids, ts):
        ids = [int(i) for i in ids]
        ts = ts.cut(len(ids))
        special = set(int(i) for i in getattr(tokenizer, 'all_special_ids', []) or [])
        pieces = tokenizer.convert_ids_to_tokens(ids) if ids else []
        tokens = []
        for t, (i, pc) in enumerate(zip(ids, pieces)):
            alt_ids = [int(a) for a in ts.top_ids[t] if a >= 0]
            alt_pc = tokenizer.convert_ids_to_tokens(alt_ids) if alt_ids else []
            tokens.append(TokenScore(i, pc, float(ts.logprobs[t]), [(a, p, float(l)) for a, p, l in zip(alt_ids, alt_pc, ts.top_logprobs[t])]))
        kept = [t for t, i in enumerate(ids) if i not in special]
        if kept:
            lps = [tokens[t].logprob for t in kept]
            mean = float(sum(lps) / len(lps))
            k = min(range(len(lps)), key=lambda j: lps[j])
            return cls(tokens, kept, mean, float(lps[k]), kept[k], math.exp(mean), float(sum(lps)))
        return cls(tokens, kept, float('nan'), float('nan'), -1, float('nan'))

    def pieces(self):
        """The pieces of the kept tokens, in order: tokenizer.convert_tokens_to_string of them is the response before stripping."""
        return [self.tokens[t].piece for t in self.kept]

    def to_json(self, total=False):
        """Plain lists and floats (inference.py --scores writes this per image).  total: also `total_logprob` (inference.py --score_answer)."""
        if total:
            return dict(self.to_json(), total_logprob=self.total_logprob)
        return {'tokens': [tk.piece for tk in self.tokens], 'ids': [tk.id for tk in self.tokens],
                'logprobs': [tk.logprob for tk in self.tokens],
                'alternatives': [[{'id': a, 'token': p, 'logprob': l} for a, p, l in tk.top] for tk in self.tokens],
                'kept': list(self.kept), 'mean_logprob': self.mean_logprob, 'min_logprob': self.min_logprob, 'min_index': self.min_index,
                'confidence': self.confidence}

    def summary_line(self):
        """`confidence <c> min <p> at token <k> (<piece>)`"""
        piece = self.tokens[self.min_index].piece if self.min_index >= 0 else ''
        return f'confidence {self.confidence:.4f} min {self.min_logprob:.4f} at token {self.min_index} ({piece})'

"""Scoring a given text (cr_llm_score_batch in include/callireader_hip.h): the host side, which needs no GPU.

A scoring call is one prefill-shaped pass over  prompt ++ embed(y[0 .. T-1))  in which row P - 1 + j predicts y[j]: the rows to feed and the per-row targets
are built here, the arguments are validated here, and the device's numbers become a scores.ResponseScores here -- per-token log-probability and alternatives
as chat_ocr(return_scores=True) reports them for a text it generated, plus total_logprob, the sum over the kept tokens, which ranks candidates."""
from dataclasses import dataclass
from typing import List

import numpy as np

from .scores import ResponseScores, check_top_n


@dataclass
class ScorePlan:
    """ids = the scored ids y (EOS appended when asked for), feed = y[:-1], the ids whose embedding rows follow the prompt rows, targets = one entry per row
    of prompt ++ feed: -1 for the first prompt_len - 1 rows, then y (row prompt_len - 1 + j is scored against y[j])."""
    ids: List[int]
    feed: List[int]
    targets: List[int]


def plan(prompt_len, answer_ids, eos_id=None, score_eos=True, vocab=None):
    """The ScorePlan of an answer behind a prompt of prompt_len rows.  score_eos appends eos_id to the scored ids (the stop is part of the text's
    probability); without it, or without an eos_id, the answer is scored alone.  ValueError for an empty prompt, an answer that leaves nothing to score, or an id
    outside 0..vocab-1."""
    if isinstance(prompt_len, bool) or not isinstance(prompt_len, (int, np.integer)) or prompt_len < 1:
        raise ValueError(f'scoring needs a prompt of at least one row, got {prompt_len!r}')
    ids = [int(t) for t in answer_ids]
    if score_eos and eos_id is not None:
        ids.append(int(eos_id))
    if not ids:
        raise ValueError('nothing to score: an empty answer (and no EOS id to score with score_eos)')
    for t in ids:
        if t < 0 or (vocab is not None and t >= vocab):
            raise ValueError(f'answer id {t} is outside the vocabulary' + (f' (0..{vocab - 1})' if vocab is not None else ''))
    return ScorePlan(ids, ids[:-1], [-1] * (int(prompt_len) - 1) + ids)


def check_penalty(p, name='repetition_penalty'):
    if isinstance(p, bool) or not isinstance(p, (int, float, np.floating, np.integer)) or not (p > 0) or p == float('inf'):
        raise ValueError(f'`{name}` has to be a finite number > 0, but is {p!r}')
    return float(p)


def check_fits(rows, cached, max_tokens):
    if cached + rows > max_tokens:
        raise ValueError(f'{cached} cached + {rows} rows to score exceed the KV cache ({max_tokens} tokens)')


def refuse_generation(generation_config=None, draft=None, what='scoring'):
    """A scoring entry point generates nothing: the keywords that steer a generation are refused (ValueError), not ignored."""
    gc = dict(generation_config or {})
    if gc.get('do_sample'):
        raise ValueError(f'{what}: do_sample=True (a given text is scored under the greedy definition: the penalised logits before any warper)')
    nb = gc.get('num_beams')
    if nb is not None and nb != 1:
        raise ValueError(f'{what}: num_beams={nb!r} (there is nothing to search: the text is given)')
    for k in ('no_repeat_ngram_size', 'bad_words_ids', 'suppress_tokens', 'begin_suppress_tokens', 'allowed_token_ids', 'min_new_tokens', 'min_length',
              'constraints', 'force_words_ids', 'prefix_allowed_tokens_fn'):
        if gc.get(k):
            raise ValueError(f'{what}: {k} (logits constraints shape a generation; a given text is scored on the unconstrained distribution)')
    if draft is not None or gc.get('draft_ids') is not None:
        raise ValueError(f'{what}: draft (a draft speeds up a generation; there is none here)')
    return gc


def answer_to_ids(tokenizer, answer):
    """`answer` as ids: a string goes through the tokenizer without special tokens, a list of ids is taken as it is."""
    if isinstance(answer, str):
        enc = tokenizer(answer, add_special_tokens=False) if _takes_add_special(tokenizer) else tokenizer(answer)
        ids = enc['input_ids']
        ids = ids.reshape(-1).tolist() if hasattr(ids, 'reshape') else list(ids)
        if ids and isinstance(ids[0], (list, tuple)):
            ids = list(ids[0])
        return [int(t) for t in ids]
    return [int(t) for t in answer]


def _takes_add_special(tokenizer):
    import inspect
    try:
        ps = inspect.signature(tokenizer.__call__).parameters
    except (TypeError, ValueError):
        return True
    return 'add_special_tokens' in ps or any(p.kind == p.VAR_KEYWORD for p in ps.values())


def response_scores(tokenizer, ids, token_scores):
    """scores.ResponseScores of the scored ids (EOS included when it was scored; the aggregates run over the non-special ones)."""
    return ResponseScores.build(tokenizer, ids, token_scores)


def top_n_of(top_logprobs):
    return check_top_n(top_logprobs, 'top_logprobs', allow_zero=True)

"""The host side of generation, once: the prompt-length check, the admission of sequences into a cache, the chunked decode loop of the greedy
and sampled rows, the EOS / budget cut and the reply text.  Plain functions of an engine and a cache, so the caller's engine (generate_pages,
_generate, session.PageSession) and a pipeline's second context (pipeline.PagePipeline) run the same code.  ContinuousPipeline admits through
`admit` too; its worker stops rows on the device and is a different loop (continuous.py).  Beam search keeps its own loop (its finish test is the
group's done flag: InternVLChatModel._generate_pages_beams)."""
import time

import torch

from .draft import MAX_ROWS, DraftCursor, fit_rows
from .sampling import page_seeds
from .scores import TokenScores


def check_fits(S, max_new, max_tokens):
    """A prompt of S tokens and max_new new ones have to fit a sequence of the cache."""
    if S + max_new > max_tokens:
        raise ValueError(f'prompt of {S} tokens + {max_new} new exceeds max_tokens={max_tokens}')


def cut_ids(ids, eos, budget):
    """The ids a caller gets: at most `budget` of them, cut behind the first EOS (ids past it were speculative; the reference stops there)."""
    ids = ids[:budget]
    return ids[:ids.index(eos) + 1] if eos is not None and eos in ids else ids


def per_page_sampling(sampling, seeds, P):
    """[(SamplingParams, seed) or None] per page from generate_pages' sampling / seeds arguments."""
    if sampling is None:
        return None
    sps = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling] * P
    if len(sps) != P:
        raise ValueError(f'sampling: {len(sps)} entries for {P} pages')
    if seeds is None:
        seeds = page_seeds(P)
    if len(seeds) != P:
        raise ValueError(f'seeds: {len(seeds)} entries for {P} pages')
    return [None if sp is None else (sp, int(sd)) for sp, sd in zip(sps, seeds)]


def share_cache(kv, on):
    """The cache's prefix-sharing mode for the call that has just reset it whole (KVCache.set_prefix_sharing is accepted on an empty cache only).  A call
    that leaves the mode as it is -- every call without share_prompt on a cache that never shared -- issues nothing."""
    if bool(getattr(kv, 'prefix_sharing', False)) != bool(on):
        kv.set_prefix_sharing(bool(on))


def release_shared(kv, groups):
    """The end of a call that shared prompts.  groups: per page its sequences, the one the others read first.  Sharers are reset BEFORE their source (the
    cache refuses the other order), then the mode goes off: the cache is left as a call without share_prompt expects it."""
    for g in groups:
        for s in g[1:]:
            kv.reset(s)
    for g in groups:
        kv.reset(g[0])
    share_cache(kv, False)


def admit(engine, kv, seqs, embeds_list, penalty, per_page=None, lpn=(), prefill_batch=16, reset_each=False, constraints=()):
    """Put one prompt into each of the sequences `seqs`: reset (the whole cache in one call, or with reset_each only these sequences), then the sampled
    pages' state (per_page: per_page_sampling's list), then the constrained pages' (constraints: a constraints.Constraints or None per page), then the
    scored pages' (lpn: alternatives per id, 0 = off), then the prefill in groups of
    `prefill_batch` -- prompts of several pages share the linear layers' GEMMs, and the prefill makes every page's first pick (its step 0)."""
    if any(c is not None and e is not None for c, e in zip(constraints or (), per_page or ())):
        raise NotImplementedError('logits constraints on a sampled page are not implemented (greedy decoding only)')
    if reset_each:
        for s in seqs:
            kv.reset(s)
    else:
        kv.reset()
    for s, e in zip(seqs, per_page or ()):
        if e is not None:
            kv.set_sampling(s, e[0].temperature, e[0].top_k, e[0].top_p, e[1])
    for s, c in zip(seqs, constraints or ()):
        if c is not None:
            kv.set_constraints(s, c)
    for s, n in zip(seqs, lpn):
        if n:
            kv.set_logprobs(s, n)
    for i0 in range(0, len(seqs), prefill_batch):
        engine.prefill_batch(kv, seqs[i0:i0 + prefill_batch], embeds_list[i0:i0 + prefill_batch], penalty=penalty)


def decode_rows(engine, kv, seqs, max_new_tokens, eos, penalty, check_every=16, budgets=None, look_first=False, on_chunk=None):
    """The decode behind a prefill of the sequences `seqs` (each holds its first id): all unfinished ones as one batch per step, in chunks of
    `check_every` steps.  After each chunk a row leaves when it has its budget of ids (budgets: one per sequence, default max_new_tokens for all) or
    EOS is among them; returns the ids per sequence, in seqs order, as cut_ids cuts them.  Ids are read back (which synchronises the current stream)
    only at such a look, and only where the answer can matter: with eos None, once per row, at its budget.
    look_first: also look before the first chunk -- the one-sequence path (_generate), where a prefill whose own pick is EOS issues no decode step.
    The batch paths do not: a read-back there would hold the host's issue of the first decode step until the whole prefill has run.
    on_chunk(steps, rows, seconds): called after each chunk's steps are issued, with the host time that took (PagePipeline's counters)."""
    budget = dict(zip(seqs, budgets if budgets is not None else [max_new_tokens] * len(seqs)))
    live, done, n = list(seqs), {}, 1

    def look():
        for i in list(live):
            if eos is not None or n >= budget[i]:
                ids = kv.generated(i)
                if n >= budget[i] or eos in ids:
                    done[i] = cut_ids(ids, eos, budget[i])
                    live.remove(i)
    if look_first or max_new_tokens <= 1:
        look()
    while n < max_new_tokens and live:
        steps = min(check_every, max_new_tokens - n)
        t0 = time.perf_counter()
        for _ in range(steps):
            engine.decode(kv, live, penalty=penalty)
        if on_chunk is not None:
            on_chunk(steps, len(live), time.perf_counter() - t0)
        n += steps
        look()
    return [done[i] for i in seqs]


def decode_rows_drafted(engine, kv, seqs, max_new_tokens, eos, penalty, drafts, budgets=None, stats=None):
    """decode_rows with a draft per sequence (drafts: a list of ids or None, in seqs order): the same ids, in fewer steps where a draft is right.  Every
    step is one cr_llm_decode_draft over the unfinished rows, each with the window its draft.DraftCursor offers -- at most what its budget and the cache
    leave, and shortened (draft.fit_rows) so that the step stays within 64 rows.  The call synchronises, so each step reads the ids it appended: they move the
    cursors, and a row leaves at its EOS or budget at once (no speculative steps behind it).  A step always appends one id per row, so a wrong draft never
    costs more than one plain step per id.  More than 64 unfinished rows take plain steps.
    stats (a dict, optional) receives steps, drafted (ids offered) and accepted (ids appended beyond the one a plain step appends)."""
    budget = dict(zip(seqs, budgets if budgets is not None else [max_new_tokens] * len(seqs)))
    cursors = {i: DraftCursor(d) if d else None for i, d in zip(seqs, drafts)}
    ids, done, live = {}, {}, []
    st = dict(steps=0, drafted=0, accepted=0)

    def take(i, new):
        ids[i].extend(new)
        if cursors[i] is not None:
            cursors[i].feed(new)
        if len(ids[i]) >= budget[i] or (eos is not None and eos in new):
            done[i] = cut_ids(ids[i], eos, budget[i])
            return False
        return True
    for i in seqs:
        ids[i] = []
        if take(i, kv.generated(i)):
            live.append(i)
    while live:
        if len(live) > MAX_ROWS:
            engine.decode(kv, live, penalty=penalty)
            windows, app = [[]] * len(live), [1] * len(live)
        else:
            room = [min(budget[i] - len(ids[i]), kv.max_tokens - kv.length(i)) - 1 for i in live]
            windows = fit_rows([cursors[i].window(r) if cursors[i] is not None else [] for i, r in zip(live, room)])
            app = engine.decode_draft(kv, live, windows, penalty=penalty)
        st['steps'] += 1
        st['drafted'] += sum(len(w) for w in windows)
        st['accepted'] += sum(app) - len(live)
        live = [i for i, a in zip(live, app) if take(i, kv.generated(i)[-a:])]
    if stats is not None:
        stats.update(st)
    return [done[i] for i in seqs]


def read_scores(kv, lpn, outs):
    """TokenScores of the scored pages (None for the others), cut to the ids returned; on the current stream."""
    return [TokenScores.read(kv, i, len(ids)) if n else None for i, (n, ids) in enumerate(zip(lpn, outs))]


def reply_text(tokenizer, ids, sep):
    """The response of one sequence's new ids (a list, or the [1, T] tensor a generate_* call returns): decoded, cut at the template's separator."""
    ids = ids if torch.is_tensor(ids) else torch.tensor([ids])
    return tokenizer.batch_decode(ids, skip_special_tokens=True)[0].split(sep)[0].strip()


def reply_shape(response, history, scores, return_history, return_scores):
    """response[, history][, scores]: what chat, chat_ocr and dynamic_chat return."""
    out = (response,) + ((history,) if return_history else ()) + ((scores,) if return_scores else ())
    return out if len(out) > 1 else response

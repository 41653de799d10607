"""Page sessions: several turns about ONE page on one KV cache.

The reference's choice / bilingual / intent tasks ask for the transcription and then put the real question as a second chat_ocr call on the
same image with `history=` (evaluate.py:257-287, 321-342, 357-378).  That second call repeats the page's visual stage and prefills a prompt
whose first ~3 000 tokens the cache held a moment ago.  A PageSession (InternVLChatModel.open_page) runs the visual stage once, keeps the
page's ViT embeddings and pseudo-token rows, and owns a bf16 KV cache of 1 + max_branches sequences: sequence 0, the TRUNK, carries the
conversation from turn to turn; the others are BRANCHES that ask_many forks off it for one batch of questions.

A turn
    p = longest common prefix of the ids at the trunk's cached positions and the new prompt's ids (at most len(prompt) - 1: a prefill needs a row)
    KV.truncate(0, p)   cr_kv_truncate: the trunk keeps positions [0, p) and forgets ids, criteria, sampling state and scores -- the
                        speculative rows behind EOS are cut, and the new turn's repetition penalty sees this turn's ids only, as the
                        processors of the reference's `generate` call do
    embed rows [p, S), one continued prefill (cr_llm_prefill appends at the cached length), the decode loop of _generate

Why a common id prefix is a common embedding prefix: within a session row i of the spliced prompt depends only on ids[0..i] -- a plain id takes
its table row, the k-th <IMG_CONTEXT> takes ViT row k and the k-th aligned token takes pseudo-token row k, k counted from the prompt's start --
and the rows behind them are the session's own tensors, the same for every turn.  p is computed on IDS, not text: where re-tokenising the
history's answer does not give back the generated ids the prefix ends, and the rest is prefilled again.  That costs rows, never correctness.

What a session turn is: the reference's chat_ocr(history=...) turn, held to the oracle like every other greedy path (tests/test_gpu_session.py).
It is deterministic -- the same calls give the same bits -- but it is NOT promised bit-equal to a non-session chat_ocr: a continued prefill puts
its rows in other company inside the attention waves of deeper layers.  A branch gives the ids the same question gives when asked alone from the
same trunk state (greedy decoding; sampled branches have their own seeds: ask_many).

Not here (NotImplementedError): num_beams > 1 (cr_kv_set_beam needs empty sequences: use chat_ocr(history=...)), e4m3 caches (no bf16 prefix
to continue from: use kv_cache_dtype='bf16'), region_wise (one turn), and the pipelines / sharded entry points, which own their caches.
"""
import torch

from .constraints import parse as constraints_parse
from . import draft as drafting
from . import grounding
from . import scoring
from .generation import check_fits, decode_rows, decode_rows_drafted, reply_text
from .sampling import page_seeds, parse_beams


def common_prefix(a, b):
    """Length of the longest common prefix of two id lists."""
    n = min(len(a), len(b))
    i = 0
    while i < n and a[i] == b[i]:
        i += 1
    return i


def plan_prefix(cached_ids, prompt_ids):
    """p of a turn: the cached positions the prompt keeps.  Capped at len(prompt) - 1 -- the prefill that makes the turn's first pick needs a row."""
    return min(common_prefix(cached_ids, prompt_ids), len(prompt_ids) - 1)


def fork_groups(prefixes):
    """ask_many's forks: {prefix length: [question indices]} in first-seen order, one cr_kv_fork per distinct length."""
    groups = {}
    for j, p in enumerate(prefixes):
        groups.setdefault(p, []).append(j)
    return groups


def _refuse_e4m3(model):
    if getattr(model, 'kv_cache_dtype', 'bf16') != 'bf16':
        raise NotImplementedError("a page session continues a cached prefix, and an e4m3 cache keeps no bf16 prefix for a continued prefill to read: "
                                  "open the page on a model with kv_cache_dtype='bf16', or use chat_ocr(history=...)")


class PageSession:
    """See the module docstring.  Made by InternVLChatModel.open_page; a context manager (close() frees the cache)."""

    def __init__(self, model, tokenizer, vit_embeds, ref_embeds, n_tiles, use_p=True, max_branches=1, indices=None, boxes=None, per_box=3):
        _refuse_e4m3(model)
        if max_branches < 1:
            raise ValueError(f'max_branches has to be >= 1, got {max_branches}')
        self.m, self.tokenizer, self.use_p, self.n_tiles, self.max_branches = model, tokenizer, use_p, n_tiles, max_branches
        self.vit = vit_embeds.reshape(-1, vit_embeds.shape[-1])                               # [n_tiles * 256, hidden]: <IMG_CONTEXT> k takes row k
        self.ref = ref_embeds.reshape(-1, ref_embeds.shape[-1]).to(torch.bfloat16) if use_p else None           # [n_ref, hidden]: aligned token k takes row k
        self.kv = model.engine.kv_alloc(1 + max_branches, model.max_tokens, dtype='bf16')
        self.cached_ids = []                     # the id at every cached position of the trunk
        self.rows_prefilled = []                 # rows of every prefill the session made (turns and ask_many), in order
        self.align_ids = drafting.from_indices(indices)      # draft='align': the page's CalliAlign indices as vocabulary ids, in reading order
        self.answer_ids = []                     # draft='previous': the ids of the last answer a turn on the trunk generated
        self.boxes = None if boxes is None else [[int(v) for v in b[:4]] for b in boxes]      # ground(): the page's character boxes in reading order
        self.per_box = per_box                   # ground(): pseudo-token rows per box (3, or drop_zero's kept counts)

    @classmethod
    def open(cls, model, tokenizer, detect_model, img_path, use_p=True, drop_zero=False, hard_vq=False, boxes=None, max_branches=1, verbose=False):
        """What chat_ocr does per call before its prompt (:653-688), once: decode the page, its tiles, extract_feature, calli_align."""
        _refuse_e4m3(model)                                                                   # before any visual work
        page, pixel_values = model._open_page(img_path)
        out_tokens = None
        indices = None
        if use_p:
            out_tokens, indices = model.calli_align(page, detect_model, drop_zero=drop_zero, use_hard_vector_quant=hard_vq, verbose=verbose, boxes=boxes)
        return cls(model, tokenizer, model.extract_feature(pixel_values), out_tokens, pixel_values.shape[0], use_p=use_p, max_branches=max_branches,
                   indices=indices, boxes=boxes, per_box=grounding.kept_per_box(indices) if (use_p and drop_zero) else 3)

    # ---- lifetime ----
    def close(self):
        if self.kv is not None:
            self.kv.free()
            self.kv = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- prompts ----
    def _prompt(self, question, history, generation_config, return_scores=False):
        """chat_ocr's own prompt for this page (InternVLChatModel._ocr_prompt: the lines chat_ocr runs) and its ids as a list."""
        if parse_beams(dict(generation_config)) is not None:
            raise NotImplementedError(f"num_beams={generation_config.get('num_beams')} in a page session: cr_kv_set_beam needs empty sequences "
                                      '(beam search runs through chat_ocr(history=...))')
        question, history, template, inputs, gc = self.m._ocr_prompt(self.tokenizer, question, history, self.n_tiles, self.ref, self.use_p, None,
                                                                      generation_config, return_scores)
        return question, history, template, inputs['input_ids'].reshape(-1).tolist(), gc

    def _embed(self, ids, p):
        """Embedding rows [p, S) of the prompt `ids`: the ids before p only say how many visual and pseudo-token rows are used up."""
        img, ref = self.m.img_context_token_id, self.m.aligned_token_id
        head, tail = ids[:p], torch.tensor(ids[p:], dtype=torch.long)
        k_img, n_img = head.count(img), int((tail == img).sum())
        k_ref, n_ref = (head.count(ref), int((tail == ref).sum())) if self.use_p else (0, 0)
        eng = self.m.engine
        if n_img:
            return eng.embed_splice(tail, self.vit[k_img:k_img + n_img], self.ref[k_ref:k_ref + n_ref] if n_ref else None, img_id=img, ref_id=ref)
        if n_ref:                                # aligned tokens without a visual one before them in the tail: the splice's one-kind form on their rows
            return eng.embed_splice(tail, self.ref[k_ref:k_ref + n_ref], None, img_id=ref)
        return eng.embed_splice(tail)

    def _after_turn(self, ids):
        """cached position S + i holds generated id i (the decode step that fed it cached it); the last id generated is cached nowhere yet"""
        self.cached_ids = list(ids) + self.kv.generated(0)[:self.kv.length(0) - len(ids)]

    def _draft_ids(self, draft):
        """draft=None | 'align' (the page's CalliAlign indices) | 'previous' (the session's last answer) | a list of ids -> the ids, or None"""
        if draft is None:
            return None
        if isinstance(draft, str):
            if draft not in ('align', 'previous'):
                raise ValueError(f"draft={draft!r} (want None, 'align', 'previous' or a list of ids)")
            return list(self.align_ids if draft == 'align' else self.answer_ids)
        return [int(t) for t in draft]

    # ---- turns ----
    @torch.no_grad()
    def chat_ocr(self, question, generation_config, history=None, return_history=False, repetition_penalty=1.5, return_scores=False, draft=None):
        """chat_ocr's arguments after the image, and its return values.  The turn runs on the trunk.
        draft: None, 'align', 'previous' or a list of ids (_draft_ids): a guess at the answer, checked several ids per decode step; the answer is the same."""
        draft_ids = self._draft_ids(draft)
        if draft_ids is not None and return_scores:
            drafting.refuse('return_scores')
        question, history, template, ids, gc = self._prompt(question, history, generation_config, return_scores)
        if draft_ids is not None:
            if gc.get('do_sample'):
                drafting.refuse('do_sample=True')                                             # here, before the trunk changes (_generate checks again)
            gc['draft_ids'] = draft_ids
        p = plan_prefix(self.cached_ids, ids)
        max_new, eos, _ = self.m._gen_args({k: v for k, v in gc.items() if k != 'draft_ids'}, allow_beams=True)      # validated here: a refused turn leaves the trunk as it was
        cons = constraints_parse({k: v for k, v in gc.items() if k != 'draft_ids'}, eos)    # (installed by _generate_kw behind the truncate, for this turn only)
        if draft_ids is not None and cons is not None:
            drafting.refuse('logits constraints')
        check_fits(len(ids), max_new, self.m.max_tokens)                                      # before the trunk changes
        self.kv.truncate(0, p)
        self.cached_ids = self.cached_ids[:p]
        embeds = self._embed(ids, p)
        self.rows_prefilled.append(len(ids) - p)
        out = self.m._generate_kw(embeds, repetition_penalty, gc, kv=self.kv, seq=0, reset=False)
        self._after_turn(ids)
        self.answer_ids = (out.sequences if hasattr(out, 'sequences') else out)[0].tolist()
        return self.m._ocr_reply(self.tokenizer, out, template, question, history, return_history, return_scores)

    @torch.no_grad()
    def ask_many(self, questions, generation_config, history=None, repetition_penalty=1.5, draft=None):
        """Several questions about the page as ONE decode batch: every question's prompt is built as chat_ocr builds it (the same `history` for all),
        its branch is forked off the trunk at the prefix the two share, the tails are prefilled together and the branches decode together.  Returns
        the responses in order.  The trunk is not changed -- except that an EMPTY trunk first takes the part all the prompts share.
        Greedy: a branch gives the ids its question gives when asked alone from the same trunk state.  do_sample=True: branch j draws with
        page_seeds(n)[j] (chat_ocr_pages' rule), not with the page_seeds(1)[0] of a lone session.chat_ocr -- reproducible under torch.manual_seed, but
        not the lone call's draws.  No return_scores here.
        draft: as chat_ocr's, one draft for every branch (greedy, no constraints)."""
        draft_ids = self._draft_ids(draft)
        questions = list(questions)
        if not 1 <= len(questions) <= self.max_branches:
            raise ValueError(f'ask_many: {len(questions)} questions for a session opened with max_branches={self.max_branches}')
        m, kv = self.m, self.kv
        built = [self._prompt(q, None if history is None else list(history), generation_config) for q in questions]
        gc, template = built[0][4], built[0][2]
        max_new, eos, sp = m._gen_args(gc, allow_beams=True)
        cons = constraints_parse(gc, eos)
        if draft_ids is not None and sp is not None:
            drafting.refuse('do_sample=True')
        if draft_ids is not None and cons is not None:
            drafting.refuse('logits constraints')
        for _, _, _, ids, _ in built:
            check_fits(len(ids), max_new, m.max_tokens)
        if not self.cached_ids:                  # an empty trunk: what the prompts share goes into it first; the pick that prefill appends is dropped
            first = built[0][3]
            shared = min(min(common_prefix(first, b[3]) for b in built), min(len(b[3]) for b in built) - 1)
            if shared > 0:
                kv.truncate(0, 0)
                m.engine.prefill(kv, 0, self._embed(first[:shared], 0), penalty=repetition_penalty)
                kv.truncate(0, shared)
                self.rows_prefilled.append(shared)
                self.cached_ids = first[:shared]
        prefixes = [plan_prefix(self.cached_ids, b[3]) for b in built]
        branches = list(range(1, 1 + len(built)))
        for p, js in fork_groups(prefixes).items():
            if p > 0:
                kv.fork(0, [branches[j] for j in js], p)
            else:
                for j in js:
                    kv.truncate(branches[j], 0)
        if sp is not None:
            for b, seed in zip(branches, page_seeds(len(branches))):
                kv.set_sampling(b, sp.temperature, sp.top_k, sp.top_p, seed)
        if cons is not None:                     # behind the fork / truncate, which leave a branch without any
            for b in branches:
                kv.set_constraints(b, cons)
        tails = [self._embed(b[3], p) for b, p in zip(built, prefixes)]
        self.rows_prefilled.append(sum(len(b[3]) - p for b, p in zip(built, prefixes)))
        m.engine.prefill_batch(kv, branches, tails, penalty=repetition_penalty)
        if draft_ids is not None:
            m.draft_stats = {}
            outs = decode_rows_drafted(m.engine, kv, branches, max_new, eos, repetition_penalty, [draft_ids] * len(branches), stats=m.draft_stats)
        else:
            outs = decode_rows(m.engine, kv, branches, max_new, eos, repetition_penalty)
        return [reply_text(self.tokenizer, o, template.sep) for o in outs]

    @torch.no_grad()
    def score(self, question, answers, repetition_penalty=1.5, history=None, top_logprobs=1, score_eos=True, generation_config=None, draft=None):
        """What the model thinks of each of `answers` (strings or id lists; at most max_branches) as the reply to `question` on this page: the prompt is
        chat_ocr's, every candidate gets a branch forked off the trunk at the prefix the prompt shares with it (cr_kv_fork), and ONE cr_llm_score_batch
        scores all candidates -- the prompt's tail, the answer's ids and the end-of-turn id (score_eos).  Returns one scores.ResponseScores per candidate,
        as chat_ocr(return_scores=top_logprobs) reports a reply it generated, with total_logprob for ranking.  The trunk is not changed."""
        gc = scoring.refuse_generation(generation_config, draft, 'PageSession.score')
        top_n, penalty = scoring.top_n_of(top_logprobs), scoring.check_penalty(repetition_penalty)
        answers = list(answers)
        if not 1 <= len(answers) <= self.max_branches:
            raise ValueError(f'score: {len(answers)} answers for a session opened with max_branches={self.max_branches}')
        m, kv = self.m, self.kv
        _, _, _, ids, gc = self._prompt(question, None if history is None else list(history), gc)
        plans = [scoring.plan(len(ids), scoring.answer_to_ids(self.tokenizer, a), gc['eos_token_id'], score_eos, getattr(getattr(m, 'dims', None), 'vocab', None))
                 for a in answers]
        for pl in plans:
            scoring.check_fits(len(ids) + len(pl.feed), 0, m.max_tokens)
        p = plan_prefix(self.cached_ids, ids)
        branches = list(range(1, 1 + len(plans)))
        if p > 0:
            kv.fork(0, branches, p)
        else:
            for b in branches:
                kv.truncate(b, 0)
        tail = self._embed(ids, p)
        rows = [torch.cat([tail, m.engine.embed_splice(torch.tensor(pl.feed, dtype=torch.long))], dim=0) if pl.feed else tail for pl in plans]
        self.rows_prefilled.append(sum(r.shape[0] for r in rows))
        ts = m.engine.score_batch(kv, branches, rows, [pl.targets[p:] for pl in plans], penalty=penalty, top_n=top_n)
        return [scoring.response_scores(self.tokenizer, pl.ids, t) for pl, t in zip(plans, ts)]

    @torch.no_grad()
    def ground(self, question, answer=None, layers=None, repetition_penalty=1.5, history=None, top_logprobs=None, score_eos=True, generation_config=None,
               draft=None):
        """Which character box every id of the reply to `question` came from (model.ground_ocr's meaning), on a BRANCH forked off the trunk at the prefix the
        prompt shares with it: the trunk is not changed.  answer (a string or a list of ids): the text to ground.  answer=None: the branch generates the
        reply greedily first, is rolled back to the prompt's last row and grounds the generated ids by one continued prefill.  Returns (response,
        grounding.Grounding); the Grounding carries the page's boxes when the session was opened with boxes=."""
        gc = scoring.refuse_generation(generation_config, draft, 'PageSession.ground')
        penalty = scoring.check_penalty(repetition_penalty)
        top_n = None if top_logprobs is None else scoring.top_n_of(top_logprobs)
        if not self.use_p:
            raise ValueError('PageSession.ground: the session was opened with use_p=False (no pseudo-tokens to ground on)')
        m, kv, b = self.m, self.kv, 1
        _, _, template, ids, gc = self._prompt(question, None if history is None else list(history), gc)
        spans = grounding.check_spans(grounding.spans_of(ids, m.aligned_token_id, self.per_box))
        if self.boxes is not None and len(self.boxes) != len(spans):
            raise ValueError(f'PageSession.ground: the prompt holds the pseudo-tokens of {len(spans)} boxes, the page has {len(self.boxes)}')
        n_layers = getattr(getattr(m, 'dims', None), 'llm_layers', None)
        if layers is not None and n_layers is not None:
            layers = grounding.check_layers(layers, n_layers)
        L = len(ids)
        p = plan_prefix(self.cached_ids, ids)
        if answer is not None:
            pl = scoring.plan(L, scoring.answer_to_ids(self.tokenizer, answer), gc['eos_token_id'], score_eos, getattr(getattr(m, 'dims', None), 'vocab', None))
            y = pl.ids
            scoring.check_fits(L + len(pl.feed), 0, m.max_tokens)
        else:
            max_new, eos, _ = m._gen_args(gc)
            check_fits(L, max_new, m.max_tokens)
        if p > 0:
            kv.fork(0, [b], p)
        else:
            kv.truncate(b, 0)
        tail = self._embed(ids, p)
        if answer is None:
            self.rows_prefilled.append(L - p)
            y = m._generate(tail, max_new, eos, penalty, kv=kv, seq=b, reset=False)[0].tolist()
            kv.truncate(b, L - 1)
            p, tail = L - 1, tail[L - 1 - p:]
            response = reply_text(self.tokenizer, y, template.sep)
        else:
            response = answer if isinstance(answer, str) else reply_text(self.tokenizer, y, template.sep)
        rows = torch.cat([tail, m.engine.embed_splice(torch.tensor(y[:-1], dtype=torch.long))], dim=0) if len(y) > 1 else tail
        self.rows_prefilled.append(rows.shape[0])
        tss, ms = m.engine.ground_batch(kv, [b], [rows], [[-1] * (L - 1 - p) + list(y)], [spans], layers=layers, penalty=penalty, top_n=top_n or 0,
                                        want_scores=top_n is not None)
        sc = scoring.response_scores(self.tokenizer, y, tss[0]) if tss[0] is not None else None
        return response, grounding.Grounding.build(y, ms[0].numpy(), spans, grounding.pieces_of(self.tokenizer, y), self.boxes,
                                                   layers if layers is not None else (0, n_layers or 0), grounding.special_ids_of(self.tokenizer), sc)

"""Continuous batching of pages: a fixed set of decode rows kept full, a finished page's row refilled at once.

PagePipeline (pipeline.py) decodes in batches: a batch runs until its longest page stops, and the slots of pages that stopped
earlier stay empty until then.  ContinuousPipeline keeps up to `slots` pages decoding at every step.  It stops them on the device and reads
the stops without a stream drain:
  - the greedy pick checks each row's stop criteria (cr_kv_set_stop: EOS id, budget of new ids), records the stop count and pushes the
    sequence onto the cache's finished queue once;
  - after every step the decode thread enqueues an asynchronous copy of that queue (cr_kv_poll_finished) into pinned memory and reads it
    once the copy's event has completed; ids past a stop are speculative and are cut at the stop count.

Threads and streams, as in PagePipeline:
  - the CALLER's thread prefills waiting pages into free KV sequences on its own stream (generation.admit), in groups of up to `admit_group` pages (wide
    prefill GEMMs; a partial group once input has run out, i.e. while results() drains), and reads finished pages' ids back;
  - a WORKER thread decodes on a side stream through a second context that shares the weights (Engine.shared_context).

The cache holds `slots + spare` sequences: the next pages are prefilled into spare sequences while the current rows decode, and join the
decode as rows free up.  A sequence is reset for a new page only after the decode step that last included it (its release event), and a
page joins the decode only after its prefill (its ready event); all stop-queue writes happen on the side stream, so every poll is consistent.
Per page the ids are those of its own generate_pages([page], max_new_tokens=budget) call: the same kernels, and a row's result does not
depend on the other rows of its steps.

    pipe = ContinuousPipeline(model, slots=64, max_new_tokens=1024, eos_token_id=eos, repetition_penalty=1.5)
    t = pipe.submit(embeds, max_new_tokens=None)       # any number of pages; each gets a ticket (sampling=, seed=: a sampled page)
    done = pipe.ready()                                 # [(ticket, ids)] finished so far, without waiting
    for ticket, ids in pipe.results(): ...              # the rest, in the order they finish
    pipe.close()

Token scores (scores.py): submit(..., logprobs=n) with n in 1..8 switches the page's scores on (cr_kv_set_logprobs after its sequence's reset, before
its prefill); its result is then (ticket, (ids, TokenScores)) instead of (ticket, ids), the scores read where the ids are read, on the read-back
stream, and cut at the same stop count.  Pages submitted with logprobs=0 (the default) are returned exactly as before.
"""
import collections
import threading
import time

import torch

from .config import EOS_TOKEN_ID
from .generation import admit, check_fits
from .scores import TokenScores, check_top_n


class _TorchOps:
    """Streams, events and pinned buffers of the HIP runtime through PyTorch-ROCm (the pipeline's only device plumbing besides the engine)."""

    def __init__(self, device):
        self.device = device

    def set_device(self):
        torch.cuda.set_device(self.device)

    def stream(self, priority=0):
        return torch.cuda.Stream(device=self.device, priority=priority)

    def use(self, stream):
        return torch.cuda.stream(stream)

    def current(self):
        return torch.cuda.current_stream(self.device)

    def record(self, stream):
        e = torch.cuda.Event()
        e.record(stream)
        return e

    def wait(self, stream, event):
        stream.wait_event(event)

    def done(self, event):
        return event.query()

    def sync(self, event):
        event.synchronize()

    def sync_stream(self, stream):
        stream.synchronize()

    def buffer(self, n):
        return torch.zeros(n, dtype=torch.int32).pin_memory()


class ContinuousPipeline:
    """See the module docstring.  `slots`: most rows per decode step (the batched decode kernels take <= 64); `spare`: extra KV sequences
    prefilled ahead (default `slots`: the memory of PagePipeline's two caches); `poll_depth`: decode steps the worker may run ahead of the
    last poll it has read (bounds both the host's lead over the GPU and the speculative steps of a row after its EOS)."""

    def __init__(self, model, slots=64, max_new_tokens=1024, eos_token_id=EOS_TOKEN_ID, repetition_penalty=1.0, admit_group=16, spare=None,
                 poll_depth=3, ops=None):
        if slots < 1 or admit_group < 1 or poll_depth < 1:
            raise ValueError('slots, admit_group and poll_depth must be >= 1')
        if not 1 <= max_new_tokens <= model.max_tokens:
            raise ValueError(f'max_new_tokens={max_new_tokens}: 1 .. {model.max_tokens} (the cache holds max_tokens tokens per sequence, prompt included)')
        self.m, self.eng = model, model.engine
        self.ops = ops or _TorchOps(model.device)
        self.slots, self.admit_group, self.poll_depth = slots, admit_group, poll_depth
        self.max_new_tokens, self.eos, self.penalty = max_new_tokens, eos_token_id, repetition_penalty
        self.n_seqs = slots + (slots if spare is None else spare)
        self.max_tokens = model.max_tokens
        kv_dtype = getattr(model, 'kv_cache_dtype', 'bf16')      # the model's cache format (InternVLChatModel.kv_cache_dtype)
        self.kv = self.eng.kv_alloc(self.n_seqs, self.max_tokens) if kv_dtype == 'bf16' else self.eng.kv_alloc(self.n_seqs, self.max_tokens, dtype=kv_dtype)
        self.closed = False
        if getattr(model, '_pipes', None) is not None:
            model._pipes.add(self)                        # the model refuses a kv_cache_dtype change while this is open
        self.kv.reset()
        self.dec = self.eng.shared_context()
        self.side = self.ops.stream(priority=-1)          # another priority level also lands on another hardware queue than the caller's
        self.rb = self.ops.stream()                       # id read-back: synchronising it waits for nothing but a release event and a copy
        self.stats = dict(decode_steps=0, row_steps=0, speculative_row_steps=0, admissions=0, pages_admitted=0, polls=0,
                          decode_host_s=0.0, caller_host_s=0.0)
        # caller-side state
        self.waiting = collections.deque()                # (ticket, embeds, budget) not yet prefilled
        self.free = collections.deque(range(self.n_seqs))
        self.owner = {}                                   # sequence -> ticket of the page in it
        self.scored = {}                                  # sequence -> alternatives per id, for the pages that asked for token scores
        self.to_read = collections.deque()                # (sequence, stop count, release event) handed back by the worker
        self.finished = collections.deque()               # (ticket, ids) not yet handed to the caller
        self.outstanding = 0                              # submitted, not yet handed to the caller
        self.next_ticket = 0
        # shared with the worker (under self.cv)
        self.cv = threading.Condition()
        self.inbox = collections.deque()                  # [(sequences, budgets, ready event)] prefilled groups
        self.released = collections.deque()               # (sequence, stop count, release event)
        self.error = None
        self.closing = False
        self.worker = threading.Thread(target=self._worker, daemon=True)
        self.worker.start()

    # ---- caller side ----------------------------------------------------------------------------
    def submit(self, embeds, max_new_tokens=None, sampling=None, seed=None, logprobs=0, constraints=None, draft_ids=None, num_return_sequences=1):
        """Queue one page's prompt embeddings ([S, hidden] on the device) with its budget of new ids (default, and at most, the pipeline's);
        returns its ticket.  Prefills a group when one is complete.  ValueError for a budget the pipeline cannot take.  sampling (a
        sampling.SamplingParams) with a 64-bit `seed`: the page samples (its sequence's state is set after its reset, before its prefill);
        None: greedy.  logprobs: 0, or the number of alternatives (1..8) to record per generated id: the page's result is (ids, TokenScores).
        constraints (a constraints.Constraints, greedy pages only): installed after the sequence's reset, before its prefill."""
        if draft_ids is not None:
            from .draft import refuse
            refuse('ContinuousPipeline (its rows stop on the device, its worker never waits for a step)')
        if num_return_sequences not in (1, None):
            raise NotImplementedError(f'num_return_sequences={num_return_sequences}: ContinuousPipeline owns its cache, one decode slot per page (several '
                                      'sampled answers per page: generate_pages / chat_ocr_pages)')
        t0 = time.perf_counter()
        self._raise_worker_error()
        logprobs = check_top_n(logprobs, 'logprobs', allow_zero=True)
        budget = self.max_new_tokens if max_new_tokens is None else int(max_new_tokens)
        S = int(embeds.shape[0])
        if not 1 <= budget <= self.max_new_tokens:
            raise ValueError(f'max_new_tokens={budget}: a page budget must be 1 .. {self.max_new_tokens} (the pipeline\'s)')
        check_fits(S, budget, self.max_tokens)
        ticket = self.next_ticket
        self.next_ticket += 1
        if sampling is not None and seed is None:
            raise ValueError('a sampled page needs its seed')
        if constraints is not None and sampling is not None:
            raise NotImplementedError('logits constraints on a sampled page are not implemented (greedy decoding only)')
        if constraints is not None and not constraints.active:
            constraints = None
        self.waiting.append((ticket, embeds, budget, sampling, seed, logprobs, constraints))
        self.outstanding += 1
        self._pump(flush=False, block=False)
        self.stats['caller_host_s'] += time.perf_counter() - t0
        return ticket

    def ready(self):
        """[(ticket, ids)] of the pages finished since the last call, without waiting for any."""
        t0 = time.perf_counter()
        self._pump(flush=False, block=False)
        out = list(self.finished)
        self.finished.clear()
        self.outstanding -= len(out)
        self.stats['caller_host_s'] += time.perf_counter() - t0
        return out

    def results(self):
        """Yield (ticket, ids) for every page submitted and not yet returned, in the order they finish; partial groups are admitted now."""
        while self.outstanding > 0:
            t0 = time.perf_counter()
            self._pump(flush=True, block=not self.finished)
            self.stats['caller_host_s'] += time.perf_counter() - t0
            while self.finished:
                item = self.finished.popleft()
                self.outstanding -= 1
                yield item

    def map(self, items, errors='raise'):
        """items: an iterable of (key, embeds, budget or None[, sampling, seed[, logprobs[, constraints]]]), consumed as pages are admitted (a generator can compute the next pages' embeddings
        meanwhile); yields (key, ids) as pages finish.  errors='return': a page whose budget the pipeline refuses yields (key, that ValueError) and
        the others run; 'raise': the ValueError propagates."""
        keys = {}
        for key, emb, budget, *samp in items:
            try:
                keys[self.submit(emb, budget, *samp)] = key
            except ValueError as e:
                if errors != 'return':
                    raise
                yield key, e
            for t, ids in self.ready():
                yield keys.pop(t), ids
        for t, ids in self.results():
            yield keys.pop(t), ids

    def _raise_worker_error(self):
        if self.error is not None:
            raise self.error

    def _pump(self, flush, block):
        """Read back finished pages, then prefill waiting pages into the sequences that freed.  block: until at least one more page has finished."""
        n0 = len(self.finished)
        while True:
            with self.cv:
                self.to_read.extend(self.released)
                self.released.clear()
            self._raise_worker_error()
            self._read_back(False)
            self._admit(flush)
            if not block or len(self.finished) > n0:
                return
            if self.to_read:
                self._read_back(True)                     # the oldest released page: wait for its last step
                continue
            with self.cv:
                while not self.released and self.error is None:
                    self.cv.wait()

    def _read_back(self, block):
        """ids of released sequences whose last step has run (their release event), cut at the stop count; each sequence is free again after."""
        while self.to_read:
            seq, stop, ev = self.to_read[0]
            if not self.ops.done(ev) and not block:
                return
            self.to_read.popleft()
            with self.ops.use(self.rb):
                self.ops.wait(self.rb, ev)
                ids = self.kv.generated(seq, stop)        # synchronises the read-back stream only: the event and this copy
                ts = TokenScores(*self.kv.logprobs(seq, stop)) if self.scored.pop(seq, 0) else None
            if len(ids) != stop or (ts is not None and len(ts) != stop):
                raise RuntimeError(f'sequence {seq}: {len(ids)} ids read back, stop count {stop}')
            self.finished.append((self.owner.pop(seq), ids if ts is None else (ids, ts)))
            self.free.append(seq)                         # its last decode step has completed: a reset on any stream comes after it
            block = False

    def _admit(self, flush):
        want = min(self.admit_group, self.n_seqs)
        while self.waiting and self.free:
            k = min(len(self.waiting), len(self.free), self.admit_group)
            if k < want and not flush:
                return
            group = [self.waiting.popleft() for _ in range(k)]
            seqs = [self.free.popleft() for _ in range(k)]
            self.scored.update((s, g[5]) for s, g in zip(seqs, group) if g[5])
            admit(self.eng, self.kv, seqs, [g[1] for g in group], self.penalty, per_page=[None if g[3] is None else (g[3], g[4]) for g in group],
                  lpn=[g[5] for g in group], prefill_batch=k, reset_each=True, constraints=[g[6] for g in group])
            ready = self.ops.record(self.ops.current())
            for s, (ticket, *_) in zip(seqs, group):
                self.owner[s] = ticket
            self.stats['admissions'] += 1
            self.stats['pages_admitted'] += k
            with self.cv:
                self.inbox.append((seqs, [g[2] for g in group], ready))
                self.cv.notify_all()

    # ---- decode thread --------------------------------------------------------------------------
    def _worker(self):
        try:
            self.ops.set_device()
            with self.ops.use(self.side):
                self._decode_loop()
        except BaseException as e:                                         # hand the failure to the caller's thread
            with self.cv:
                self.error = e
                self.cv.notify_all()

    def _decode_loop(self):
        n = self.n_seqs
        pending = collections.deque()              # admitted, waiting for a decode row
        live = []                                  # decode rows, in admission order
        count, budget, included = {}, {}, {}       # per sequence: ids generated (host's count), budget, decode steps that included it
        polls = collections.deque()                # (buffer, event) enqueued, not read yet
        spare_bufs = [self.ops.buffer(1 + 2 * n) for _ in range(self.poll_depth + 1)]
        seen = 0                                   # entries of the finished queue consumed
        while True:
            with self.cv:
                while not self.closing and not self.inbox and not pending and not live and not polls:
                    self.cv.wait()
                if self.closing:
                    return
                groups = list(self.inbox)
                self.inbox.clear()
            t0 = time.perf_counter()
            for seqs, budgets, ready in groups:
                self.ops.wait(self.side, ready)                           # the prefill that filled these sequences, on the caller's stream
                for s, b in zip(seqs, budgets):
                    self.kv.set_stop(s, self.eos, b)                       # on the side stream: every push onto the queue is ordered before the polls
                    count[s], budget[s], included[s] = 1, b, 0
                    pending.append(s)
            while pending and len(live) < self.slots:
                live.append(pending.popleft())
            rows = [s for s in live if count[s] < budget[s]]               # a row at its budget has stopped: the device pushes it, nothing to run
            idle = not rows
            if rows:
                self.dec.decode(self.kv, rows, penalty=self.penalty)
                for s in rows:
                    count[s] += 1
                    included[s] += 1
                self.stats['decode_steps'] += 1
                self.stats['row_steps'] += len(rows)
            buf = spare_bufs.pop()
            self.kv.poll_finished(buf)
            polls.append((buf, self.ops.record(self.side)))
            self.stats['polls'] += 1
            self.stats['decode_host_s'] += time.perf_counter() - t0
            # read every poll that has landed; wait for the oldest when the host is poll_depth steps ahead, or when there is nothing to run
            while polls and (self.ops.done(polls[0][1]) or len(polls) > self.poll_depth or idle):
                buf, ev = polls.popleft()
                self.ops.sync(ev)
                h = buf.tolist()
                spare_bufs.append(buf)
                gone = []
                for k in range(seen, h[0]):
                    s = h[1 + k % n]
                    stop = h[1 + n + s]
                    if s not in count or stop <= 0:
                        raise RuntimeError(f'finished queue entry {k}: sequence {s} (stop count {stop}) is not decoding here')
                    gone.append((s, stop))
                seen = max(seen, h[0])
                if gone:
                    for s, stop in gone:
                        if s in live:
                            live.remove(s)
                        else:
                            pending.remove(s)
                        self.stats['speculative_row_steps'] += included[s] - (stop - 1)
                        del count[s], budget[s], included[s]
                    rel = self.ops.record(self.side)                      # after the last step that included them
                    with self.cv:
                        self.released.extend((s, stop, rel) for s, stop in gone)
                        self.cv.notify_all()
                    idle = False                                          # rows changed: go round before waiting for another poll

    def close(self):
        """Stop the decode thread (pages still in flight are dropped) and free the cache and the second context."""
        if self.worker is not None:
            with self.cv:
                self.closing = True
                self.cv.notify_all()
            self.worker.join()
            self.worker = None
            self.ops.sync_stream(self.side)
            self.ops.sync_stream(self.ops.current())
        if self.kv is not None:
            self.kv.free()
            self.kv = None
        if self.dec is not None:
            self.dec.close()
            self.dec = None
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

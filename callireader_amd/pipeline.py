"""PagePipeline: two batches of pages in flight, the decode of one beside the visual stage and the prefill of the next (chat_ocr_stream's engine)."""
import os
import queue
import sys
import threading
import time

import torch

from .config import EOS_TOKEN_ID
from .constraints import per_page as constraints_per_page
from .generation import admit, decode_rows, per_page_sampling, read_scores
from .scores import per_page as scores_per_page


class PagePipeline:
    """Two batches of pages in flight.  The batched decode is HBM-bound (weights + KV cache streamed once per step) and leaves the
    matrix cores idle; the visual stage and the prefill of the NEXT batch are matrix-bound.  A worker thread decodes batch i-1 on
    its own HIP stream, through a second context that shares this model's weights (Engine.shared_context: own workspace, no
    copy), while the caller runs batch i's visual stage and prefill as usual.  Measured on MI355X: a 63-tile ViT chunk takes 54 ms
    instead of 50 beside a decode step that takes 26 ms instead of 11, i.e. 1.33x the work per unit time while both run.  The
    two streams have to be fed by two host threads: one thread alternating between them got a quarter of that (scripts/overlap_probe.py).
    Per page the ids are those of generate_pages (same kernels, same order per page; the same admission and decode loop: generation.py).

        pipe = model.page_pipeline(max_new_tokens=..., eos_token_id=...)
        for batch in batches:
            embeds = ... visual stage of `batch`, as for generate_pages ...
            outs_prev = pipe.start(embeds)                 # prefill; returns the PREVIOUS batch's ids (None the first time)
        outs_last = pipe.finish()
        pipe.close()

    The two KV caches alternate between batches."""

    def __init__(self, model, max_new_tokens=1024, eos_token_id=EOS_TOKEN_ID, repetition_penalty=1.0, check_every=16, prefill_batch=16):
        self.m, self.eng = model, model.engine
        self.closed = False
        model._pipes.add(self)                        # the model refuses a kv_cache_dtype change while this is open
        self.max_new_tokens, self.eos, self.penalty = max_new_tokens, eos_token_id, repetition_penalty
        self.check_every, self.prefill_batch = int(os.environ.get('CR_PIPE_CHECK_EVERY', check_every)), prefill_batch      # (env: development aid, how often the decode thread looks for EOS)
        self.dec = self.eng.shared_context()
        # a stream of another priority level also lands on another hardware queue than the caller's (two streams of one level may share one)
        self.side = torch.cuda.Stream(device=self.eng.device, priority=int(os.environ.get('CR_PIPE_PRIO', '-1')))
        self.kvs = [None, None]
        self.turn = 0
        self.jobs, self.results = queue.Queue(), queue.Queue()
        self.in_flight = 0
        self.host_s, self.host_steps = 0.0, 0         # host time the decode thread spent issuing steps (diagnostic)
        self.row_steps = 0                            # decode rows summed over those steps (diagnostic)
        self.worker = threading.Thread(target=self._decode_loop, daemon=True)
        self.worker.start()

    def _kv(self, slot, P):
        kv = self.kvs[slot]
        if kv is None or kv.n_seqs < P:
            if kv is not None:
                kv.free()
            kv = self.kvs[slot] = self.m._kv_alloc(max(P, self.m.max_pages), self.m.max_tokens)
        return kv

    def _decode_loop(self):
        torch.cuda.set_device(self.eng.device)
        while True:
            job = self.jobs.get()
            if job is None:
                return
            kv, P, ready, budgets, lpn = job
            try:
                with torch.cuda.stream(self.side):
                    self.side.wait_event(ready)                        # the prefill that filled this cache, on the caller's stream
                    span = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)] if os.environ.get('CR_PIPE_MARKS') else None
                    if span:
                        span[0].record(self.side)
                        span[1].record(self.side)
                        t_first = t_issued = time.perf_counter()

                    def count(steps, rows, seconds):
                        nonlocal t_issued
                        self.host_s += seconds
                        self.host_steps += steps
                        self.row_steps += steps * rows
                        if span:                                       # behind the last chunk these hold the end of the batch's decode
                            span[1].record(self.side)
                            t_issued = time.perf_counter()
                    outs = decode_rows(self.dec, kv, list(range(P)), self.max_new_tokens, self.eos, self.penalty, self.check_every, budgets,
                                       on_chunk=count)               # a look synchronises the side stream only
                    if span:
                        span[1].synchronize()
                        print(f'[marks] decode of a batch: {span[0].elapsed_time(span[1]):.0f} ms on the GPU, all steps issued after {1e3 * (t_issued - t_first):.0f} ms of host time',
                              file=sys.stderr, flush=True)
                    if any(lpn):
                        outs = (outs, read_scores(kv, lpn, outs))
                self.results.put(outs)
            except BaseException as e:                                 # hand the failure to the caller's thread
                self.results.put(e)

    def _collect(self):
        if not self.in_flight:
            return None
        self.in_flight -= 1
        out = self.results.get()
        if isinstance(out, BaseException):
            raise out
        return out

    def start(self, embeds_list, budgets=None, sampling=None, seeds=None, logprobs=0, constraints=None, num_return_sequences=1):
        """Prefill a batch on the caller's stream and hand it to the decode thread; returns the previous batch's ids (None if there
        was none), waiting for them if they are not there yet.  budgets: optional per-page max_new_tokens (<= the pipeline's): a page
        leaves the batch at the first EOS check at or past its budget and its ids are cut there, as its own generate_pages call would.
        sampling / seeds / logprobs: as generate_pages takes them; a batch started with a non-zero logprobs is returned as (ids, scores).
        constraints: None, one constraints.Constraints for every page, or a list with one (or None) per page."""
        if num_return_sequences not in (1, None):
            raise NotImplementedError(f'num_return_sequences={num_return_sequences}: PagePipeline owns its two caches, one sequence per page (several sampled '
                                      'answers per page: generate_pages / chat_ocr_pages)')
        P = len(embeds_list)
        per_page = per_page_sampling(sampling, seeds, P)
        lpn = scores_per_page(logprobs, P)
        # The OTHER slot may be under the worker's decode right now (the previous batch, not collected yet): it is only ever
        # CREATED here, on the first batch (28 GB at 64 pages: not inside a later step), never regrown -- a batch larger than it
        # holds regrows it when that slot's turn comes, i.e. after _collect() has returned the batch that last used it.
        if self.kvs[self.turn ^ 1] is None:
            self._kv(self.turn ^ 1, P)
        kv = self._kv(self.turn, P)                # last used two batches ago, and that batch has been collected
        self.turn ^= 1
        admit(self.eng, kv, list(range(P)), embeds_list, self.penalty, per_page, lpn, self.prefill_batch, constraints=constraints_per_page(constraints, P))
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        prev = self._collect()
        self.jobs.put((kv, P, ready, None if budgets is None else [min(int(b), self.max_new_tokens) for b in budgets], lpn))
        self.in_flight += 1
        return prev

    def finish(self):
        return self._collect()

    def close(self):
        if self.worker is not None:
            while self.in_flight:
                self._collect()
            self.jobs.put(None)
            self.worker.join()
            self.worker = None
        for kv in self.kvs:
            if kv is not None:
                kv.free()
        self.kvs = [None, None]
        if self.dec is not None:
            self.dec.close()
            self.dec = None
        self.closed = True

"""ContinuousPipeline's scheduling on the CPU (callireader_amd/continuous.py): a fake engine with the device semantics of cr_kv_set_stop /
cr_kv_poll_finished and of the greedy decode (one id per row and step, ids past a stop are kept), and synchronous fake streams."""
import contextlib
import random
import threading
import time

import pytest
import torch

from callireader_amd.continuous import ContinuousPipeline


class Page:
    """A prompt of S rows whose greedy stream is a fixed function of its seed."""

    def __init__(self, seed, S=10):
        self.seed, self.shape = seed, (S, 4096)

    def id_at(self, k):
        return (self.seed * 7919 + k * 104729) % 50 + 1


def reference(page, budget, eos):
    ids = [page.id_at(k) for k in range(budget)]
    return ids[:ids.index(eos) + 1] if eos is not None and eos in ids else ids


class FakeKV:
    def __init__(self, n_seqs, max_tokens):
        self.n_seqs, self.max_tokens = n_seqs, max_tokens
        self.lock = threading.Lock()
        self.freed = False
        self.reset()

    def reset(self, seq=-1):
        with self.lock:
            if seq < 0:
                self.page, self.ids, self.len = {}, {}, {}
                self.eos, self.budget, self.stop = {}, {}, {}
                self.count, self.ring = 0, [0] * self.n_seqs
            for s in (range(self.n_seqs) if seq < 0 else [seq]):
                self.page[s], self.ids[s], self.len[s] = None, [], 0
                self.eos[s], self.budget[s], self.stop[s] = -1, 0, 0

    def length(self, seq):
        return self.len[seq]

    def _check(self, s):                      # pick_kernel's stop_check
        n = len(self.ids[s])
        if self.stop[s] == 0 and ((self.eos[s] >= 0 and self.ids[s][-1] == self.eos[s]) or (self.budget[s] > 0 and n >= self.budget[s])):
            self.stop[s] = n
            self.ring[self.count % self.n_seqs] = s
            self.count += 1

    def append(self, s):
        with self.lock:
            assert self.len[s] + 1 <= self.max_tokens
            self.ids[s].append(self.page[s].id_at(len(self.ids[s])))
            self.len[s] += 1
            self._check(s)

    def set_stop(self, seq, eos_id=None, max_new=0):
        with self.lock:
            if max_new > self.max_tokens - self.len[seq]:
                raise RuntimeError('budget exceeds the cache')
            self.eos[seq], self.budget[seq] = (-1 if eos_id is None else eos_id), max_new
            if self.stop[seq] == 0:
                ids = self.ids[seq]
                at = ids.index(self.eos[seq]) + 1 if self.eos[seq] in ids else 0
                if max_new > 0 and len(ids) >= max_new and (at == 0 or at > max_new):
                    at = max_new
                if at:
                    self.stop[seq] = at
                    self.ring[self.count % self.n_seqs] = seq
                    self.count += 1

    def poll_finished(self, out):
        with self.lock:
            n = self.n_seqs
            out[0] = self.count
            out[1:1 + n] = torch.tensor(self.ring, dtype=torch.int32)
            out[1 + n:1 + 2 * n] = torch.tensor([self.stop[s] for s in range(n)], dtype=torch.int32)

    def generated(self, seq, max_tokens=4096):
        with self.lock:
            return list(self.ids[seq][:max_tokens])

    def free(self):
        self.freed = True


class FakeDecoder:
    def __init__(self, eng):
        self.eng, self.closed = eng, False

    def decode(self, kv, seqs, penalty=1.0):
        e = self.eng
        e.decode_calls += 1
        if e.fail_at is not None and e.decode_calls >= e.fail_at:
            raise RuntimeError('decode failed on purpose')
        assert len(seqs) == len(set(seqs)) and len(seqs) <= e.max_rows
        e.rows_seen = max(e.rows_seen, len(seqs))
        for s in seqs:
            assert kv.page[s] is not None and kv.ids[s], f'sequence {s} decoded without a prefill'
            kv.append(s)
        if e.step_sleep:
            time.sleep(e.step_sleep)

    def close(self):
        self.closed = True


class FakeEngine:
    def __init__(self, max_rows, fail_at=None, step_sleep=0.0):
        self.max_rows, self.fail_at, self.step_sleep = max_rows, fail_at, step_sleep
        self.decode_calls, self.rows_seen = 0, 0
        self.prefills = []                    # [(sequences, pages)] in call order
        self.kvs, self.decoders = [], []

    def kv_alloc(self, n_seqs, max_tokens):
        kv = FakeKV(n_seqs, max_tokens)
        self.kvs.append(kv)
        return kv

    def shared_context(self):
        d = FakeDecoder(self)
        self.decoders.append(d)
        return d

    def prefill_batch(self, kv, seqs, embeds, penalty=1.0):
        self.prefills.append((list(seqs), list(embeds)))
        for s, p in zip(seqs, embeds):
            assert kv.page[s] is None and not kv.ids[s], f'sequence {s} prefilled without a reset'
            kv.page[s] = p
            kv.len[s] = p.shape[0]
            kv.append(s)


class FakeModel:
    def __init__(self, max_rows, max_tokens=200, **kw):
        self.engine, self.max_tokens, self.device = FakeEngine(max_rows, **kw), max_tokens, None


class FakeOps:
    class Event:
        pass

    def set_device(self):
        pass

    def stream(self, priority=0):
        return object()

    def use(self, stream):
        return contextlib.nullcontext()

    def current(self):
        return None

    def record(self, stream):
        return FakeOps.Event()

    def wait(self, stream, event):
        pass

    def done(self, event):
        return True

    def sync(self, event):
        pass

    def sync_stream(self, stream):
        pass

    def buffer(self, n):
        return torch.zeros(n, dtype=torch.int32)


def pipeline(slots=3, max_rows=None, **kw):
    fk = {k: kw.pop(k) for k in ('fail_at', 'step_sleep') if k in kw}
    m = FakeModel(max_rows or slots, **fk)
    return m, ContinuousPipeline(m, slots=slots, ops=FakeOps(), **kw)


def test_admission_in_submission_order_and_groups():
    m, pipe = pipeline(slots=2, spare=4, admit_group=3, max_new_tokens=30, eos_token_id=None)
    pages = [Page(i) for i in range(7)]
    tickets = [pipe.submit(p) for p in pages]
    pre = m.engine.prefills
    assert [len(s) for s, _ in pre] == [3, 3]              # a full group each; the seventh page waits for a group or for the input to end
    got = dict(pipe.ready())
    got.update(pipe.results())
    pipe.close()
    order = [p for _, ps in pre for p in ps]
    assert order == pages                                  # first come, first prefilled
    assert all(len(s) <= 3 for s, _ in pre) and sum(len(s) for s, _ in pre) == 7
    assert m.engine.rows_seen <= 2
    assert [got[t] for t in tickets] == [reference(p, 30, None) for p in pages]
    assert pipe.stats['pages_admitted'] == 7 and pipe.stats['admissions'] == len(pre)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_every_ticket_returned_exactly_once_with_its_own_ids(seed):
    rng = random.Random(seed)
    eos = 17
    m, pipe = pipeline(slots=4, admit_group=3, max_new_tokens=40, eos_token_id=eos, poll_depth=2)
    pages = [Page(rng.randrange(1000), S=rng.randrange(5, 60)) for _ in range(40)]
    budgets = [rng.choice([None, 1, 2, 5, 17, 40]) for _ in pages]
    seen = []
    keys = {}
    for p, b in zip(pages, budgets):
        keys[pipe.submit(p, max_new_tokens=b)] = (p, b)
        seen += pipe.ready()
    seen += list(pipe.results())
    stats = dict(pipe.stats)
    pipe.close()
    assert sorted(t for t, _ in seen) == sorted(keys)      # each ticket once
    for t, ids in seen:
        p, b = keys[t]
        assert ids == reference(p, b or 40, eos), t
    assert m.engine.rows_seen <= 4
    assert stats['row_steps'] == sum(len(ids) - 1 for _, ids in seen) + stats['speculative_row_steps']
    assert list(pipe.results()) == []


def test_budget_validation_fails_only_the_offending_page():
    m, pipe = pipeline(slots=2, max_new_tokens=20, eos_token_id=None)
    with pytest.raises(ValueError):
        pipe.submit(Page(1), max_new_tokens=21)           # above the pipeline's
    with pytest.raises(ValueError):
        pipe.submit(Page(1), max_new_tokens=0)
    with pytest.raises(ValueError):
        pipe.submit(Page(1, S=190), max_new_tokens=20)    # prompt + budget past max_tokens (200)
    items = [('a', Page(1), None), ('b', Page(2), 50), ('c', Page(3, S=195), 10), ('d', Page(4), 3)]
    out = dict(pipe.map(iter(items), errors='return'))
    pipe.close()
    assert set(out) == {'a', 'b', 'c', 'd'}
    assert isinstance(out['b'], ValueError) and isinstance(out['c'], ValueError)
    assert out['a'] == reference(Page(1), 20, None) and out['d'] == reference(Page(4), 3, None)
    m, pipe = pipeline(slots=2, max_new_tokens=20, eos_token_id=None)
    with pytest.raises(ValueError):
        list(pipe.map(iter(items), errors='raise'))
    pipe.close()


def test_worker_exception_reaches_the_caller():
    m, pipe = pipeline(slots=2, max_new_tokens=50, eos_token_id=None, fail_at=5)
    for i in range(4):
        pipe.submit(Page(i))
    with pytest.raises(RuntimeError, match='on purpose'):
        list(pipe.results())
    with pytest.raises(RuntimeError, match='on purpose'):
        pipe.submit(Page(9))
    pipe.close()
    assert m.engine.kvs[0].freed and m.engine.decoders[0].closed


def test_close_with_work_in_flight():
    m, pipe = pipeline(slots=2, spare=2, admit_group=1, max_new_tokens=200, eos_token_id=None, step_sleep=0.002)
    pages = [Page(i, S=5) for i in range(6)]
    for p in pages:
        pipe.submit(p, max_new_tokens=150)
    time.sleep(0.02)
    t0 = time.perf_counter()
    pipe.close()
    assert time.perf_counter() - t0 < 5
    assert pipe.worker is None and m.engine.kvs[0].freed and m.engine.decoders[0].closed
    assert m.engine.decode_calls < 150                     # stopped, not run to the end
    pipe.close()                                           # a second close is harmless

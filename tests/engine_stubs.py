"""A stub engine and KV cache for host-logic tests without a GPU: they log the cache operations, `prefill`, `prefill_batch` and `decode` with
their rows, and emit scripted ids (tests/test_session_cpu.py, tests/test_generation_cpu.py)."""
import numpy as np
import torch

from chat_helpers import FakeTokenizer, SPECIALS

IMG, REF, EOS = SPECIALS['<IMG_CONTEXT>'], SPECIALS['[UNUSED_TOKEN_140]'], SPECIALS['<|im_end|>']
HID = 8


class StubKV:
    def __init__(self, n_seqs, max_tokens, log):
        self.n_seqs, self.max_tokens, self.log = n_seqs, max_tokens, log
        self.len, self.gen, self.freed = [0] * n_seqs, [[] for _ in range(n_seqs)], False

    def length(self, seq):
        return self.len[seq]

    def generated(self, seq):
        self.log.append(('generated', seq))
        return list(self.gen[seq])

    def reset(self, seq=-1):
        self.log.append(('reset', seq))
        for s in (range(self.n_seqs) if seq < 0 else [seq]):
            self.len[s], self.gen[s] = 0, []

    def truncate(self, seq, n):
        assert 0 <= n <= self.len[seq]
        self.log.append(('truncate', seq, n))
        self.len[seq], self.gen[seq] = n, []

    def fork(self, src, dsts, n):
        assert 1 <= n <= self.len[src] and src not in dsts and len(set(dsts)) == len(dsts)
        self.log.append(('fork', src, list(dsts), n))
        for d in dsts:
            self.len[d], self.gen[d] = n, []

    def set_sampling(self, seq, *a):
        self.log.append(('set_sampling', seq))

    def set_logprobs(self, seq, n):
        self.log.append(('set_logprobs', seq, n))

    def logprobs(self, seq):
        T = len(self.gen[seq])
        return np.zeros(T, np.float32), np.zeros((T, 1), np.int32), np.zeros((T, 1), np.float32)

    def free(self):
        self.freed = True


class StubEngine:
    """embed_splice returns one row per id (the id in column 0); prefill / decode advance the lengths and append the next scripted id."""

    def __init__(self):
        self.log, self.script, self.kvs = [], {}, []

    def kv_alloc(self, n_seqs, max_tokens, dtype='bf16'):
        self.kvs.append(StubKV(n_seqs, max_tokens, self.log))
        return self.kvs[-1]

    def embed_splice(self, ids, vit=None, ref=None, img_id=None, ref_id=None):
        ids = ids.reshape(-1)
        self.log.append(('embed', ids.tolist(), None if vit is None else vit[:, 0].tolist(), None if ref is None else ref[:, 0].tolist(), img_id))
        out = torch.zeros(len(ids), HID)
        out[:, 0] = ids
        return out

    def _pick(self, kv, seq):
        s = self.script.get(seq, [])
        kv.gen[seq].append(s.pop(0) if s else 77)

    def prefill(self, kv, seq, embeds, penalty=1.0):
        self.log.append(('prefill', seq, embeds[:, 0].long().tolist()))
        kv.len[seq] += embeds.shape[0]
        self._pick(kv, seq)

    def prefill_batch(self, kv, seqs, embeds_list, penalty=1.0):
        self.log.append(('prefill_batch', list(seqs), [e.shape[0] for e in embeds_list]))
        for s, e in zip(seqs, embeds_list):
            kv.len[s] += e.shape[0]
            self._pick(kv, s)

    def decode(self, kv, seqs, penalty=1.0):
        self.log.append(('decode', list(seqs)))
        for s in seqs:
            kv.len[s] += 1
            self._pick(kv, s)


def make_model(kv_cache_dtype='bf16'):
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    from callireader_amd.conversation import get_conv_template
    m = InternVLChatModel.__new__(InternVLChatModel)                  # no Engine: there is no GPU here
    m._kv_cache_dtype = kv_cache_dtype
    m.engine = StubEngine()
    m.device = torch.device('cpu')
    m.template = 'internlm2-chat'
    m.num_image_token = 4
    m.aligned_token_id = REF
    m.img_context_token_id = None
    m.conv_template = get_conv_template(m.template)
    m.system_message = m.conv_template.system_message
    m.max_tokens = 512
    m.max_pages = 1
    m._kv = None
    return m


class RoundTripTokenizer(FakeTokenizer):
    """FakeTokenizer whose decode gives back the characters it encodes: a re-tokenised answer is the generated ids."""

    def batch_decode(self, out, skip_special_tokens=True):
        return [''.join('<|im_end|>' if int(t) == EOS else chr(int(t) - 10) for t in row) for row in out]


def ids_of(text):
    return [10 + ord(c) for c in text]


N_TILES, N_REF = 2, 3


def make_session(tok=None, max_branches=1, **kw):
    from callireader_amd.session import PageSession
    m = make_model(**kw)
    vit = torch.arange(N_TILES * 4, dtype=torch.float32).reshape(N_TILES, 4, 1).expand(N_TILES, 4, HID) + 100      # row k holds 100 + k
    ref = torch.arange(N_REF, dtype=torch.float32).reshape(N_REF, 1).expand(N_REF, HID) + 200                      # row k holds 200 + k
    return PageSession(m, tok or RoundTripTokenizer(), vit, ref, N_TILES, use_p=True, max_branches=max_branches), m.engine

"""Thin torch<->C-ABI plumbing: device buffers and streams come from PyTorch-ROCm,
all compute goes through libcallireader_hip.so.  No torch math on the hot path."""
import ctypes as C

import numpy as np
import torch

from . import _binding as B
from .config import ModelDims

_DT = {torch.bfloat16: B.CR_BF16, torch.float32: B.CR_F32, torch.int64: B.CR_I64, torch.int32: B.CR_I32}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def rope_tables(dims: ModelDims, rows=None):
    """bf16 cos/sin cache exactly as InternLM2DynamicNTKScalingRotaryEmbedding builds it at init
    (reference InternVL/modeling_internlm2.py:154,213-229; returned in bf16 by :177-180).
    Host-side setup (fp32 torch on CPU, like the reference), uploaded once as weights."""
    rows = dims.max_pos if rows is None else rows
    hd = dims.llm_head_dim
    inv_freq = 1.0 / (dims.rope_theta ** (torch.arange(0, hd, 2).float() / hd))
    t = torch.arange(rows).to(inv_freq.dtype)
    freqs = torch.einsum('i,j->ij', t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)


class Engine:
    """One context per device (include/callireader_hip.h)."""

    def __init__(self, dims: ModelDims = None, device=0, max_pos=None):
        if not torch.cuda.is_available():
            raise RuntimeError('callireader_amd needs a ROCm GPU: there is no CPU fallback for the hot path')
        self.dims = dims or ModelDims.full()
        self.device = torch.device('cuda', device)
        self.max_pos = max_pos or self.dims.max_pos
        d = B.ModelDesc(vit_layers=self.dims.vit_layers, rs_depth=self.dims.rs_depth, llm_layers=self.dims.llm_layers,
                        vocab=self.dims.vocab, max_pos=self.max_pos, vit_ln_eps=self.dims.vit_ln_eps,
                        rms_eps=self.dims.rms_eps)
        h = C.c_void_p()
        torch.cuda.set_device(self.device)
        B.check(B.lib.cr_create(device, C.byref(d), C.byref(h)), 'cr_create')
        self._h = h
        self._kv = []
        self.fp8_decode, self.fp8_mfma = False, 0          # mirrors of the context's options (parallel.default_cost picks the cost table by them)
        self.weights_version = 0                           # bumped by everything after which a borrower (share_weights_from) must share again: loads, finalize, the fp8 switches

    def close(self):
        if getattr(self, '_h', None):
            B.lib.cr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ----
    def load_weight(self, name, t):
        t = t.detach().contiguous()
        if not name.startswith('orderformer.'):
            self.fp8_decode, self.fp8_mfma = False, 0      # cr_load_weight switches the options off with the copies they read
        self.weights_version += 1
        shape = (C.c_int64 * t.dim())(*t.shape)
        B.check(B.lib.cr_load_weight(self._h, name.encode(), _p(t), _DT[t.dtype], shape, t.dim(),
                                     0 if t.is_cuda else 1, _stream()), f'cr_load_weight({name})')
        if t.is_cuda:
            torch.cuda.current_stream().synchronize()   # the source may be freed by the caller right after

    def load_state_dict(self, sd):
        for k, v in (sd.items() if hasattr(sd, 'items') else sd):
            self.load_weight(k, v if v.dtype in (torch.bfloat16,) or not v.is_floating_point() else v.to(torch.bfloat16))

    def load_rope(self):
        cos, sin = rope_tables(self.dims, self.max_pos)
        self.load_weight('rope.cos', cos)
        self.load_weight('rope.sin', sin)

    def finalize(self):
        B.check(B.lib.cr_finalize(self._h, _stream()), 'cr_finalize')
        self.weights_version += 1

    def share_weights_from(self, other):
        """cr_share_weights: this (fresh) engine uses `other`'s finalized weights without copying them -- a second host thread can
        then run stages through it on its own stream while `other` keeps working (PagePipeline).  `other` must outlive it."""
        B.check(B.lib.cr_share_weights(self._h, other._h), 'cr_share_weights')
        self._shared_from = other

    def shared_context(self):
        """A fresh Engine on this device that uses this engine's finalized weights (share_weights_from): own workspace, own staging, for a second
        host thread on its own stream.  This engine must outlive it."""
        other = Engine(self.dims, device=self.device.index, max_pos=self.max_pos)
        other.share_weights_from(self)
        return other

    def enable_fp8_decode(self, on=True):
        """Batched decode streams e4m3 copies of the LLM's linear weights (one fp32 scale per output row) instead of the
        bf16 ones: half the HBM bytes per step.  Off by default: the reference computes in bf16 (include/callireader_hip.h)."""
        B.check(B.lib.cr_enable_fp8_decode(self._h, 1 if on else 0, _stream()), 'cr_enable_fp8_decode')
        self.fp8_decode = bool(on)
        self.weights_version += 1

    # ---- vision ----
    def enable_fp8_mfma(self, on=True, level=1):
        """cr_enable_fp8_mfma.  level 1: norm-fed linears (ViT QKV / fc1, mlp1[1], LLM prefill wqkv / w1|w3) multiply e4m3 x e4m3 on the
        matrix cores; level 2: also ViT fc2 and the prefill's wo / w2.  OFF by default (the reference's arithmetic is bf16); a throughput
        option whose accuracy only a real checkpoint can price (evaluate.py --compare_fp8)."""
        B.check(B.lib.cr_enable_fp8_mfma(self._h, (2 if level >= 2 else 1) if on else 0, _stream()), 'cr_enable_fp8_mfma')
        self.fp8_mfma = ((2 if level >= 2 else 1) if on else 0)
        self.weights_version += 1

    def _chk_pixels(self, px):
        if px.dim() != 4:
            raise ValueError(f'wrong pixel_values size: {px.shape}')       # modeling_intern_vit.py:417-420
        if tuple(px.shape[1:]) != (3, self.dims.image_size, self.dims.image_size):
            raise ValueError(f'pixel_values must be (T,3,448,448), got {tuple(px.shape)}')
        return px.to(self.device, torch.bfloat16).contiguous()

    def vit_forward(self, pixel_values):
        px = self._chk_pixels(pixel_values)
        T = px.shape[0]
        out = torch.empty(T, self.dims.vit_tokens, self.dims.vit_hidden, device=self.device, dtype=torch.bfloat16)
        B.check(B.lib.cr_vit_forward(self._h, _p(px), T, _p(out), _stream()), 'cr_vit_forward')
        return out

    def project(self, vit_out):
        T = vit_out.shape[0]
        vit_out = vit_out.contiguous()
        out = torch.empty(T, self.dims.tokens_per_tile, self.dims.llm_hidden, device=self.device, dtype=torch.bfloat16)
        B.check(B.lib.cr_project(self._h, _p(vit_out), T, _p(out), _stream()), 'cr_project')
        return out

    def extract_feature(self, pixel_values):
        px = self._chk_pixels(pixel_values)
        T = px.shape[0]
        out = torch.empty(T, self.dims.tokens_per_tile, self.dims.llm_hidden, device=self.device, dtype=torch.bfloat16)
        B.check(B.lib.cr_extract_feature(self._h, _p(px), T, _p(out), _stream()), 'cr_extract_feature')
        return out

    # ---- tile preprocessing on the GPU ----
    def preprocess(self, page_u8, jobs, n_tiles, out=None):
        """page_u8: uint8 (H,W,3) RGB tensor (moved to the device once); jobs: dict rows from preprocess.plan_*, or their int32 (n, 11) table
        (preprocess.jobs_array / plan_chars_array); out: the (n_tiles,3,448,448) bf16 tensor the jobs' tile0 slots index (default: a new one)."""
        import numpy as np
        from .preprocess import norm_lut, jobs_array
        if getattr(self, '_lut', None) is None:
            self._lut = norm_lut().to(self.device)
        page = page_u8.to(self.device).contiguous()
        assert page.dtype == torch.uint8 and page.dim() == 3 and page.shape[2] == 3
        tab = np.ascontiguousarray(jobs if isinstance(jobs, np.ndarray) else jobs_array(jobs), dtype=np.int32)
        assert tab.ndim == 2 and tab.shape[1] * 4 == C.sizeof(B.PrepJob)
        if out is None:
            out = torch.empty(n_tiles, 3, self.dims.image_size, self.dims.image_size, device=self.device, dtype=torch.bfloat16)
        assert out.is_contiguous() and out.shape[0] == n_tiles and out.dtype == torch.bfloat16
        B.check(B.lib.cr_preprocess(self._h, _p(page), page.shape[0], page.shape[1], tab.ctypes.data_as(C.c_void_p), tab.shape[0], _p(self._lut), _p(out),
                                    n_tiles, _stream()), 'cr_preprocess')
        return out

    # ---- CalliAlign ----
    def resample(self, feats):
        feats = feats.contiguous()
        T = feats.shape[0]
        out = torch.empty(T, self.dims.rs_queries, self.dims.llm_hidden, device=self.device, dtype=torch.bfloat16)
        B.check(B.lib.cr_resample(self._h, _p(feats), T, _p(out), _stream()), 'cr_resample')
        return out

    def orderformer(self, boxes):
        """boxes (B, L, 4) bf16 -> (B, L) fp32 scores of the OrderFormer (weights `orderformer.*` loaded beforehand)."""
        x = boxes.to(device=self.device, dtype=torch.bfloat16).contiguous()
        Bn, L, four = x.shape
        assert four == 4
        out = torch.empty(Bn, L, device=self.device, dtype=torch.float32)
        B.check(B.lib.cr_orderformer(self._h, _p(x), Bn, L, _p(out), _stream()), 'cr_orderformer')
        return out

    def vq(self, x, with_cos=False):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        n = x2.shape[0]
        idx = torch.empty(n, device=self.device, dtype=torch.int64)
        cos = torch.empty(n, device=self.device, dtype=torch.bfloat16) if with_cos else None
        B.check(B.lib.cr_vq(self._h, _p(x2), n, _p(idx), _p(cos), _stream()), 'cr_vq')
        idx = idx.reshape(x.shape[:-1])
        return (idx, cos.reshape(x.shape[:-1])) if with_cos else idx

    def denorm(self, x, idx, cos=None, drop_zero=False, hard_vq=False):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        n = x2.shape[0]
        idx1 = idx.reshape(-1).contiguous()
        out = torch.empty_like(x2)
        n_out = torch.zeros(1, device=self.device, dtype=torch.int32)
        flags = (1 if drop_zero else 0) | (2 if hard_vq else 0)
        if hard_vq and cos is None:
            raise ValueError('hard_vq needs the cosine values from vq(..., with_cos=True)')
        cosr = cos.reshape(-1).contiguous() if cos is not None else None
        B.check(B.lib.cr_denorm(self._h, _p(x2), _p(idx1), _p(cosr), n, flags, _p(out), _p(n_out), _stream()), 'cr_denorm')
        return out[:int(n_out.item())] if drop_zero else out

    # ---- language model ----
    def embed_splice(self, input_ids, vit_embeds=None, ref_embeds=None, img_id=92546, ref_id=92537):
        ids = input_ids.reshape(-1).to(self.device, torch.int64).contiguous()
        S = ids.shape[0]
        out = torch.empty(S, self.dims.llm_hidden, device=self.device, dtype=torch.bfloat16)
        v = vit_embeds.reshape(-1, self.dims.llm_hidden).contiguous() if vit_embeds is not None else None
        r = ref_embeds.reshape(-1, self.dims.llm_hidden).to(torch.bfloat16).contiguous() if ref_embeds is not None else None
        B.check(B.lib.cr_embed_splice(self._h, _p(ids), S, _p(v), 0 if v is None else v.shape[0], img_id,
                                      _p(r), 0 if r is None else r.shape[0], ref_id, _p(out), _stream()), 'cr_embed_splice')
        return out

    def kv_alloc(self, n_seqs, max_tokens, dtype='bf16'):
        """cr_kv_alloc_ex.  dtype 'bf16' (default: the reference's cache) or 'e4m3' (cr_kv_alloc_ex CR_KV_E4M3: e4m3 rows + one fp32 scale each, 0.52x
        the bytes; a throughput option, not parity-preserving -- include/callireader_hip.h)."""
        fmt = kv_format(dtype)
        h = C.c_void_p()
        B.check(B.lib.cr_kv_alloc_ex(self._h, n_seqs, max_tokens, fmt, C.byref(h)), 'cr_kv_alloc')
        return KVCache(self, h, n_seqs, max_tokens)

    def prefill(self, kv, seq, embeds, penalty=1.0, want_logits=False):
        e = embeds.reshape(-1, self.dims.llm_hidden).contiguous()
        S = e.shape[0]
        logits = torch.empty(self.dims.vocab, device=self.device, dtype=torch.float32) if want_logits else None
        B.check(B.lib.cr_llm_prefill(self._h, kv._h, seq, _p(e), S, float(penalty), _p(logits), _stream()), 'cr_llm_prefill')
        return logits

    def prefill_batch(self, kv, seqs, embeds_list, penalty=1.0, want_logits=False):
        """Prefill several sequences in one pass (linear layers over all prompt rows, attention per sequence)."""
        n = len(seqs)
        es = [e.reshape(-1, self.dims.llm_hidden) for e in embeds_list]
        lens = [e.shape[0] for e in es]
        cat = es[0].contiguous() if n == 1 else torch.cat(es, dim=0)
        logits = torch.empty(n, self.dims.vocab, device=self.device, dtype=torch.float32) if want_logits else None
        B.check(B.lib.cr_llm_prefill_batch(self._h, kv._h, (C.c_int32 * n)(*seqs), n, _p(cat), (C.c_int32 * n)(*lens),
                                           float(penalty), _p(logits), _stream()), 'cr_llm_prefill_batch')
        return logits

    def score_batch(self, kv, seqs, embeds_list, targets_list, penalty=1.0, top_n=0, want_logits=False):
        """cr_llm_score_batch on the current stream: a continued prefill of embeds_list[i] into sequence seqs[i] that makes no pick and scores the rows
        whose target is >= 0 -- targets_list[i][r] is the id that FOLLOWS row r (< 0: not scored); the repetition penalty of a row runs over the targets of
        the sequence's scored rows before it.  Returns one scores.TokenScores per sequence (top_ids / top_logprobs [T, top_n]), or with want_logits
        (scores, logits): logits [R, vocab] float32 on the device, the raw rows of all R scored rows in row order.  Synchronises the stream."""
        from .scores import TokenScores
        n = len(seqs)
        top_n = int(top_n)
        if not 0 <= top_n <= 8:
            raise ValueError(f'top_n has to be 0..8, got {top_n}')
        if len(embeds_list) != n or len(targets_list) != n:
            raise ValueError(f'score_batch: {n} sequences, {len(embeds_list)} embeddings, {len(targets_list)} target lists')
        es = [e.reshape(-1, self.dims.llm_hidden) for e in embeds_list]
        lens = [e.shape[0] for e in es]
        tg = [[int(t) for t in tl] for tl in targets_list]
        for i in range(n):
            if len(tg[i]) != lens[i]:
                raise ValueError(f'score_batch: sequence {seqs[i]} has {lens[i]} rows but {len(tg[i])} targets')
        flat = [t for tl in tg for t in tl]
        counts = [sum(1 for t in tl if t >= 0) for tl in tg]
        R = sum(counts)
        cat = es[0].contiguous() if n == 1 else torch.cat(es, dim=0)
        lp = torch.empty(max(R, 1), device=self.device, dtype=torch.float32)
        ti = torch.empty(max(R, 1), 8, device=self.device, dtype=torch.int32) if top_n else None
        tl = torch.empty(max(R, 1), 8, device=self.device, dtype=torch.float32) if top_n else None
        logits = torch.empty(max(R, 1), self.dims.vocab, device=self.device, dtype=torch.float32) if want_logits else None
        B.check(B.lib.cr_llm_score_batch(self._h, kv._h, (C.c_int32 * n)(*seqs), n, _p(cat), (C.c_int32 * n)(*lens), (C.c_int64 * len(flat))(*flat),
                                         float(penalty), top_n, _p(lp), _p(ti), _p(tl), _p(logits), _stream()), 'cr_llm_score_batch')
        lp_h = lp.cpu().numpy()
        ti_h = ti.cpu().numpy()[:, :top_n] if top_n else np.empty((R, 0), dtype=np.int32)
        tl_h = tl.cpu().numpy()[:, :top_n] if top_n else np.empty((R, 0), dtype=np.float32)
        out, r = [], 0
        for k in counts:
            out.append(TokenScores(lp_h[r:r + k].copy(), ti_h[r:r + k].copy(), tl_h[r:r + k].copy()))
            r += k
        return (out, logits) if want_logits else out

    def ground_batch(self, kv, seqs, embeds_list, targets_list, spans_list, layers=None, penalty=1.0, top_n=0, want_scores=True):
        """cr_llm_ground_batch on the current stream: score_batch's pass, which also reports the attention mass every scored row puts on the spans of its
        sequence.  spans_list[i] = [(start, end), ...] absolute cache positions of sequence seqs[i] (sorted, not overlapping, inside the sequence's length after
        the call); layers = (layer0, layer1) or None for all.  Returns (scores, mass): one scores.TokenScores per sequence (None each with want_scores=False:
        a grounding-only call that runs no LM head, top_n must be 0) and one float32 CPU tensor [T_i, len(spans_list[i])] per sequence.  Synchronises the
        stream."""
        from . import grounding
        from .scores import TokenScores
        n = len(seqs)
        top_n = int(top_n)
        if not 0 <= top_n <= 8:
            raise ValueError(f'top_n has to be 0..8, got {top_n}')
        if top_n and not want_scores:
            raise ValueError('ground_batch: top_n > 0 needs want_scores')
        if len(embeds_list) != n or len(targets_list) != n or len(spans_list) != n:
            raise ValueError(f'ground_batch: {n} sequences, {len(embeds_list)} embeddings, {len(targets_list)} target lists, {len(spans_list)} span lists')
        l0, l1 = grounding.check_layers(layers, self.dims.llm_layers)
        es = [e.reshape(-1, self.dims.llm_hidden) for e in embeds_list]
        lens = [e.shape[0] for e in es]
        tg = [[int(t) for t in tl] for tl in targets_list]
        for i in range(n):
            if len(tg[i]) != lens[i]:
                raise ValueError(f'ground_batch: sequence {seqs[i]} has {lens[i]} rows but {len(tg[i])} targets')
        spans = [grounding.check_spans(sp) for sp in spans_list]
        flat = [t for tl in tg for t in tl]
        counts = [sum(1 for t in tl if t >= 0) for tl in tg]
        R = sum(counts)
        sp_counts = [len(sp) for sp in spans]
        sp_flat = [v for sp in spans for se in sp for v in se] or [0]
        ld = max(sp_counts + [1])
        cat = es[0].contiguous() if n == 1 else torch.cat(es, dim=0)
        lp = torch.empty(max(R, 1), device=self.device, dtype=torch.float32) if want_scores else None
        ti = torch.empty(max(R, 1), 8, device=self.device, dtype=torch.int32) if top_n else None
        tl = torch.empty(max(R, 1), 8, device=self.device, dtype=torch.float32) if top_n else None
        mass = torch.empty(max(R, 1), ld, device=self.device, dtype=torch.float32)
        B.check(B.lib.cr_llm_ground_batch(self._h, kv._h, (C.c_int32 * n)(*seqs), n, _p(cat), (C.c_int32 * n)(*lens), (C.c_int64 * len(flat))(*flat),
                                          float(penalty), top_n, _p(lp), _p(ti), _p(tl), (C.c_int32 * len(sp_flat))(*sp_flat), (C.c_int32 * n)(*sp_counts),
                                          l0, l1, _p(mass), ld, _stream()), 'cr_llm_ground_batch')
        mass_h = mass.cpu()
        lp_h = lp.cpu().numpy() if want_scores else None
        ti_h = ti.cpu().numpy()[:, :top_n] if top_n else np.empty((R, 0), dtype=np.int32)
        tl_h = tl.cpu().numpy()[:, :top_n] if top_n else np.empty((R, 0), dtype=np.float32)
        out, ms, r = [], [], 0
        for k, w in zip(counts, sp_counts):
            out.append(TokenScores(lp_h[r:r + k].copy(), ti_h[r:r + k].copy(), tl_h[r:r + k].copy()) if want_scores else None)
            ms.append(mass_h[r:r + k, :w].clone())
            r += k
        return out, ms

    def hidden_probe(self, rows=None, row0=0):
        """cr_llm_hidden_probe: `rows` > 0 arms it and returns the [llm_layers + 1, rows, 4096] bf16 tensor the next prefill fills
        (residual stream before layer 0 and after each layer); rows=None disarms."""
        if not rows:
            B.check(B.lib.cr_llm_hidden_probe(self._h, C.c_void_p(0), 0, 0), 'cr_llm_hidden_probe')
            self._probe = None
            return None
        self._probe = torch.zeros(self.dims.llm_layers + 1, rows, self.dims.llm_hidden, device=self.device, dtype=torch.bfloat16)
        B.check(B.lib.cr_llm_hidden_probe(self._h, _p(self._probe), row0, rows), 'cr_llm_hidden_probe')
        return self._probe

    def decode(self, kv, seqs, penalty=1.0, force_tokens=None, want_logits=False):
        n = len(seqs)
        seq_arr = (C.c_int32 * n)(*seqs)
        ft = force_tokens.reshape(-1).to(self.device, torch.int64).contiguous() if force_tokens is not None else None
        logits = torch.empty(n, self.dims.vocab, device=self.device, dtype=torch.float32) if want_logits else None
        B.check(B.lib.cr_llm_decode(self._h, kv._h, seq_arr, n, _p(ft), float(penalty), _p(logits), _stream()), 'cr_llm_decode')
        return logits

    def decode_draft(self, kv, seqs, drafts, penalty=1.0):
        """cr_llm_decode_draft on the current stream: one greedy step that checks `drafts[i]` (0..7 guessed next ids) for sequence seqs[i] in the same
        weight pass.  Returns the count of ids appended per sequence (1 .. len(drafts[i]) + 1); the ids are those of plain decode steps whatever the
        drafts hold.  Synchronises the stream."""
        n = len(seqs)
        lens = [len(d) for d in drafts]
        stride = max(max(lens), 1)
        flat = (C.c_int64 * (n * stride))()
        for i, d in enumerate(drafts):
            flat[i * stride:i * stride + len(d)] = [int(t) for t in d]
        app = (C.c_int32 * n)()
        B.check(B.lib.cr_llm_decode_draft(self._h, kv._h, (C.c_int32 * n)(*seqs), n, flat, (C.c_int32 * n)(*lens), stride, float(penalty), app,
                                          _stream()), 'cr_llm_decode_draft')
        return list(app)


KV_DTYPES = {'bf16': B.CR_KV_BF16, 'e4m3': B.CR_KV_E4M3}


def kv_format(dtype):
    """'bf16' | 'e4m3' -> the cache format of cr_kv_alloc_ex (ValueError otherwise)."""
    if dtype not in KV_DTYPES:
        raise ValueError(f"kv cache dtype must be one of {sorted(KV_DTYPES)}, got {dtype!r}")
    return KV_DTYPES[dtype]


class KVCache:
    def __init__(self, eng, h, n_seqs, max_tokens):
        self.eng, self._h, self.n_seqs, self.max_tokens = eng, h, n_seqs, max_tokens
        fmt = B.lib.cr_kv_format(h)
        self.format = {v: k for k, v in KV_DTYPES.items()}[fmt]      # 'bf16' | 'e4m3'
        self._top_n = {}                                             # seq -> alternatives recorded per id (set_logprobs)
        self.prefix_sharing = False                                  # set_prefix_sharing

    def length(self, seq):
        return B.lib.cr_kv_length(self._h, seq)

    def reset(self, seq=-1):
        """Forget one sequence, or all of them (seq < 0); enqueued on the current stream."""
        B.check(B.lib.cr_kv_reset(self._h, seq, _stream()), 'cr_kv_reset')
        if seq < 0:
            self._top_n.clear()
        else:
            self._top_n.pop(seq, None)

    def truncate(self, seq, n):
        """cr_kv_truncate on the current stream: the sequence keeps its first `n` cached positions and forgets what reset forgets (ids, stop
        criteria, sampling state, scores).  Cache rows are not touched; n = 0 is reset(seq)."""
        B.check(B.lib.cr_kv_truncate(self._h, int(seq), int(n), _stream()), 'cr_kv_truncate')
        self._top_n.pop(seq, None)

    def fork(self, src, dsts, n):
        """cr_kv_fork on the current stream: every sequence of `dsts` takes the cached positions [0, n) of `src` (one launch, the source read once)
        and is otherwise as after truncate(dst, n).  bf16 caches only."""
        dsts = [int(d) for d in dsts]
        B.check(B.lib.cr_kv_fork(self._h, int(src), (C.c_int32 * len(dsts))(*dsts), len(dsts), int(n), _stream()), 'cr_kv_fork')
        for d in dsts:
            self._top_n.pop(d, None)

    def fork_shared(self, src, dsts, n):
        """cr_kv_fork_shared on the current stream: as fork, but only positions [n & ~255, n) are copied; every sequence of `dsts` reads positions
        [0, n & ~255) from `src` from then on (its share), and the decode attention loads those once for all the rows that share them.  Same bits as
        fork.  While it has sharers `src` cannot be reset, cut below the share or prefilled below it: reset the sharers first."""
        dsts = [int(d) for d in dsts]
        B.check(B.lib.cr_kv_fork_shared(self._h, int(src), (C.c_int32 * len(dsts))(*dsts), len(dsts), int(n), _stream()), 'cr_kv_fork_shared')
        for d in dsts:
            self._top_n.pop(d, None)

    def set_prefix_sharing(self, on=True):
        """cr_kv_set_prefix_sharing: while on, fanout and a beam group's fan-out share the prompt instead of copying it (same results, bit for bit).
        Only on a cache none of whose sequences holds tokens; bf16 caches only."""
        B.check(B.lib.cr_kv_set_prefix_sharing(self._h, 1 if on else 0), 'cr_kv_set_prefix_sharing')
        self.prefix_sharing = bool(on)

    def fanout(self, src, dsts, seeds, last_logits):
        """cr_kv_fanout on the current stream: `src` has just been prefilled with sampling on (one generated id); every sequence of `dsts` becomes what a
        lone prefill of the same prompt with seeds[j] would have left -- src's cached prefix (the source read once), its own first id drawn from
        `last_logits` (the raw fp32 row [vocab] that src's prefill returned with want_logits), src's sampling parameters, stop criteria and score
        setting.  bf16 caches, at most 63 destinations; src is not changed."""
        dsts, seeds = [int(d) for d in dsts], [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
        if len(seeds) != len(dsts):
            raise ValueError(f'fanout: {len(seeds)} seeds for {len(dsts)} destinations')
        lg = last_logits
        if lg is not None:
            if not (torch.is_tensor(lg) and lg.is_cuda and lg.dtype == torch.float32 and lg.is_contiguous() and lg.numel() == self.eng.dims.vocab):
                raise ValueError(f'fanout: last_logits has to be one contiguous fp32 row of {self.eng.dims.vocab} scores on the device')
        B.check(B.lib.cr_kv_fanout(self._h, int(src), (C.c_int32 * len(dsts))(*dsts), len(dsts), (C.c_uint64 * len(seeds))(*seeds), _p(lg), _stream()),
                'cr_kv_fanout')
        for d in dsts:
            self._top_n.pop(d, None)
            if src in self._top_n:
                self._top_n[d] = self._top_n[src]

    def read(self, layer, seq, pos, which=0):
        """(8, 128) bf16: K (which=0, after RoPE) or V (which=1) of one cached position, all KV heads."""
        out = torch.empty(8, 128, device=self.eng.device, dtype=torch.bfloat16)
        B.check(B.lib.cr_kv_read(self._h, layer, seq, pos, which, _p(out), _stream()), 'cr_kv_read')
        return out

    def read_e4m3(self, layer, seq, pos, which=0):
        """e4m3 caches: ((8, 128) uint8 e4m3 bytes, (8,) fp32 scales) of one cached position, all KV heads."""
        q = torch.empty(8, 128, device=self.eng.device, dtype=torch.uint8)
        s = torch.empty(8, device=self.eng.device, dtype=torch.float32)
        B.check(B.lib.cr_kv_read_e4m3(self._h, layer, seq, pos, which, _p(q), _p(s), _stream()), 'cr_kv_read_e4m3')
        return q, s

    def set_stop(self, seq, eos_id=None, max_new=0):
        """cr_kv_set_stop on the current stream: from now on the greedy pick records the sequence's stop (its first `eos_id`, or its
        `max_new`-th generated id) and pushes it once onto the finished queue read by poll_finished."""
        B.check(B.lib.cr_kv_set_stop(self._h, seq, -1 if eos_id is None else int(eos_id), int(max_new), _stream()), 'cr_kv_set_stop')

    def set_sampling(self, seq, temperature=0.0, top_k=0, top_p=1.0, seed=0):
        """cr_kv_set_sampling on the current stream: the sequence's later picks sample (temperature > 0; 0 = greedy).  Call after reset(seq) and
        before the sequence's prefill, which makes its first pick."""
        B.check(B.lib.cr_kv_set_sampling(self._h, seq, float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
                'cr_kv_set_sampling')

    def set_constraints(self, seq, constraints):
        """cr_kv_set_constraints on the current stream: the sequence's later picks (its prefill's included) choose among the ids `constraints`
        (a constraints.Constraints) leaves; None switches them off (the default, what reset / truncate / fork restore).  Call after reset(seq) and
        before the sequence's prefill."""
        if constraints is None:
            B.check(B.lib.cr_kv_set_constraints(self._h, int(seq), None, _stream()), 'cr_kv_set_constraints')
            return
        c, _keep = c_constraints(constraints)
        B.check(B.lib.cr_kv_set_constraints(self._h, int(seq), C.byref(c), _stream()), 'cr_kv_set_constraints')

    def poll_finished(self, out):
        """cr_kv_poll_finished: enqueue on the current stream an asynchronous copy of the finished queue into `out`, a pinned int32 CPU tensor of
        at least 1 + 2 n_seqs entries ([0] count pushed, [1 + k % n_seqs] the k-th sequence pushed, [1 + n_seqs + s] stop count of s).  Read it
        after an event recorded behind this call has completed."""
        assert out.dtype == torch.int32 and not out.is_cuda and out.is_contiguous()
        B.check(B.lib.cr_kv_poll_finished(self._h, C.c_void_p(out.data_ptr()), out.numel(), _stream()), 'cr_kv_poll_finished')

    def generated(self, seq, max_tokens=None):
        """The ids generated so far (all of them by default: a sequence never holds more ids than the cache holds tokens)."""
        max_tokens = self.max_tokens if max_tokens is None else max_tokens
        buf = (C.c_int64 * max_tokens)()
        n = B.lib.cr_kv_generated(self._h, seq, buf, max_tokens, _stream())
        if n < 0:
            B.check(n, 'cr_kv_generated')
        return list(buf[:n])

    def set_beam(self, first_seq, num_beams, length_penalty=1.0, early_stopping=False, eos_id=None, max_new=1024):
        """cr_kv_set_beam on the current stream: sequences first_seq .. first_seq + num_beams - 1 become one beam group (transformers' deterministic beam
        search; early_stopping False | True | 'never').  Call after reset and before the prefill of `first_seq`, which is the group's step 0."""
        from .sampling import early_code
        es = early_code(early_stopping)
        B.check(B.lib.cr_kv_set_beam(self._h, int(first_seq), int(num_beams), float(length_penalty), es, -1 if eos_id is None else int(eos_id), int(max_new),
                                     _stream()), 'cr_kv_set_beam')

    def beam_result(self, first_seq):
        """cr_kv_beam_result: (ids of the group's best finished hypothesis so far, its score, done).  Synchronises the current stream."""
        buf = (C.c_int64 * self.max_tokens)()
        score, length, done = C.c_float(), C.c_int32(), C.c_int32()
        n = B.lib.cr_kv_beam_result(self._h, int(first_seq), buf, self.max_tokens, C.byref(score), C.byref(length), C.byref(done), _stream())
        if n < 0:
            B.check(n, 'cr_kv_beam_result')
        return list(buf[:n]), float(score.value), bool(done.value)

    def beam_reorder(self, first_seq, src, start=0):
        """cr_kv_beam_reorder (test entry, plain sequences): sequence first_seq + j takes the cache positions [start, length) and the id history of
        first_seq + src[j], j < len(src)."""
        B.check(B.lib.cr_kv_beam_reorder(self._h, int(first_seq), len(src), (C.c_int32 * len(src))(*[int(x) for x in src]), int(start), _stream()),
                'cr_kv_beam_reorder')

    def set_logprobs(self, seq, top_n):
        """cr_kv_set_logprobs on the current stream: record the log-probability and the `top_n` (1..8) best alternatives of every id the sequence
        generates from now on; 0 switches the scores off (the default, what reset restores).  Call after reset(seq) and before the sequence's prefill."""
        top_n = int(top_n)
        if not 0 <= top_n <= 8:
            raise ValueError(f'top_n has to be 0 (off) or 1..8, got {top_n}')
        B.check(B.lib.cr_kv_set_logprobs(self._h, seq, top_n, _stream()), 'cr_kv_set_logprobs')
        self._top_n[seq] = top_n

    def logprobs(self, seq, max_tokens=None):
        """cr_kv_logprobs: (lp [T] float32, top_ids [T, n] int32, top_lp [T, n] float32) numpy arrays for the T ids generated so far (generated()'s
        count), n the sequence's top_n.  Synchronises the current stream.  CalliReaderError for a sequence whose scores are off."""
        max_tokens = self.max_tokens if max_tokens is None else max_tokens
        lp = np.empty(max_tokens, dtype=np.float32)
        ti = np.empty((max_tokens, 8), dtype=np.int32)
        tl = np.empty((max_tokens, 8), dtype=np.float32)
        n = B.lib.cr_kv_logprobs(self._h, seq, C.c_void_p(lp.ctypes.data), C.c_void_p(ti.ctypes.data), C.c_void_p(tl.ctypes.data), max_tokens, _stream())
        if n < 0:
            B.check(n, 'cr_kv_logprobs')
        k = self._top_n.get(seq) or 8
        return lp[:n].copy(), ti[:n, :k].copy(), tl[:n, :k].copy()

    def free(self):
        if self._h:
            B.lib.cr_kv_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def c_constraints(c):
    """(cr_constraints of a constraints.Constraints, the ctypes arrays it points to: keep them alive across the call)."""
    def arr(ids):
        return (C.c_int32 * len(ids))(*ids) if ids else None
    sup, beg = arr(c.suppress_tokens), arr(c.begin_suppress_tokens)
    alw = arr(c.allowed_token_ids) if c.allowed_token_ids is not None else None
    flat = [t for w in c.bad_words_ids for t in w]
    offs = [0]
    for w in c.bad_words_ids:
        offs.append(offs[-1] + len(w))
    bw, bo = arr(flat), (arr(offs) if c.bad_words_ids else None)
    out = B.Constraints(no_repeat_ngram_size=c.no_repeat_ngram_size, min_new_tokens=c.min_new_tokens,
                        eos_id=-1 if c.eos_token_id is None else c.eos_token_id, n_suppress=len(c.suppress_tokens), suppress=sup,
                        n_begin_suppress=len(c.begin_suppress_tokens), begin_suppress=beg,
                        n_allowed=len(c.allowed_token_ids) if c.allowed_token_ids is not None else 0, allowed=alw,
                        n_bad_words=len(c.bad_words_ids), bad_word_ids=bw, bad_word_offsets=bo)
    return out, (sup, beg, alw, bw, bo)


# ---- single operators (tests / profiling) ----
def op_gemm(epi, A, Wt, bias=None, scale=None, res=None, group=0, out_dtype=torch.bfloat16, n_out=None, kernel=0, out=None, decode_layout=None):
    """kernel: 0 dispatcher's choice, 1 128x128 tiles, 2 256x256 persistent (schedule per shape), 3 weight-streaming, 5 / 6 the 256x256 kernel with
    its 16- / 32-MFMA-slot schedule pinned (tests pin one).  decode_layout = (kind, op_decode_swizzle(which, Wt)): the weight-streaming kernels
    (M <= 64) read that copy of the weight (kind 1: plain tiles, 2: wqkv's RoPE tile order with epi 7); Wt still gives N."""
    M, K = A.shape
    N = Wt.shape[0]
    hi = 0
    if decode_layout is not None:
        hi = decode_layout[0] << 18
        Wt = decode_layout[1].view(-1, K)
    ncols = n_out if n_out is not None else (N // 2 if epi == 4 else N)
    mrows = M if epi != 5 else (M // group) * (group + 1)
    if epi == 7:                     # fp32 K-slice partial sums [S <= 8][M][N]; unused slabs stay zero
        mrows, out_dtype = 8 * M, torch.float32
    if epi == 8:                     # cosine-VQ partials: per row and 64-column block {column (low word), bits of the bf16 max (high word)}
        ncols, out_dtype = ((N + 63) // 64 + 1) & ~1, torch.int64
    Cc = out if out is not None else torch.zeros(mrows, ncols, device=A.device, dtype=out_dtype)
    B.check(B.lib.cr_op_gemm(epi | (kernel << 8) | hi, _p(A), A.stride(0), _p(Wt), Wt.stride(0), _p(Cc), Cc.stride(0), _p(bias), _p(scale),
                             _p(res), res.stride(0) if res is not None else 0, M, N, K, group, _stream()), 'cr_op_gemm')
    return Cc


def op_quantize_fp8(Wt):
    """rows of a bf16 [N, K] matrix -> (uint8 e4m3 [N, K], fp32 scale [N]) exactly as cr_enable_fp8_decode builds them"""
    N, K = Wt.shape
    q = torch.empty(N, K, device=Wt.device, dtype=torch.uint8)
    sc = torch.empty(N, device=Wt.device, dtype=torch.float32)
    B.check(B.lib.cr_op_quantize_fp8(_p(Wt), Wt.stride(0), N, K, _p(q), _p(sc), _stream()), 'cr_op_quantize_fp8')
    return q, sc


def op_decode_swizzle8(q):
    """cr_op_decode_swizzle(which = 8): the decode layout of an e4m3 [N, K] weight copy (1 KiB per 16-row tile and 64-deep k-step)."""
    N, K = q.shape
    out = torch.empty(((N + 15) // 16) * 16 * K, dtype=torch.uint8, device=q.device)
    B.check(B.lib.cr_op_decode_swizzle(8, _p(q), q.stride(0), N, K, _p(out), _stream()), 'cr_op_decode_swizzle(e4m3)')
    return out


def op_gemm_fp8(epi, A, q, sc, res=None, out_dtype=torch.bfloat16, decode_layout=None):
    """cr_op_gemm with e4m3 weights `q` [N, K] and row scales `sc` (decode kernel, M <= 64); decode_layout = op_decode_swizzle8(q): the kernel streams that copy."""
    M, K = A.shape
    N = q.shape[0]
    hi = 0
    if decode_layout is not None:
        hi = 1 << 18
        q = decode_layout.view(-1, K)
    ncols = N // 2 if epi == 4 else N
    mrows = M
    if epi == 7:
        mrows, out_dtype = 8 * M, torch.float32
    Cc = torch.zeros(mrows, ncols, device=A.device, dtype=out_dtype)
    B.check(B.lib.cr_op_gemm(epi | (1 << 16) | hi, _p(A), A.stride(0), _p(q), q.stride(0), _p(Cc), Cc.stride(0), _p(None), _p(sc),
                             _p(res), res.stride(0) if res is not None else 0, M, N, K, 0, _stream()), 'cr_op_gemm(fp8)')
    return Cc


def op_gemm_fp8x8(epi, a8, a_scale, q, sc, bias=None, out_dtype=torch.bfloat16):
    """cr_op_gemm with e4m3 activations `a8` [M, K] + row scales and e4m3 weights `q` [N, K] + row scales: the 256x256 kernel's
    v_mfma_f32_16x16x128_f8f6f4 instance (epi 0 | 1 | 4 | 6)."""
    M, K = a8.shape
    N = q.shape[0]
    Cc = torch.zeros(M, N // 2 if epi == 4 else N, device=a8.device, dtype=out_dtype)
    B.check(B.lib.cr_op_gemm(epi | (1 << 16) | (1 << 17), _p(a8), a8.stride(0), _p(q), q.stride(0), _p(Cc), Cc.stride(0), _p(bias), _p(sc),
                             _p(a_scale), 0, M, N, K, 0, _stream()), 'cr_op_gemm(fp8 x fp8)')
    return Cc


def op_norm_fp8(x, gamma, beta, eps, next_bound=None):
    """LayerNorm (beta given) or RMSNorm (beta None) of bf16 rows -> (uint8 e4m3 [rows, n], fp32 scale [rows]); with next_bound
    (device floats {largest weight-row norm, largest |bias|} of the next linear) also that linear's output-row scales [rows]"""
    rows, n = x.shape
    q = torch.empty(rows, n, device=x.device, dtype=torch.uint8)
    sc = torch.empty(rows, device=x.device, dtype=torch.float32)
    nxt = torch.empty(rows, device=x.device, dtype=torch.float32) if next_bound is not None else None
    B.check(B.lib.cr_op_norm_fp8(_p(x), _p(gamma), _p(beta), rows, n, float(eps), _p(q), _p(sc), _p(nxt), _p(next_bound), _stream()), 'cr_op_norm_fp8')
    return (q, sc, nxt) if nxt is not None else (q, sc)


def op_gemm_q8(a8, a_scale, q, sc, bias, c_scale):
    """cr_op_gemm_q8: fc1 of the fp8 path -- e4m3 x e4m3, GELU, output as e4m3 rows divided by c_scale[m]"""
    M, K = a8.shape
    N = q.shape[0]
    out = torch.zeros(M, N, device=a8.device, dtype=torch.uint8)
    B.check(B.lib.cr_op_gemm_q8(_p(a8), _p(a_scale), _p(q), _p(sc), _p(bias), _p(c_scale), _p(out), M, N, K, _stream()), 'cr_op_gemm_q8')
    return out


def op_layernorm(x, gamma, beta, eps, pixel_shuffle=False):
    if pixel_shuffle:
        T = x.shape[0]
        out = torch.empty(T * 256, 4096, device=x.device, dtype=torch.bfloat16)
        rows, n = T * 256, 4096
    else:
        out = torch.empty_like(x)
        rows, n = x.shape[0], x.shape[1]
    B.check(B.lib.cr_op_layernorm(_p(x), _p(out), _p(gamma), _p(beta), rows, n, eps, 1 if pixel_shuffle else 0, _stream()),
            'cr_op_layernorm')
    return out


def op_layernorm_regroup(x, out, gamma, beta, eps, in_group=0, out_group=0, out_off=0):
    """cr_op_layernorm_regroup: LayerNorm of x's rows written into `out` with the resampler's row regrouping (input row r -> output row
    (r // in_group) * out_group + out_off + r % in_group; out_group = 0: row r).  x (rows, n), out (any rows, n) contiguous bf16.  That the last row written
    lies inside `out` is checked here, where the shape is known; the group arguments themselves are the C entry's to reject."""
    rows, n = x.shape
    for t in (x, out, gamma, beta):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError('op_layernorm_regroup: contiguous bf16 tensors')
    if out.dim() != 2 or out.shape[1] != n or gamma.numel() != n or beta.numel() != n:
        raise ValueError('op_layernorm_regroup: x (rows, n), out (rows_out, n), gamma / beta (n,)')
    if rows and out_group > 0 and in_group > 0:
        last = ((rows - 1) // in_group) * out_group + out_off + (rows - 1) % in_group
    else:
        last = rows - 1
    if last >= out.shape[0]:
        raise ValueError(f'op_layernorm_regroup: output row {last} outside out ({out.shape[0]} rows)')
    B.check(B.lib.cr_op_layernorm_regroup(_p(x), _p(out), _p(gamma), _p(beta), rows, n, eps, int(in_group), int(out_group), int(out_off), _stream()),
            'cr_op_layernorm_regroup')
    return out


def op_perceiver_attention(q, kv, which=0, out=None):
    """cr_op_perceiver_attention: the resampler's attention alone.  q (T * 3, 512), kv (T * 259, 1024) contiguous bf16 (K | V); returns out (T * 3, 512).
    which = 0: the production kernel, 1: round 1's."""
    if q.dim() != 2 or kv.dim() != 2 or q.shape[1] != 512 or kv.shape[1] != 1024 or q.shape[0] % 3 or kv.shape[0] != q.shape[0] // 3 * 259:
        raise ValueError('op_perceiver_attention: q (T * 3, 512), kv (T * 259, 1024)')
    if out is None:
        out = torch.empty_like(q)
    for t in (q, kv, out):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError('op_perceiver_attention: contiguous bf16 tensors')
    if out.shape != q.shape:
        raise ValueError('op_perceiver_attention: out has q\'s shape')
    B.check(B.lib.cr_op_perceiver_attention(int(which), _p(q), _p(kv), _p(out), q.shape[0] // 3, _stream()), 'cr_op_perceiver_attention')
    return out


def op_rmsnorm(x, gamma, eps):
    out = torch.empty_like(x)
    B.check(B.lib.cr_op_rmsnorm(_p(x), _p(out), _p(gamma), x.shape[0], x.shape[1], eps, _stream()), 'cr_op_rmsnorm')
    return out


def op_attention(q, k, v, o, strides, Bn, H, Sq, Sk, head_dim, kv_group=1, causal=False, q_pos0=0, q_prescale=1.0, s_div=1.0):
    st = (C.c_int64 * 12)(*strides)
    B.check(B.lib.cr_op_attention(_p(q), _p(k), _p(v), _p(o), st, Bn, H, Sq, Sk, head_dim, kv_group, 1 if causal else 0,
                                  q_pos0, q_prescale, s_div, _stream()), 'cr_op_attention')
    return o


def op_attention_segments(q, kc, vc, o, segs, s_div=11.313708498984761, Sq=None):
    """cr_op_attention_segments: the prefill attention's segment launch alone.  q / o (rows, H, 128) bf16, kc / vc (n_slots, H_kv, max_tokens, 128) bf16 caches
    holding every segment's keys / values, segs = [(first row, rows, first position, cache slot), ...] on the host; Sq = the grid's longest segment (default: the
    longest of segs).  The ranges are checked here, where the shapes are known: the C entry only sees a device array."""
    rows, H, hd = q.shape
    n_slots, n_kv, max_tokens, _ = kc.shape
    if hd != 128 or kc.shape[3] != 128 or vc.shape != kc.shape or o.shape != q.shape or H % n_kv or not segs:
        raise ValueError('op_attention_segments: q / o (rows, H, 128), kc / vc (n_slots, H_kv, max_tokens, 128)')
    for t in (q, kc, vc, o):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError('op_attention_segments: contiguous bf16 tensors')
    if Sq is None:
        Sq = max(s[1] for s in segs)
    for row0, S, pos0, slot in segs:
        if not (0 <= row0 and 0 < S <= Sq and row0 + S <= rows and 0 <= pos0 and pos0 + S <= max_tokens and 0 <= slot < n_slots):
            raise ValueError(f'op_attention_segments: segment {(row0, S, pos0, slot)} outside q / o ({rows} rows), the cache ({n_slots} x {max_tokens}) or Sq = {Sq}')
    d_seg = torch.tensor([int(x) for s in segs for x in s], dtype=torch.int32).to(q.device)
    B.check(B.lib.cr_op_attention_segments(_p(q), _p(kc), _p(vc), _p(o), _p(d_seg), len(segs), int(Sq), H, H // n_kv, max_tokens, float(s_div), _stream()),
            'cr_op_attention_segments')
    return o


def op_span_mass(q, kc, segs, spans_list, grounded=None, s_div=11.313708498984761, mass_ld=None):
    """cr_op_span_mass: the span-mass kernels of cr_llm_ground_batch alone, on one layer.  q (rows, H, 128) bf16 roped queries, kc (n_slots, H / 4, max_tokens,
    128) bf16 K cache holding every segment's keys, segs = [(first row, rows, first position, cache slot), ...], spans_list[i] = [(start, end), ...] of segment
    i, grounded = a bool per row of q (default: every row).  Returns mass [R, mass_ld] float32 on the device, R = the grounded rows in segment then row order:
    the mean over the H heads of the probability each row puts on each span."""
    rows, H, hd = q.shape
    n_slots, n_kv, max_tokens, _ = kc.shape
    if hd != 128 or kc.shape[3] != 128 or H != 4 * n_kv or not segs or len(spans_list) != len(segs):
        raise ValueError('op_span_mass: q (rows, H, 128), kc (n_slots, H / 4, max_tokens, 128), one span list per segment')
    for t in (q, kc):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError('op_span_mass: contiguous bf16 tensors')
    flags = bytes([1] * rows) if grounded is None else bytes(1 if g else 0 for g in grounded)
    if len(flags) != rows:
        raise ValueError(f'op_span_mass: {len(flags)} grounded flags for {rows} rows')
    R = sum(sum(flags[r0:r0 + S]) for r0, S, _, _ in segs)
    counts = [len(sp) for sp in spans_list]
    ld = max(counts + [1]) if mass_ld is None else int(mass_ld)
    sp_flat = [int(v) for sp in spans_list for se in sp for v in se] or [0]
    seg_flat = [int(x) for s in segs for x in s]
    mass = torch.empty(max(R, 1), ld, device=q.device, dtype=torch.float32)
    B.check(B.lib.cr_op_span_mass(_p(q), rows, _p(kc), n_slots, max_tokens, H, H // n_kv, (C.c_int32 * len(seg_flat))(*seg_flat), len(segs), flags,
                                  (C.c_int32 * len(sp_flat))(*sp_flat), (C.c_int32 * len(counts))(*counts), float(s_div), _p(mass), ld, _stream()),
            'cr_op_span_mass')
    return mass[:R]


def op_decode_swizzle(which, W):
    """cr_op_decode_swizzle: the decode layout of a [N, K] weight for op_decode_gemm's `which` (1 KiB per 16-row tile and 32-deep k-step)."""
    N, K = W.shape
    out = torch.empty(((N + 15) // 16) * 16 * K, dtype=torch.bfloat16, device=W.device)
    B.check(B.lib.cr_op_decode_swizzle(which, _p(W), W.stride(0), N, K, _p(out), _stream()), 'cr_op_decode_swizzle')
    return out


def op_decode_gemm(which, W, M, X=None, xres=None, gamma=None, eps=1e-5, xio=None, C_out=None, rope=None, flags=0, swizzled=None):
    """cr_op_decode_gemm: one small-batch decode GEMM with its neighbours folded in (gemm_decode.hip).  which: 0 wqkv (rope = dict with
    cos, sin, q_out, kc, vc, seqs, lens, max_tokens), 1 wo, 2 w1|w3, 3 w2, 4 LM head.  swizzled: op_decode_swizzle(which, W) -- the kernel then
    streams that copy (W still gives N and K)."""
    N, K = W.shape
    r = rope or {}
    Wp = W if swizzled is None else swizzled
    B.check(B.lib.cr_op_decode_gemm(which, flags | (256 if swizzled is not None else 0), _p(Wp), K, M, N, K, _p(X), X.shape[1] if X is not None else 0,
                                    _p(xres), _p(gamma), eps, _p(xio),
                                    _p(C_out), C_out.shape[1] if C_out is not None else 0, _p(r.get('cos')), _p(r.get('sin')), _p(r.get('q_out')),
                                    _p(r.get('kc')), _p(r.get('vc')), _p(r.get('seqs')), _p(r.get('lens')), r.get('max_tokens', 0), _stream()),
            'cr_op_decode_gemm')


def op_decode_attention(q, kc, vc, seqs, lens, s_div=11.313708498984761, which=0, max_keys=None, scratch=None, out=None):
    """cr_op_decode_attention: q (B, 4096) bf16 = one new token per row, kc / vc (n_slots, 8, max_tokens, 128) bf16 caches that already hold the token's own K / V row at
    position lens[slot], seqs / lens int32 device tensors; returns (B, 4096) bf16.  which = 1 pins the matrix-core split kernel (A/B)."""
    Bn = q.shape[0]
    max_tokens = kc.shape[2]
    if max_keys is None:
        max_keys = int(lens.max().item()) + 1                      # (a host round trip: benchmarks pass max_keys, scratch and out)
    if scratch is None:
        scratch = torch.empty(int(B.lib.cr_op_decode_attention_scratch_floats(Bn, max_keys)), device=q.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(Bn, 4096, device=q.device, dtype=torch.bfloat16)
    B.check(B.lib.cr_op_decode_attention(which, _p(q), _p(kc), _p(vc), max_tokens, _p(seqs), _p(lens), Bn, max_keys, float(s_div), _p(scratch), _p(out), _stream()),
            'cr_op_decode_attention')
    return out


def op_decode_attention_shared(q, kc, vc, seqs, lens, pfx_src, pfx_len, s_div=11.313708498984761, max_keys=None, scratch=None, out=None):
    """cr_op_decode_attention_shared: op_decode_attention where row b reads positions [0, pfx_len[b]) from slot pfx_src[b] (-1: its own throughout) and the
    rest from its own slot seqs[b].  pfx_src / pfx_len: one int per ROW, host sequences; pfx_len a multiple of 256.  Returns (B, 4096) bf16."""
    Bn = q.shape[0]
    max_tokens = kc.shape[2]
    if max_keys is None:
        max_keys = int(lens.max().item()) + 1
    if scratch is None:
        scratch = torch.empty(int(B.lib.cr_op_decode_attention_scratch_floats(Bn, max_keys)), device=q.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(Bn, 4096, device=q.device, dtype=torch.bfloat16)
    ps, pl = [int(x) for x in pfx_src], [int(x) for x in pfx_len]
    if len(ps) != Bn or len(pl) != Bn:
        raise ValueError(f'op_decode_attention_shared: {len(ps)} / {len(pl)} share entries for {Bn} rows')
    B.check(B.lib.cr_op_decode_attention_shared(_p(q), _p(kc), _p(vc), max_tokens, _p(seqs), _p(lens), (C.c_int32 * Bn)(*ps), (C.c_int32 * Bn)(*pl), Bn, max_keys,
                                                float(s_div), _p(scratch), _p(out), _stream()), 'cr_op_decode_attention_shared')
    return out


def op_decode_attention_e4m3(q, kc, vc, ks, vs, seqs, lens, s_div=11.313708498984761, max_keys=None, scratch=None, out=None):
    """cr_op_decode_attention_e4m3: as op_decode_attention over an e4m3 cache -- kc / vc (n_slots, 8, max_tokens, 128) uint8 e4m3 bytes, ks / vs
    (n_slots, 8, max_tokens) fp32 row scales; returns (B, 4096) bf16."""
    Bn = q.shape[0]
    max_tokens = kc.shape[2]
    if max_keys is None:
        max_keys = int(lens.max().item()) + 1
    if scratch is None:
        scratch = torch.empty(int(B.lib.cr_op_decode_attention_scratch_floats(Bn, max_keys)), device=q.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(Bn, 4096, device=q.device, dtype=torch.bfloat16)
    B.check(B.lib.cr_op_decode_attention_e4m3(0, _p(q), _p(kc), _p(vc), _p(ks), _p(vs), max_tokens, _p(seqs), _p(lens), Bn, max_keys, float(s_div),
                                              _p(scratch), _p(out), _stream()), 'cr_op_decode_attention_e4m3')
    return out


def op_sample(eng, logits, temperature, top_k, top_p, seed, step, history=None, hist_len=None, penalty=1.0):
    """cr_op_sample: the sampling pick on given fp32 logits [n, vocab] (per-row temperature / top_k / top_p / seed / step sequences; history
    [n, cap] int64 with hist_len ids per row for the repetition penalty).  Returns (ids int64 [n], kept int32 [n]) on the device."""
    dev = eng.device
    lg = logits.to(dev, torch.float32).contiguous()
    n, V = lg.shape
    col = lambda v, dt: torch.as_tensor(v, dtype=dt).reshape(-1).expand(n).contiguous().to(dev)
    t, k, p, st = col(temperature, torch.float32), col(top_k, torch.int32), col(top_p, torch.float32), col(step, torch.int32)
    u64 = [int(x) & 0xFFFFFFFFFFFFFFFF for x in (seed if hasattr(seed, '__len__') else [seed] * n)]
    sd = torch.tensor([x - (1 << 64) if x >> 63 else x for x in u64], dtype=torch.int64).to(dev)      # the uint64 bits
    if history is None:
        hist, cap, hl = None, 0, torch.zeros(n, dtype=torch.int32, device=dev)
    else:
        hist = history.to(dev, torch.int64).contiguous()
        cap = hist.shape[1]
        hl = (torch.full((n,), cap, dtype=torch.int32) if hist_len is None else col(hist_len, torch.int32)).to(dev)
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    B.check(B.lib.cr_op_sample(eng._h, _p(lg), n, V, _p(hist), cap, _p(hl), float(penalty), _p(t), _p(k), _p(p), _p(sd), _p(st), _p(ids), _p(kept),
                               _stream()), 'cr_op_sample')
    return ids, kept


def op_constrain(logits, constraints, history=None, hist_len=None, seqs=None):
    """cr_op_constrain: the constraint kernel on given fp32 rows [n, vocab] (a contiguous device tensor, MODIFIED in place and returned): row r is
    masked by `constraints` (a constraints.Constraints) against the history of s = seqs[r] (default r): history [n, cap] int64 with hist_len[s] ids.
    Synchronises the current stream."""
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32 and logits.dim() == 2
    n, V = logits.shape
    dev = logits.device
    if history is None:
        hist, cap, hl = None, 0, torch.zeros(n, dtype=torch.int32, device=dev)
    else:
        hist = history.to(dev, torch.int64).contiguous()
        cap = hist.shape[1]
        hl = (torch.full((n,), cap, dtype=torch.int32) if hist_len is None else torch.as_tensor(hist_len, dtype=torch.int32).reshape(-1)).to(dev).contiguous()
        assert hist.shape[0] == n and hl.numel() == n
    sq = None
    if seqs is not None:
        sq_host = [int(x) for x in seqs]
        assert len(sq_host) == n and all(0 <= x < n for x in sq_host)        # the C entry cannot see the device array
        sq = torch.tensor(sq_host, dtype=torch.int32).to(dev)
    c, _keep = c_constraints(constraints)
    B.check(B.lib.cr_op_constrain(C.byref(c), _p(logits), n, V, _p(sq), _p(hist), cap, _p(hl), _stream()), 'cr_op_constrain')
    return logits


BEAM_WORDS = 64          # four-byte words of a beam group's device state (include/callireader_hip.h, cr_op_beam_step)


def op_beam_step(logits, history, hist_len, group, state, fin_ids, penalty=1.0):
    """cr_op_beam_step: one beam-search step on given fp32 rows.  logits [n, V] float32 (overwritten with the penalised log-probabilities), history [n, cap]
    int64 and hist_len [n] int32 (updated), group [n] int32 (first row of each row's group), state [n, 64] int32 (bit patterns; layout in the header),
    fin_ids [n, cap] int64 -- all contiguous device tensors, modified in place.  Synchronises the current stream."""
    n, V = logits.shape
    for t, dt in ((logits, torch.float32), (history, torch.int64), (hist_len, torch.int32), (group, torch.int32), (state, torch.int32), (fin_ids, torch.int64)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt
    assert history.shape[0] == n and fin_ids.shape == history.shape and state.shape == (n, BEAM_WORDS) and hist_len.numel() == n and group.numel() == n
    B.check(B.lib.cr_op_beam_step(_p(logits), n, V, _p(history), history.shape[1], _p(hist_len), float(penalty), _p(group), _p(state), _p(fin_ids), _stream()),
            'cr_op_beam_step')


def op_score_rows(logits, targets, row_seq, hist_index, penalty=1.0, top_n=1):
    """cr_op_score_rows: the score kernels of cr_llm_score_batch on given raw fp32 rows [n, vocab] (device, not modified).  targets[r] = the id scored in row
    r, row_seq[r] = which history the row belongs to, hist_index[r] = its ordinal in it (host lists): row r is penalised at the targets of the rows of the same
    history with a smaller ordinal.  Returns (lp [n] float32, top_ids [n, top_n] int32, top_lp [n, top_n] float32) on the device."""
    top_n = int(top_n)
    if not 0 <= top_n <= 8:
        raise ValueError(f'top_n has to be 0..8, got {top_n}')
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    n, V = logits.shape
    tg, rs, hi = [int(t) for t in targets], [int(t) for t in row_seq], [int(t) for t in hist_index]
    assert len(tg) == n and len(rs) == n and len(hi) == n
    lp = torch.empty(n, dtype=torch.float32, device=logits.device)
    ti = torch.empty(n, 8, dtype=torch.int32, device=logits.device) if top_n else None
    tl = torch.empty(n, 8, dtype=torch.float32, device=logits.device) if top_n else None
    B.check(B.lib.cr_op_score_rows(_p(logits), n, V, (C.c_int64 * n)(*tg), (C.c_int32 * n)(*rs), (C.c_int32 * n)(*hi), float(penalty), top_n, _p(lp), _p(ti),
                                   _p(tl), _stream()), 'cr_op_score_rows')
    if not top_n:
        return lp, None, None
    return lp, ti[:, :top_n].contiguous(), tl[:, :top_n].contiguous()


def op_logprobs(logits, ids, top_n=1):
    """cr_op_logprobs: the score kernels on given fp32 rows z [n, vocab] and the id scored in each row.  Returns (lp [n] float32, top_ids [n, top_n] int32,
    top_lp [n, top_n] float32) on the device."""
    top_n = int(top_n)
    if not 1 <= top_n <= 8:
        raise ValueError(f'top_n has to be 1..8, got {top_n}')
    lg = logits.to(torch.float32).contiguous()
    n, V = lg.shape
    idt = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).to(lg.device).contiguous()
    assert idt.numel() == n and lg.is_cuda
    lp = torch.empty(n, dtype=torch.float32, device=lg.device)
    ti = torch.empty(n, 8, dtype=torch.int32, device=lg.device)
    tl = torch.empty(n, 8, dtype=torch.float32, device=lg.device)
    B.check(B.lib.cr_op_logprobs(_p(lg), n, V, _p(idt), top_n, _p(lp), _p(ti), _p(tl), _stream()), 'cr_op_logprobs')
    return lp, ti[:, :top_n].contiguous(), tl[:, :top_n].contiguous()

"""Host-side mirror of the reference's InternVLChatModel for the image->text path.

Same method names, argument meaning, return values and error behaviour as
/root/reference/InternVL/modeling_internvl_chat.py (extract_feature :299, calli_align :322,
chat_ocr :649, batch_chat :903, chat :955, generate_origin :1021, generate_ocr :1067), so a
caller of the reference (inference.py:37-57, evaluate.py) can switch classes.  All tensor
math runs in libcallireader_hip.so through `Engine`; this file only builds prompts and moves
ids and pixels.  Admission, the decode loop, the EOS / budget cut and the reply text are generation.py's; PagePipeline is pipeline.py's.
There is no PyTorch compute fallback.

`detect_model` is what the reference passes (inference.py:37-42,98): an ultralytics `YOLO` object (or any callable
returning raw boxes); with the sorter loaded (`params/orderformer.pth`, as the reference's __init__ :159 does) the
whole front end of calli_align runs on its detections (ordering.py).  The detector NETWORK itself is third-party
(ultralytics) and is not re-implemented; `boxes=` bypasses it with ordered boxes (examples/0.json).
"""
import json
import os
import time
import weakref

import numpy as np
import torch
from PIL import Image

from .config import ModelDims, IMG_CONTEXT_TOKEN_ID, ALIGNED_TOKEN_ID, EOS_TOKEN_ID
from .conversation import get_conv_template
from .engine import Engine
from .constraints import parse as constraints_parse, per_page as constraints_per_page
from . import draft as drafting
from . import grounding
from . import scoring
from .generation import admit, check_fits, decode_rows, decode_rows_drafted, per_page_sampling, read_scores, release_shared, reply_shape, reply_text, share_cache
from .pipeline import PagePipeline
from .preprocess import load_image, load_image_2, plan_page, plan_chars_array
from .sampling import base_seed, check_rows, fan_seeds, page_seeds, parse as sampling_parse, parse_beams, parse_returns, parse_share, refuse_share, splitmix64
from .scores import generate_outputs, ResponseScores, TokenScores, generate_output, parse as scores_parse, per_page as scores_per_page


class InternVLChatModel:
    main_input_name = 'pixel_values'

    def __init__(self, dims: ModelDims = None, device=0, max_tokens=8192, max_pages=1, kv_cache_dtype='bf16'):
        from .engine import kv_format
        kv_format(kv_cache_dtype)                                            # ValueError for anything but 'bf16' / 'e4m3'
        self._kv_cache_dtype = kv_cache_dtype
        self._pipes = weakref.WeakSet()          # pipelines made from this model that are not closed yet (their caches follow kv_cache_dtype)
        self.dims = dims or ModelDims.full()
        self.engine = Engine(self.dims, device=device, max_pos=min(self.dims.max_pos, max(max_tokens, 64)))
        self.device = self.engine.device
        self.template = 'internlm2-chat'
        self.num_image_token = self.dims.tokens_per_tile                    # :146
        self.downsample_ratio = self.dims.downsample_ratio
        self.ps_version = 'v2'
        self.select_layer = -1
        self.img_context_token_id = None                                    # :192
        self.aligned_token_id = ALIGNED_TOKEN_ID                            # 92537, hard-coded at :1100
        self.conv_template = get_conv_template(self.template)
        self.system_message = self.conv_template.system_message            # :194
        self.max_tokens = max_tokens
        self.max_pages = max_pages
        self.sorter = None                 # ordering.OrderFormer once load_orderformer() has run (modeling_internvl_chat.py:159)
        self.draft_stats = {}            # steps / drafted / accepted of the last call that decoded with a draft (generation.decode_rows_drafted)
        self.gpu_preprocess = True       # tiles are cut/resized/normalised on the GPU (bit-identical to the PIL path)
        self._kv = None
        self._ready = False

    # ---- construction --------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, dims=None, **kw):
        m = cls(dims, **kw)
        m.engine.load_state_dict(sd)
        m._finish()
        return m

    @classmethod
    def from_synthetic(cls, dims=None, seed=0, parts=('vit', 'mlp1', 'resampler', 'vq', 'llm'), outlier_shift=0, **kw):
        """Seeded random weights of the checkpoint's architecture, drawn on the GPU tensor by tensor (outlier_shift: synthetic.outlier_transform)."""
        from . import synthetic
        m = cls(dims, **kw)
        for k, v in synthetic.iter_state_dict(m.dims, parts=parts, seed=seed, device=m.device, outlier_shift=outlier_shift):
            m.engine.load_weight(k, v)
            del v
        m._finish()
        return m

    @classmethod
    def from_pretrained(cls, path, *model_args, params_dir='./params', torch_dtype=torch.bfloat16, config=None, **kw):
        """HF sharded safetensors (model.safetensors.index.json) + params/gauss_norm_mu_sigma.pth, as
        AutoModel.from_pretrained(INTERNVL_PATH, torch_dtype=torch.bfloat16, low_cpu_mem_usage=True,
        trust_remote_code=True) does in inference.py:85-89 / __init__ :153-159.  Shapes come from <path>/config.json.
        Keyword arguments of the HF loader that mean nothing here (low_cpu_mem_usage, trust_remote_code, revision,
        code_revision, ...) are accepted and ignored, so the reference's call works unchanged through the auto_map shim
        (callireader_amd/hf_entry/)."""
        from .weights import load_checkpoint
        if torch_dtype not in (torch.bfloat16, None, 'auto', 'bfloat16'):
            raise ValueError('the engine computes in bf16, the dtype the reference loads the model in (inference.py:87)')
        ours = {k: kw.pop(k) for k in ('device', 'max_tokens', 'max_pages', 'kv_cache_dtype') if k in kw}
        dims = kw.pop('dims', None)
        if dims is None:
            dims = ModelDims.from_hf_config(path) if os.path.exists(os.path.join(path, 'config.json')) else ModelDims.full()
        m = cls(dims, **ours)
        load_checkpoint(m.engine, path, params_dir)
        m._finish()
        of = os.path.join(params_dir, 'orderformer.pth')                    # :159 ORDERFORMER_CHECKPOINT
        if os.path.exists(of):
            m.load_orderformer(torch.load(of, map_location='cpu', weights_only=True))
        return m

    # hooks transformers' AutoModel.from_pretrained(..., trust_remote_code=True) calls on the class auto_map names
    @classmethod
    def register_for_auto_class(cls, auto_class='AutoModel'):
        cls._auto_class = auto_class

    _auto_class = None

    def _finish(self):
        self.engine.load_rope()
        self.engine.finalize()
        self._ready = True

    def eval(self):
        return self

    def cuda(self):
        return self

    def close(self):
        """Release what the model holds on the device and the host: the page feeder (its decode threads, stream and context), the KV cache, the engine's context."""
        f = getattr(self, '_pagefeeder', None)
        if f is not None:
            f.close()
            self._pagefeeder = None
        if self._kv is not None:
            self._kv.free()
            self._kv = None
        self.engine.close()

    @property
    def kv_cache_dtype(self):
        """Format of every KV cache this model allocates (its own, generate_pages', PagePipeline's, ContinuousPipeline's): 'bf16' (default, the
        reference's) or 'e4m3' (Engine.kv_alloc: e4m3 rows + one fp32 scale each, 0.52x the bytes; a throughput option, not parity-preserving)."""
        return self._kv_cache_dtype

    @kv_cache_dtype.setter
    def kv_cache_dtype(self, dtype):
        from .engine import kv_format
        kv_format(dtype)
        if dtype == self._kv_cache_dtype:
            return
        live = [p for p in list(self._pipes) if not getattr(p, 'closed', False)]
        if live:
            raise RuntimeError(f'kv_cache_dtype: {len(live)} pipeline(s) made from this model are still open (close them first: their caches keep their format)')
        if self._kv is not None:                  # the model's own cache is re-made in the new format on next use
            self._kv.free()
            self._kv = None
        self._kv_cache_dtype = dtype

    def _kv_alloc(self, n_seqs, max_tokens):
        return self.engine.kv_alloc(n_seqs, max_tokens, dtype=self._kv_cache_dtype)

    def kv(self, n_seqs=None):
        """The model's own KV cache (the pipeline of chat_ocr_stream has two of its own), with at least `n_seqs` sequences: made with `n_seqs` (default: max_pages)
        when none exists yet, freed and re-made with max(n_seqs, max_pages) when it holds fewer; max_pages follows.  This is the only place that allocates it.  The one-page
        calls ask for ONE sequence -- 1 GB at max_tokens 8192, where a 64-page cache is 69 GB that folder mode's per-image fallback would hold beside the pipeline's."""
        if self._kv is None or self._kv.n_seqs < (n_seqs or 0):
            if self._kv is not None:
                self._kv.free()
                n_seqs = max(n_seqs, self.max_pages)
            self.max_pages = max(n_seqs or 0, self.max_pages)
            self._kv = self._kv_alloc(n_seqs or self.max_pages, self.max_tokens)
        return self._kv

    # ---- the * stages --------------------------------------------------------------------------
    def extract_feature(self, pixel_values):
        """:299-319  (T,3,448,448) -> (T,256,4096)"""
        return self.engine.extract_feature(pixel_values)

    def resampler(self, image_embeddings):
        """models/perceiver_resampler.py:81-100  (T,256,4096) -> (T,3,4096)"""
        return self.engine.resample(image_embeddings)

    @staticmethod
    def pixel_shuffle(x, scale_factor=0.5):
        """:283-297, ps_version 'v2': (N, W, H, C) -> (N, W * s, H * s, C / s^2), a pure re-indexing.  Kept for callers of the reference's method; extract_feature does
        not call it (csrc/vision.hip reads the ViT output in this order while it normalises the rows for mlp1)."""
        n, w, h, c = x.shape
        hs, ws = int(h * scale_factor), int(w * scale_factor)
        x = x.reshape(n, w, hs, int(c / scale_factor)).transpose(1, 2)                    # fold 1 / s of H into the channels
        x = x.reshape(n, hs, ws, int(c / (scale_factor * scale_factor)))                  # ... then 1 / s of W
        return x.transpose(1, 2).contiguous()

    @staticmethod
    def find_coordinates(text):
        """:642-648: every run of digits in the question, as ints (region_wise: x1, x2, y1, y2)."""
        import re
        return [int(n) for n in re.findall(r'\d+', text)]

    def align_tiles(self, pixel_values, drop_zero=False, use_hard_vector_quant=False, verbose=False):
        """The tile path of calli_align after the boxes are known (:587-640):
        extract_feature -> resampler -> vq_cos_sim -> (hard VQ) -> (drop_zero) -> sigma/mu de-normalisation.
        Returns (back_to_origin_flat (n,4096), indices (T,3))."""
        st = time.time()
        image_embeddings = self.extract_feature(pixel_values)
        output = self.resampler(image_embeddings)
        outs = self.engine.vq(output, with_cos=use_hard_vector_quant)
        if use_hard_vector_quant:
            indices, cos_sim_values = outs
            print('Dynamic vector quantization...')                          # :610
        else:
            indices, cos_sim_values = outs, None
        back = self.engine.denorm(output, indices, cos_sim_values, drop_zero=drop_zero, hard_vq=use_hard_vector_quant)
        if verbose:
            torch.cuda.synchronize()
            print(f'extract feat + resampler + vq {time.time() - st:.2f}s')
        # the reference returns vq_cos_sim's squeezed indices: shape (3,) for a single tile (similarity.py:27)
        return back, (indices.squeeze(0) if indices.shape[0] == 1 else indices)

    def calli_align(self, img_path, detect_model, drop_zero=False, use_hard_vector_quant=False, save_path=None,
                    verbose=False, boxes=None):
        """:322-640.  Boxes come from `boxes=` (reading order), or from `detect_model`:
          * with a sorter loaded (`load_orderformer`): `detect_model(image array)` returns RAW detections in any order
            and the reference's front end runs on them -- repeated detection passes, duplicate removal, column merge /
            area split, OrderFormer, per-column top-to-bottom (ordering.py, :346-556);
          * without one: `detect_model(PIL image)` must return the boxes already in reading order.
        The detector network itself (YOLOv10 through ultralytics) is third-party and stays outside this package."""
        if img_path is None:
            return None, None                                               # :554-555
        img = Image.open(img_path).convert('RGB') if isinstance(img_path, str) else img_path.convert('RGB')
        if boxes is None:
            from . import ordering
            boxes = ordering.acquire_boxes(detect_model, img, self.sorter)      # :346-394, :558 (one helper for chat_ocr and the page batches)
        if len(boxes) == 0:
            # the reference reaches torch.cat([]) at :585 with no box on the page
            raise RuntimeError('calli_align: no character box on the page (the reference fails here too: torch.cat() of an empty list, modeling_internvl_chat.py:585)')
        arr = np.array(img)
        if self.gpu_preprocess:
            # one page upload, every crop resized/padded/normalised by cr_preprocess (replaces the per-box PIL loop :580-583)
            h, w = arr.shape[:2]
            jobs = plan_chars_array(boxes, w, h)                                          # clipped to the page, as numpy slicing clips the reference's crops
            results = self.engine.preprocess(torch.from_numpy(arr), jobs, len(jobs))
        else:
            tiles = []
            for xyxy in boxes:                                              # :580-583
                x1, y1, x2, y2 = int(xyxy[0]), int(xyxy[1]), int(xyxy[2]), int(xyxy[3])
                tiles.append(load_image_2(Image.fromarray(arr[y1:y2, x1:x2])).to(torch.bfloat16))
            results = torch.cat(tiles).to(self.device)                      # :585
        return self.align_tiles(results, drop_zero, use_hard_vector_quant, verbose)

    def load_orderformer(self, state_dict, max_nums=50):
        """:159, models/model.py:530-552: `state_dict` = params/orderformer.pth (the reference's `Transformer` keys)."""
        from .ordering import OrderFormer
        self.sorter = OrderFormer.from_state_dict(self.engine, state_dict, max_nums=max_nums)
        return self.sorter

    # ---- generation ----------------------------------------------------------------------------
    def _generate(self, input_embeds, max_new_tokens, eos_token_id, repetition_penalty, sampling=None, check_every=16, logprobs=0, kv=None, seq=0,
                  reset=True, constraints=None, draft_ids=None):
        """transformers 4.45.2 GenerationMixin._sample with num_beams=1 for ONE sequence: greedy (sampling None), or do_sample=True with
        `sampling` (a sampling.SamplingParams; the page's seed is page_seeds(1)[0]); returns only the new ids, EOS included (oracle/generate.py
        documents the semantics).  logprobs = n > 0: returns (ids, scores.TokenScores with n alternatives per id, cut like the ids).
        kv / seq: the cache and sequence to run in (default: the model's own, sequence 0).  reset=False (session.PageSession): the sequence keeps the
        tokens it holds -- the caller has rolled it back with KV.truncate, which leaves no ids and no state -- and `input_embeds` are the rows that
        continue it.  constraints (a constraints.Constraints, greedy only): the masks in front of every pick of this call.
        draft_ids (a list of ids, greedy only): a guess at the ids to come, checked several per decode step (generation.decode_rows_drafted); the ids
        returned are the same with any draft, self.draft_stats says how many steps they took."""
        if constraints is not None and sampling is not None:
            raise NotImplementedError('logits constraints with do_sample=True are not implemented (greedy decoding only)')
        kv = self.kv(1) if kv is None else kv
        if draft_ids is not None:
            if sampling is not None:
                drafting.refuse('do_sample=True')
            if logprobs:
                drafting.refuse('token scores (output_scores / return_scores)')
            if constraints is not None and constraints.active:
                drafting.refuse('logits constraints')
            if kv.format != 'bf16':
                drafting.refuse("an e4m3 KV cache (kv_cache_dtype='e4m3')")
        if reset:
            kv.reset(seq)
        check_fits(kv.length(seq) + input_embeds.shape[0], max_new_tokens, self.max_tokens)
        if sampling is not None:
            kv.set_sampling(seq, sampling.temperature, sampling.top_k, sampling.top_p, page_seeds(1)[0])
        if constraints is not None and constraints.active:
            kv.set_constraints(seq, constraints)
        if logprobs:
            kv.set_logprobs(seq, logprobs)
        self.engine.prefill(kv, seq, input_embeds, penalty=repetition_penalty)
        # one sequence looks BEFORE its first chunk too: a prefill whose own pick is EOS issues no decode step (the batch paths do not look first)
        if draft_ids is not None:
            self.draft_stats = {}
            ids = decode_rows_drafted(self.engine, kv, [seq], max_new_tokens, eos_token_id, repetition_penalty, [draft_ids], stats=self.draft_stats)[0]
        else:
            ids = decode_rows(self.engine, kv, [seq], max_new_tokens, eos_token_id, repetition_penalty, check_every, look_first=True)[0]
        out = torch.tensor([ids], dtype=torch.long, device=self.device)
        return (out, TokenScores.read(kv, seq, len(ids))) if logprobs else out

    def _generate_kw(self, input_embeds, repetition_penalty, generate_kwargs, **where):
        """_generate driven by transformers' keyword arguments: the new ids, or under return_dict_in_generate=True a scores.GenerateOutput.
        where: _generate's kv / seq / reset (a session's turn; no beams there).  draft_ids among the keywords: _generate's draft."""
        generate_kwargs = dict(generate_kwargs)
        draft_ids = generate_kwargs.pop('draft_ids', None)
        max_new, eos, sp = self._gen_args(generate_kwargs, allow_beams=True, allow_returns=True)
        beams = parse_beams(generate_kwargs)
        nret = parse_returns(generate_kwargs)
        share = parse_share(generate_kwargs)       # (with one row per page it is accepted and does nothing)
        if share and draft_ids is not None:
            refuse_share('a draft (draft_ids / draft=)')
        if share and where:
            refuse_share('a page session (its turns continue prefills, which read a sequence\'s own rows)')
        if share and self.kv_cache_dtype != 'bf16':
            refuse_share("kv_cache_dtype='e4m3'")
        if draft_ids is not None:
            if beams is not None:
                drafting.refuse(f'num_beams={beams.num_beams}')
            if nret > 1:
                drafting.refuse(f'num_return_sequences={nret} (sampled answers)')
            draft_ids = [int(t) for t in draft_ids]
        if nret > 1 and where:
            raise NotImplementedError(f'num_return_sequences={nret} in a page session: the samples need sequences of their own beside the trunk '
                                      '(use chat_ocr(history=...), or ask_many for several questions)')
        cons = constraints_parse(generate_kwargs, eos)          # (NotImplementedError with beams or do_sample)
        if cons is not None:
            where = dict(where, constraints=cons)
        if beams is not None and (where.keys() - {'constraints'}):
            raise NotImplementedError(f'num_beams={beams.num_beams} in a page session: cr_kv_set_beam needs empty sequences (use chat_ocr(history=...))')
        if beams is not None:                      # beam search: the page's beams decode as one batch (generate_pages)
            ids, sc = self.generate_pages([input_embeds], max_new, eos, repetition_penalty, num_beams=beams.num_beams, length_penalty=beams.length_penalty,
                                          early_stopping=beams.early_stopping, share_prompt=share)
            seq = torch.tensor([ids[0]], dtype=torch.long, device=self.device)
            if not generate_kwargs.get('return_dict_in_generate', False):
                return seq
            out = generate_output(seq)
            out.sequences_scores = torch.tensor([sc[0]], dtype=torch.float32)
            return out
        if draft_ids is not None:
            where = dict(where, draft_ids=draft_ids)
        n = scores_parse(generate_kwargs)
        if nret > 1:                               # several sampled answers: one prefill, the page's samples decode as one batch (generate_pages)
            outs = self.generate_pages([input_embeds], max_new, eos, repetition_penalty, sampling=sp, logprobs=n, num_return_sequences=nret, share_prompt=share)
            ids, tss = (outs[0][0], outs[1][0]) if n else (outs[0], None)
            pad = generate_kwargs.get('pad_token_id')
            pad = (eos if eos is not None else 0) if pad is None else pad         # transformers: pad_token_id defaults to the EOS id
            seq = torch.full((nret, max(len(r) for r in ids)), int(pad), dtype=torch.long)
            for j, r in enumerate(ids):
                seq[j, :len(r)] = torch.tensor(r, dtype=torch.long)
            seq = seq.to(self.device)
            if not generate_kwargs.get('return_dict_in_generate', False):
                return seq
            return generate_outputs(seq, tss)
        if not generate_kwargs.get('return_dict_in_generate', False):
            return self._generate(input_embeds, max_new, eos, repetition_penalty, sp, **where)
        if not n:
            return generate_output(self._generate(input_embeds, max_new, eos, repetition_penalty, sp, **where))
        return generate_output(*self._generate(input_embeds, max_new, eos, repetition_penalty, sp, logprobs=n, **where))

    @staticmethod
    def _gen_args(generate_kwargs, allow_beams=False, allow_returns=False):
        """(max_new_tokens, eos_token_id, SamplingParams or None for greedy): transformers' defaults and validation (sampling.parse).  These are the
        arguments of the one-row-per-page loops: a caller that has no beam path (the pipelines, the sharded entry points, chat) gets NotImplementedError for
        num_beams > 1; the callers that run beams (allow_beams) parse them with sampling.parse_beams.  Likewise num_return_sequences > 1: the callers that
        fan a page out (allow_returns) read the count with sampling.parse_returns, the others raise NotImplementedError."""
        if not allow_beams and parse_beams(generate_kwargs) is not None:
            raise NotImplementedError(f"num_beams={generate_kwargs.get('num_beams')}: this entry point decodes one row per page (num_beams=1); beam search runs "
                                      'through generate / generate_ocr / generate_origin, chat_ocr, dynamic_chat, generate_pages and chat_ocr_pages')
        sp = sampling_parse(generate_kwargs)
        if not allow_returns and parse_share(generate_kwargs):      # the entry points that fan a page out are the ones that can share its prompt
            refuse_share('this entry point (the pipelines, the sharded entry points, page sessions and chat decode one row per page or own their caches)')
        if not allow_returns and parse_returns(generate_kwargs) > 1:
            raise NotImplementedError(f"num_return_sequences={generate_kwargs.get('num_return_sequences')}: this entry point returns one answer per page (the "
                                      'pipelines, the sharded entry points and page sessions own their caches); several sampled answers per page come from '
                                      'generate / generate_ocr / generate_origin, chat_ocr, dynamic_chat, chat_ocr_pages and generate_pages')
        return generate_kwargs.get('max_new_tokens', 1024), generate_kwargs.get('eos_token_id', EOS_TOKEN_ID), sp

    @staticmethod
    def _score_args(generation_config, return_scores):
        """(generation_config with the score keywords set, n) for a chat entry point called with return_scores: True records the
        generation_config's `top_logprobs` alternatives per token (default 1), an int 1..8 that many."""
        gc = dict(generation_config)
        if not return_scores:
            return gc, 0
        n = (gc.get('top_logprobs') or 1) if return_scores is True else return_scores
        gc.update(return_dict_in_generate=True, output_scores=True, top_logprobs=n)
        return gc, scores_parse(gc)

    @staticmethod
    def _with_scores(tokenizer, out):
        """(ids tensor, ResponseScores or None) of what a generate_* call returned."""
        if hasattr(out, 'sequences'):
            if isinstance(out.scores, list):       # num_return_sequences > 1: one ResponseScores per sample, over its own (unpadded) ids
                return out.sequences, [ResponseScores.build(tokenizer, row[:len(ts)].tolist(), ts) for row, ts in zip(out.sequences, out.scores)]
            return out.sequences, ResponseScores.build(tokenizer, out.sequences[0].tolist(), out.scores)
        return out, None

    @staticmethod
    def _reply_texts(tokenizer, out, sep):
        """reply_text of a generate_* call's ids: the response, or for num_return_sequences > 1 (an [n, L] tensor, right-padded) the list of n responses."""
        if out.shape[0] == 1:
            return reply_text(tokenizer, out, sep)
        return [reply_text(tokenizer, out[j:j + 1], sep) for j in range(out.shape[0])]

    @staticmethod
    def _first(response):
        """What the history keeps of a turn: the response, sample 0's when several were returned."""
        return response[0] if isinstance(response, list) else response

    @torch.no_grad()
    def generate_ocr(self, pixel_values=None, input_ids=None, attention_mask=None, visual_features=None,
                     generation_config=None, reference_embeds=None, output_hidden_states=None, return_dict=None,
                     repetition_penalty=1.5, **generate_kwargs):
        """:1067-1122.  draft_ids=[...] among the keywords (not the reference's): a guess at the answer's ids, checked several per decode step; the
        ids returned do not depend on it (draft.py).  Greedy, num_beams=1, no scores, no constraints, a bf16 cache."""
        assert self.img_context_token_id is not None                        # :1081
        if input_ids.shape[0] != 1:
            raise NotImplementedError('generate_ocr handles one page per call, as chat_ocr does')
        if pixel_values is not None:
            vit_embeds = visual_features if visual_features is not None else self.extract_feature(pixel_values)
            ids = input_ids.reshape(-1)
            assert (ids == self.img_context_token_id).sum() != 0            # :1095
            if reference_embeds is not None:
                assert (ids == self.aligned_token_id).sum() != 0            # :1101
            input_embeds = self.engine.embed_splice(ids, vit_embeds, reference_embeds,
                                                    img_id=self.img_context_token_id, ref_id=self.aligned_token_id)
        else:
            input_embeds = self.engine.embed_splice(input_ids.reshape(-1))  # :1107
        return self._generate_kw(input_embeds, repetition_penalty, generate_kwargs)

    @torch.no_grad()
    def generate_origin(self, pixel_values=None, input_ids=None, attention_mask=None, visual_features=None,
                        generation_config=None, output_hidden_states=None, return_dict=None, **generate_kwargs):
        """:1021-1065 (no pseudo-tokens, no repetition penalty unless passed)"""
        penalty = generate_kwargs.pop('repetition_penalty', 1.0)
        return self.generate_ocr(pixel_values, input_ids, attention_mask, visual_features, generation_config, None,
                                 output_hidden_states, return_dict, repetition_penalty=penalty, **generate_kwargs)

    @torch.no_grad()
    def generate(self, pixel_values=None, input_ids=None, attention_mask=None, visual_features=None, generation_config=None,
                 output_hidden_states=None, return_dict=None, **generate_kwargs):
        """:1124-1183.  The CalliAlign-only path: every tile's 256 visual tokens are resampled to 3 pseudo-tokens,
        snapped to the normalised table, de-normalised (no drop_zero, no hard VQ) and spliced at the <IMG_CONTEXT>
        positions (3 per tile: dynamic_chat sets num_image_token = 3).  One row per call, like the other generate_*."""
        assert self.img_context_token_id is not None                        # :1137
        if input_ids.shape[0] != 1:
            raise NotImplementedError('generate handles one prompt per call; dynamic_chat(batch=True) loops over rows')
        penalty = generate_kwargs.pop('repetition_penalty', 1.0)
        if pixel_values is not None:
            vit_embeds = visual_features if visual_features is not None else self.extract_feature(pixel_values)   # :1139-1143
            vit_embeds = self.resampler(vit_embeds)                         # :1147
            indices = self.engine.vq(vit_embeds)                            # :1153
            vit_embeds = self.engine.denorm(vit_embeds, indices)            # :1156  x * sigma[idx] + mu[idx]
            ids = input_ids.reshape(-1)
            assert (ids == self.img_context_token_id).sum() != 0            # :1164
            input_embeds = self.engine.embed_splice(ids, vit_embeds, None, img_id=self.img_context_token_id)
        else:
            input_embeds = self.engine.embed_splice(input_ids.reshape(-1))  # :1172
        return self._generate_kw(input_embeds, penalty, generate_kwargs)

    # ---- chat API ------------------------------------------------------------------------------
    def _build_query(self, question, history, num_patches_list, IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN):
        template = get_conv_template(self.template)
        template.system_message = self.system_message
        history = [] if history is None else history
        for (old_question, old_answer) in history:
            template.append_message(template.roles[0], old_question)
            template.append_message(template.roles[1], old_answer)
        template.append_message(template.roles[0], question)
        template.append_message(template.roles[1], None)
        query = template.get_prompt()
        for num_patches in num_patches_list:
            image_tokens = IMG_START_TOKEN + IMG_CONTEXT_TOKEN * self.num_image_token * num_patches + IMG_END_TOKEN
            query = query.replace('<image>', image_tokens, 1)
        return query, template, history

    def chat(self, tokenizer, pixel_values, question, generation_config, history=None, return_history=False,
             num_patches_list=None, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>', IMG_CONTEXT_TOKEN='<IMG_CONTEXT>',
             verbose=False, return_scores=False):
        """:955-1018.  return_scores (True, or the number of alternatives per token): a scores.ResponseScores is returned after the response
        (after `history` when that is returned)."""
        if history is None and pixel_values is not None and '<image>' not in question:
            question = '<image>\n' + question
        if num_patches_list is None:
            num_patches_list = [pixel_values.shape[0]] if pixel_values is not None else []
        assert pixel_values is None or len(pixel_values) == sum(num_patches_list)       # :965
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        query, template, history = self._build_query(question, history, num_patches_list, IMG_START_TOKEN,
                                                     IMG_END_TOKEN, IMG_CONTEXT_TOKEN)
        model_inputs = tokenizer(query, return_tensors='pt')
        generation_config, _ = self._score_args(generation_config, return_scores)
        generation_config['eos_token_id'] = tokenizer.convert_tokens_to_ids(template.sep)
        self._gen_args(generation_config)           # the plain chat keeps its num_beams=1 contract (beams: chat_ocr, dynamic_chat, generate_*)
        out = self.generate_origin(pixel_values=pixel_values, input_ids=model_inputs['input_ids'],
                                   attention_mask=model_inputs['attention_mask'], **generation_config)
        out, sc = self._with_scores(tokenizer, out)
        response = reply_text(tokenizer, out, template.sep)
        history.append((question, response))
        return reply_shape(response, history, sc, return_history, return_scores)

    def chat_ocr(self, tokenizer, detect_model, img_path, questions, generation_config, num_patches_list=None,
                 history=None, return_history=False, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>',
                 IMG_CONTEXT_TOKEN='<IMG_CONTEXT>', ALIGNED_TOKEN='[UNUSED_TOKEN_140]', verbose=False, image_counts=None,
                 batch=False, use_p=True, drop_zero=False, hard_vq=False, repetition_penalty=1.5, region_wise=False,
                 boxes=None, return_scores=False, draft=None):
        """:649-762.  return_scores (True, or the number of alternatives per token): a scores.ResponseScores is returned after the response
        (after `history` when that is returned); a detection failure still returns its message alone.
        num_return_sequences = n > 1 in the generation_config (with do_sample=True): the response is a LIST of n sampled responses from one visual stage
        and one prefill, the scores a list of n ResponseScores (total_logprob ranks them); the history keeps sample 0's response.
        draft (None: off): 'align' drafts the answer with this call's CalliAlign indices -- the rows of the LLM's own embedding table that the VQ step
        snapped the character boxes to (draft.from_indices; needs use_p) -- or a list of ids does; the response is the same, in fewer decode steps where
        the draft is right."""
        if draft is not None and return_scores:
            drafting.refuse('return_scores')
        if isinstance(draft, str) and (draft != 'align' or not use_p):
            raise ValueError(f"chat_ocr: draft={draft!r} (want None, 'align' with use_p=True, or a list of ids)")
        if self._returns(generation_config, 1) > 1 and draft is not None:      # refused before the visual stage
            drafting.refuse('num_return_sequences > 1 (sampled answers)')
        pixel_values = None
        sub_img = None
        page = None                       # the decoded page, handed on to calli_align (the reference opens the file a second time there, :558: 14.5 ms of JPEG decode on the example page)
        if img_path is not None:
            try:
                if region_wise:
                    img = np.array(Image.open(img_path).convert('RGB'))
                    x1, x2, y1, y2 = self.find_coordinates(questions)                    # :661-663
                    sub_img = Image.fromarray(img[y1:y2, x1:x2])
                    questions = '输出图片中所有文字:'
                    pixel_values = load_image(sub_img).to(torch.bfloat16).to(self.device)
            except Exception:
                raise FileNotFoundError                                         # :670-671
            if not region_wise:
                page, pixel_values = self._open_page(img_path)
        out_tokens = None
        if use_p:
            if region_wise:
                try:
                    out_tokens, indices = self.calli_align(sub_img, detect_model, drop_zero=drop_zero,
                                                           use_hard_vector_quant=hard_vq, verbose=verbose, boxes=boxes)
                except Exception:
                    return '检测失败'                                            # :676-679
            else:
                out_tokens, indices = self.calli_align(page, detect_model, drop_zero=drop_zero, use_hard_vector_quant=hard_vq, verbose=verbose, boxes=boxes)
        question, history, template, model_inputs, generation_config = self._ocr_prompt(
            tokenizer, questions, history, None if pixel_values is None else len(pixel_values), out_tokens, use_p, num_patches_list, generation_config,
            return_scores, IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN, ALIGNED_TOKEN)
        if draft is not None:
            generation_config['draft_ids'] = drafting.from_indices(indices) if isinstance(draft, str) else list(draft)
        out = self.generate_ocr(pixel_values=pixel_values, input_ids=model_inputs['input_ids'],
                                attention_mask=model_inputs['attention_mask'],
                                reference_embeds=out_tokens if use_p else None,
                                repetition_penalty=repetition_penalty, **generation_config)
        return self._ocr_reply(tokenizer, out, template, question, history, return_history, return_scores)

    def _open_page(self, img_path):
        """(the decoded page, its tiles' pixel_values) of chat_ocr's image (:664-671), shared with session.PageSession.open: the tiles are cut on the GPU, or
        through PIL with gpu_preprocess off.  Whatever fails, the reference's FileNotFoundError."""
        try:
            page = Image.open(img_path).convert('RGB') if isinstance(img_path, str) else img_path.convert('RGB')
            if self.gpu_preprocess:
                jobs, n = plan_page(*page.size)
                return page, self.engine.preprocess(torch.from_numpy(np.array(page)), jobs, n)
            return page, load_image(page).to(torch.bfloat16).to(self.device)
        except Exception:
            raise FileNotFoundError                                             # :670-671

    def _ocr_prompt(self, tokenizer, questions, history, n_tiles, out_tokens, use_p, num_patches_list, generation_config, return_scores,
                    IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>', IMG_CONTEXT_TOKEN='<IMG_CONTEXT>', ALIGNED_TOKEN='[UNUSED_TOKEN_140]'):
        """chat_ocr between the visual stage and the language model (:690-732), shared with session.PageSession: the question as the history keeps it,
        the history list, the template, the tokenised query and the generation_config with the score keywords and the EOS id set.  n_tiles: the page's
        tiles, None without an image; out_tokens: the pseudo-token rows (their count is appended to a first turn's question)."""
        question = questions
        if n_tiles is not None and '<image>' not in questions:
            question = '<image>\n' + questions                                  # :690-691
        if history is None and use_p and ALIGNED_TOKEN not in question:
            question = question + ALIGNED_TOKEN * out_tokens.shape[0]           # :698-699
        if num_patches_list is None:
            num_patches_list = [n_tiles] if n_tiles is not None else []
        assert n_tiles is None or n_tiles == sum(num_patches_list)              # :702
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        query, template, history = self._build_query(question, history, num_patches_list, IMG_START_TOKEN,
                                                     IMG_END_TOKEN, IMG_CONTEXT_TOKEN)
        model_inputs = tokenizer(query, return_tensors='pt')
        generation_config, _ = self._score_args(generation_config, return_scores)
        generation_config['eos_token_id'] = tokenizer.convert_tokens_to_ids(template.sep)   # :709,732
        return question, history, template, model_inputs, generation_config

    def _ocr_reply(self, tokenizer, out, template, question, history, return_history, return_scores):
        """chat_ocr after the language model (:752-762): the response text, appended to the history, in the shape the caller asked for."""
        out, sc = self._with_scores(tokenizer, out)
        response = self._reply_texts(tokenizer, out, template.sep)              # :752-753
        history.append((question, self._first(response)))
        return reply_shape(response, history, sc, return_history, return_scores)

    def open_page(self, tokenizer, detect_model, img_path, use_p=True, drop_zero=False, hard_vq=False, boxes=None, max_branches=1, verbose=False):
        """A session.PageSession on one page: the visual stage of chat_ocr runs once here, and the turns asked through the session
        (session.chat_ocr, session.ask_many) keep the page's KV cache between them.  A detection failure behaves as chat_ocr's does."""
        from .session import PageSession
        return PageSession.open(self, tokenizer, detect_model, img_path, use_p=use_p, drop_zero=drop_zero, hard_vq=hard_vq, boxes=boxes,
                                max_branches=max_branches, verbose=verbose)

    def dynamic_chat(self, tokenizer, pixel_values, questions, generation_config, num_patches_list=None, history=None,
                     return_history=False, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>', IMG_CONTEXT_TOKEN='<IMG_CONTEXT>',
                     verbose=False, image_counts=None, batch=False, use_p=True, return_scores=False):
        """:765-901.  `use_p` switches every tile to 3 pseudo-tokens (and, as upstream, leaves num_image_token at 3 on
        the object afterwards).  batch=True: a list of questions, one answer each (the reference pads them into one
        batch; here every row runs at its own length and the rows decode together).  batch=False: the reference's
        hard-wired single-turn prompt (:857-866), history only feeds the returned list.  return_scores: a scores.ResponseScores after the
        response (after `history` when returned); batch=True: (responses, [ResponseScores per question])."""
        if use_p:
            self.num_image_token = 3                                        # :768-769
        gen = self.generate if use_p else self.generate_origin
        generation_config, _ = self._score_args(generation_config, return_scores)
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        if batch:
            assert isinstance(questions, list) and len(questions) > 0 and isinstance(questions[0], str)
            if history is not None or return_history:
                print('Now multi-turn chat is not supported in batch_chat.')
                raise NotImplementedError
            if image_counts is not None:
                num_patches_list = image_counts
                print('Warning: `image_counts` is deprecated. Please use `num_patches_list` instead.')
            if verbose and pixel_values is not None:
                print(f'dynamic ViT batch size: {pixel_values.shape[0]}')
            template = get_conv_template(self.template)
            generation_config['eos_token_id'] = tokenizer.convert_tokens_to_ids(template.sep)
            responses, all_sc, off = [], [], 0
            for idx, num_patches in enumerate(num_patches_list):
                question = questions[idx]
                if pixel_values is not None and '<image>' not in question:
                    question = '<image>\n' + question
                t = get_conv_template(self.template)                         # no system_message override here (:790)
                t.append_message(t.roles[0], question)
                t.append_message(t.roles[1], None)
                query = t.get_prompt().replace('<image>', IMG_START_TOKEN + IMG_CONTEXT_TOKEN * self.num_image_token * num_patches + IMG_END_TOKEN, 1)
                ids = tokenizer(query, return_tensors='pt')['input_ids']
                px = pixel_values[off:off + num_patches] if pixel_values is not None else None
                off += num_patches
                out, sc = self._with_scores(tokenizer, gen(pixel_values=px, input_ids=ids, **generation_config))
                all_sc.append(sc)
                responses.append(self._reply_texts(tokenizer, out, template.sep))
            return (responses, all_sc) if return_scores else responses
        assert isinstance(questions, str)
        if num_patches_list is None:
            num_patches_list = [pixel_values.shape[0]] if pixel_values is not None else []
        assert pixel_values is None or len(pixel_values) == sum(num_patches_list)          # :829
        template = get_conv_template(self.template)
        template.system_message = self.system_message
        generation_config['eos_token_id'] = tokenizer.convert_tokens_to_ids(template.sep)
        history = [] if history is None else history
        if verbose and pixel_values is not None:
            print(f'dynamic ViT batch size: {pixel_values.shape[0]}')
        # the reference discards the template's prompt and builds this string (:857-866): no newline after the roles,
        # no <img> markers, `num_image_token` context tokens per <image> whatever the tile count
        query = ('<|im_start|>system你是由上海人工智能实验室联合商汤科技开发的书生多模态大模型，英文名叫InternVL, 是一个有用无害的人工智能助手。<|im_end|>\n'
                 f'<|im_start|>user{questions}') + '<image>'
        for _ in num_patches_list:
            query = query.replace('<image>', IMG_CONTEXT_TOKEN * self.num_image_token, 1)
        query += '<|im_end|>\n<|im_start|>assistant'
        model_inputs = tokenizer(query, return_tensors='pt')
        out = gen(pixel_values=pixel_values, input_ids=model_inputs['input_ids'], attention_mask=model_inputs['attention_mask'],
                  **generation_config)
        out, sc = self._with_scores(tokenizer, out)
        response = self._reply_texts(tokenizer, out, template.sep)
        history.append((questions, self._first(response)))
        if verbose and not return_history and not return_scores:               # only on the plain-response return
            print(query.replace(IMG_CONTEXT_TOKEN, '').replace(f'{IMG_START_TOKEN}{IMG_END_TOKEN}', '<image>'), response)
        return reply_shape(response, history, sc, return_history, return_scores)

    def chat_ocr_pages(self, tokenizer, detect_model, images, question, generation_config, boxes_list=None, use_p=True,
                       drop_zero=False, hard_vq=False, repetition_penalty=1.5, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>',
                       IMG_CONTEXT_TOKEN='<IMG_CONTEXT>', ALIGNED_TOKEN='[UNUSED_TOKEN_140]', errors='raise', return_scores=False, share_prompt=False):
        """Many pages at once (new: the reference's chat_ocr is one page per call, evaluate.py loops over it).  The
        character tiles of ALL pages go through the visual stage as one batch, the prompts are prefilled together and
        the pages decode as one batch; every page gets exactly the response its own chat_ocr call would produce.
        errors='return': a page whose own chat_ocr call would raise before generation (unreadable image, detector failure, no box, prompt too long) gets that
        exception object in its slot and the other pages run -- what folder mode's per-image try/except needs (inference.py:55-57).
        return_scores (True, or the number of alternatives per token): returns (responses, scores) with one scores.ResponseScores per page (None for a
        page that failed).
        share_prompt (or share_prompt=True in the generation_config): with beams or num_return_sequences > 1 a page's rows read one cached copy of its
        prompt in decode (generate_pages); the responses are the same."""
        constraints_parse(generation_config, 0)                 # refused before the visual stage (the EOS id does not change what is refused)
        _, lpn = self._score_args(generation_config, return_scores)
        beams = parse_beams(dict(generation_config, return_scores=return_scores))
        nret = self._returns(generation_config, len(images))    # (so are too many rows and an e4m3 cache)
        share = parse_share(dict(share_prompt=share_prompt)) or parse_share(generation_config)
        if share and self.kv_cache_dtype != 'bf16':
            refuse_share("kv_cache_dtype='e4m3'")
        embeds, meta = self._ocr_embeds(tokenizer, detect_model, images, question, generation_config, boxes_list, use_p, drop_zero,
                                        hard_vq, IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN, ALIGNED_TOKEN, errors=errors, allow_returns=True)
        if beams is not None:                      # every page's beams in one decode batch; a page gets what its own chat_ocr call gives
            outs = self.generate_pages(embeds, meta['max_new'], meta['eos'], repetition_penalty, num_beams=beams.num_beams, length_penalty=beams.length_penalty,
                                       early_stopping=beams.early_stopping, share_prompt=share)[0] if embeds else []
            return self._answer(tokenizer, outs, meta, False)
        outs = self.generate_pages(embeds, meta['max_new'], meta['eos'], repetition_penalty, sampling=meta['sampling'],
                                   seeds=self._ok_seeds(meta, nret), logprobs=lpn, constraints=meta['constraints'],
                                   num_return_sequences=nret, share_prompt=share) if embeds else []
        return self._answer(tokenizer, outs, meta, return_scores)

    def _returns(self, generation_config, P):
        """num_return_sequences of a call over P pages, with what can be refused before the visual stage runs."""
        nret = parse_returns(dict(generation_config))
        if nret > 1:
            check_rows(P, nret)
            if self.kv_cache_dtype != 'bf16':
                raise NotImplementedError(f"num_return_sequences={nret} with kv_cache_dtype='e4m3': the fan-out copies bf16 rows (cr_kv_fanout); call the "
                                          'entry point n times, or use a bf16 cache')
        return nret

    def _answer(self, tokenizer, outs, meta, return_scores):
        """_responses of a batch, or with return_scores (outs = (ids, TokenScores) lists, or empty) the pair (responses, ResponseScores per page: None for
        a page that did not run)."""
        if not return_scores:
            return self._responses(tokenizer, outs, meta)
        outs, tss = outs if outs else ([], [])
        sc = [None] * meta['n']
        for i, o, ts in zip(meta['ok'], outs, tss):
            sc[i] = [ResponseScores.build(tokenizer, oj, tj) for oj, tj in zip(o, ts)] if isinstance(ts, list) else ResponseScores.build(tokenizer, o, ts)
        return self._responses(tokenizer, outs, meta), sc

    @staticmethod
    def _ok_seeds(meta, nret=1):
        """Seeds of the pages that reach the language model: page j of the call (input order, failed pages included) has page_seeds(n)[j]; with nret
        returned sequences per page its sample k has page_seeds(n * nret)[j * nret + k] (sampling.fan_seeds), flat in page order."""
        if meta['sampling'] is None:
            return None
        seeds = fan_seeds(meta['n'], nret)
        return [sd for i in meta['ok'] for sd in seeds[i]]

    @staticmethod
    def _responses(tokenizer, outs, meta):
        """ids of the pages that ran + the exceptions of those that did not -> one entry per page of the batch, in order (:752-753 per page)."""
        sep = meta['template'].sep
        res = [None] * meta['n']
        for i, o in zip(meta['ok'], outs):
            res[i] = [reply_text(tokenizer, oj, sep) for oj in o] if o and isinstance(o[0], list) else reply_text(tokenizer, o, sep)
        for i, e in meta['failed'].items():
            res[i] = e
        return res

    def chat_ocr_stream(self, tokenizer, detect_model, image_batches, question, generation_config, boxes_batches=None, use_p=True,
                        drop_zero=False, hard_vq=False, repetition_penalty=1.5, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>',
                        IMG_CONTEXT_TOKEN='<IMG_CONTEXT>', ALIGNED_TOKEN='[UNUSED_TOKEN_140]', errors='raise', stats=None, return_scores=False, draft=None):
        """chat_ocr_pages over a sequence of page batches with two batches in flight (PagePipeline): a generator that yields one
        list of responses per batch, in order; batch i decodes on a second stream while batch i+1 is detected, tiled, encoded and
        prefilled, and the image files of batch i+2 are being decoded on the feeder's threads (pageio.PageFeeder).  Every page gets the
        response of its own chat_ocr call.  stats (a dict) receives the host seconds per stage and, per batch, how long the compute stream
        sat between the previous batch's prefill and this batch's first kernel.  return_scores: every batch is yielded as (responses, scores), as
        chat_ocr_pages returns it."""
        if parse_beams(generation_config) is not None:
            raise NotImplementedError('chat_ocr_stream: beam search does not go through PagePipeline (use chat_ocr_pages)')
        if parse_share(generation_config):
            refuse_share('PagePipeline (chat_ocr_stream: it owns its caches and decodes one row per page)')
        if draft is not None:
            drafting.refuse('PagePipeline (chat_ocr_stream: its decode thread issues steps without waiting for them)')
        if parse_returns(dict(generation_config)) > 1:
            raise NotImplementedError('chat_ocr_stream: num_return_sequences > 1 does not go through PagePipeline, which owns its caches (use chat_ocr_pages)')
        constraints_parse(generation_config, 0)                 # refused before the first batch is pulled
        _, lpn = self._score_args(generation_config, return_scores)
        pipe, pending = None, None
        sampled = sampling_parse(generation_config) is not None
        base, page0, n_prev = (base_seed() if sampled else 0), 0, 0           # page j of the call (over all batches) samples with splitmix64(base + j)
        feeder = self._feeder()
        marks, host0 = [], dict(feeder.stats, tokenize_s=self._tok_s)
        it = iter(image_batches)
        boxes_it = iter(boxes_batches) if boxes_batches is not None else None

        def pull():
            images = next(it, None)
            if images is None:
                return None
            images = list(images)
            return [images, (next(boxes_it) if boxes_it is not None else None), feeder.decode(images), None]

        def tile(item):
            """uploads + tile kernels of a pulled batch on the feeder's stream; a failure is kept for the batch's own turn"""
            if item is not None and item[3] is None:
                try:
                    item[3] = feeder.tiles(item[2], item[1], detect_model, use_p, errors)
                except Exception as e:
                    item[3] = e
        import collections
        ahead = collections.deque()              # pulled batches, oldest first: [0] next to run (tiled while its predecessor ran), [1] decoding

        def fill():
            while len(ahead) < 2:
                item = pull()
                if item is None:
                    return
                ahead.append(item)
        try:
            fill()
            while ahead:
                cur = ahead.popleft()
                tile(cur)
                page0 += n_prev                                 # counted before anything can fail: a failed batch's pages keep their place
                n_prev = len(cur[0])
                try:
                    if isinstance(cur[3], Exception):
                        raise cur[3]
                    embeds, meta = self._ocr_embeds(tokenizer, None, cur[0], question, generation_config, None, use_p, drop_zero, hard_vq,
                                                    IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN, ALIGNED_TOKEN, tiles=cur[3], errors=errors,
                                                    mark=marks if stats is not None else None)
                except Exception:
                    # this batch fails as a whole (errors='raise', or the visual stage itself): the batch before it is still decoding and its responses are good --
                    # they are handed out first, then the failure surfaces (folder mode re-runs exactly the failing batch page by page)
                    if pending is not None:
                        done, pending = pending, None
                        yield self._answer(tokenizer, pipe.finish(), done, return_scores)
                    raise
                # batch i+1's tiles BEFORE this thread blocks for batch i-1's decode: when it comes back the compute stream is close to the end of batch i's
                # prefill, and the first kernel of batch i+1 must not wait for 64 uploads to be issued (measured: 40-60 ms of idle compute stream per batch)
                if ahead:
                    tile(ahead[0])
                fill()                                          # batch i+2: its files start decoding
                if not embeds:                                  # nothing of this batch reached the language model
                    if pending is not None:
                        yield self._answer(tokenizer, pipe.finish(), pending, return_scores)
                        pending = None
                    yield self._answer(tokenizer, [], meta, return_scores)
                    continue
                if pipe is None:
                    pipe = self.page_pipeline(max_new_tokens=meta['max_new'], eos_token_id=meta['eos'], repetition_penalty=repetition_penalty)
                prev = pipe.start(embeds, sampling=meta['sampling'],
                                  seeds=[splitmix64(base + page0 + i) for i in meta['ok']] if sampled else None, logprobs=lpn,
                                  constraints=meta['constraints'])
                if stats is not None:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record(torch.cuda.current_stream())
                    marks.append(('end', e))
                if pending is not None:
                    yield self._answer(tokenizer, prev, pending, return_scores)
                pending = meta
            if pending is not None:
                done, pending = pending, None
                yield self._answer(tokenizer, pipe.finish(), done, return_scores)
        finally:
            for item in ahead:
                if item is not None:
                    for f in item[2]:
                        f.cancel()
            if pipe is not None:
                pipe.close()
            if stats is not None:
                torch.cuda.current_stream().synchronize()
                idle, last_end = [], None
                for kind, e in marks:
                    if kind == 'begin' and last_end is not None:
                        idle.append(round(last_end.elapsed_time(e), 2))
                    elif kind == 'end':
                        last_end = e
                stats['compute_stream_idle_ms_between_batches'] = idle
                stats['host'] = {k: v - host0[k] for k, v in dict(feeder.stats, tokenize_s=self._tok_s).items()}       # this call's share of the feeder's counters

    def chat_ocr_continuous(self, tokenizer, detect_model, images, question, generation_config, boxes_list=None, use_p=True, drop_zero=False,
                            hard_vq=False, repetition_penalty=1.5, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>', IMG_CONTEXT_TOKEN='<IMG_CONTEXT>',
                            ALIGNED_TOKEN='[UNUSED_TOKEN_140]', slots=64, admit_group=16, visual_group=16, errors='raise', stats=None,
                            return_scores=False, draft=None):
        """chat_ocr_pages over any number of pages with continuous batching (continuous.ContinuousPipeline): a generator that yields
        (index into `images`, response) as pages finish -- a page that stops early frees its decode row for the next page at once, instead of
        waiting for the longest page of a batch.  The visual stage runs `visual_group` pages at a time ahead of admission (the next group's files
        are decoded on pageio.PageFeeder's threads meanwhile); prefill admits up to `admit_group` pages at once into `slots` decode rows.  Every
        response is the one the page's own chat_ocr call gives.  errors='return': a page whose own chat_ocr call would raise before generation
        yields that exception (chat_ocr_pages' semantics; when a group's visual stage fails as a whole, its pages are retried one by one).
        stats (a dict) receives the pipeline's counters.  return_scores (True, or the number of alternatives per token): yields
        (index, response, scores.ResponseScores), the scores None for a page that failed."""
        if parse_beams(generation_config) is not None:
            raise NotImplementedError('chat_ocr_continuous: beam search does not go through ContinuousPipeline (use chat_ocr_pages)')
        if parse_share(generation_config):
            refuse_share('ContinuousPipeline (chat_ocr_continuous: it owns its caches and refills rows one page at a time)')
        if draft is not None:
            drafting.refuse('ContinuousPipeline (chat_ocr_continuous: its rows stop on the device, its worker never waits for a step)')
        if parse_returns(dict(generation_config)) > 1:
            raise NotImplementedError('chat_ocr_continuous: num_return_sequences > 1 does not go through ContinuousPipeline, which owns its caches '
                                      '(use chat_ocr_pages)')
        from .continuous import ContinuousPipeline
        _, lpn = self._score_args(generation_config, return_scores)
        images = list(images)
        feeder = self._feeder()
        groups = [list(range(i, min(len(images), i + visual_group))) for i in range(0, len(images), visual_group)]

        def pull(g):
            return feeder.decode([images[i] for i in g]) if g is not None else None

        def embed(idx, decoded):
            bx = [boxes_list[i] for i in idx] if boxes_list is not None else None
            tiles = feeder.tiles(decoded, bx, detect_model, use_p, errors)
            return self._ocr_embeds(tokenizer, None, [images[i] for i in idx], question, generation_config, None, use_p, drop_zero, hard_vq,
                                    IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN, ALIGNED_TOKEN, tiles=tiles, errors=errors)
        template = get_conv_template(self.template)
        gc = dict(generation_config, eos_token_id=tokenizer.convert_tokens_to_ids(template.sep))      # what _ocr_embeds gives every page
        max_new, eos, sp = self._gen_args(gc)
        cons = constraints_parse(gc, eos)
        seeds = page_seeds(len(images)) if sp is not None else None
        failed = []

        def items():
            nxt = pull(groups[0]) if groups else None
            for gi, idx in enumerate(groups):
                cur, nxt = nxt, pull(groups[gi + 1]) if gi + 1 < len(groups) else None
                try:
                    parts = [(idx, embed(idx, cur))]
                except Exception:
                    if errors != 'return' or len(idx) == 1:
                        raise
                    parts = []
                    for i in idx:                       # the group failed as a whole: each page on its own, with its own exception
                        try:
                            parts.append(([i], embed([i], pull([i]))))
                        except Exception as e:
                            failed.append((i, e))
                for sub, (embeds, meta) in parts:
                    failed.extend((sub[k], e) for k, e in meta['failed'].items())
                    for k, emb in zip(meta['ok'], embeds):
                        yield sub[k], emb, None, sp, (seeds[sub[k]] if sp is not None else None), lpn, cons

        def response(ids):
            return reply_text(tokenizer, ids, template.sep)
        if not images:
            return
        pipe = ContinuousPipeline(self, slots=slots, max_new_tokens=max_new, eos_token_id=eos, repetition_penalty=repetition_penalty,
                                  admit_group=admit_group)
        try:
            fail = (lambda f: tuple(f) + (None,)) if return_scores else (lambda f: f)
            for i, ids in pipe.map(items(), errors=errors):
                while failed:
                    yield fail(failed.pop(0))
                if isinstance(ids, BaseException):
                    yield fail((i, ids))
                elif return_scores:
                    yield i, response(ids[0]), ResponseScores.build(tokenizer, *ids)
                else:
                    yield i, response(ids)
            while failed:
                yield fail(failed.pop(0))
        finally:
            if stats is not None:
                stats.update(pipe.stats)
            pipe.close()

    def _feeder(self):
        if getattr(self, '_pagefeeder', None) is None:
            from .pageio import PageFeeder
            self._pagefeeder = PageFeeder(self)
            if getattr(self, '_tok_cache', None) is None:
                self._tok_cache, self._tok_s = {}, 0.0
        return self._pagefeeder

    def _prompt_ids(self, tokenizer, q, n_tiles, n_ref, IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN, ALIGNED_TOKEN):
        """ids of one page's prompt = tokenizer(query of chat_ocr, :690-726).  A page prompt is ~40 KB of text of which all but ~100 characters are two RUNS of one
        added token each (256 x tiles <IMG_CONTEXT>, n_ref [UNUSED_TOKEN_140] appended to the question): tokenizers split added tokens out first and
        tokenise the stretches between them on their own, so the ids are those of the SKELETON (both runs at length one) with the two ids repeated.
        The skeleton is tokenised once per question; the FIRST page of every skeleton is also tokenised in full and compared -- a tokenizer for which the
        shortcut does not hold keeps the full path."""
        t0 = time.perf_counter()
        if getattr(self, '_tok_cache', None) is None:
            self._tok_cache, self._tok_s = {}, 0.0
        ctx = IMG_CONTEXT_TOKEN * (self.num_image_token * n_tiles)
        appended = n_ref is not None and ALIGNED_TOKEN not in q
        def full():
            query, _, _ = self._build_query(q + ALIGNED_TOKEN * n_ref if appended else q, None, [n_tiles], IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN)
            return tokenizer(query, return_tensors='pt')['input_ids'].reshape(-1)
        ids = None
        if n_tiles > 0 and (not appended or n_ref > 0) and IMG_CONTEXT_TOKEN not in q:
            skel, _, _ = self._build_query(q + ALIGNED_TOKEN if appended else q, None, [n_tiles], IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN)
            skel = skel.replace(ctx, IMG_CONTEXT_TOKEN, 1)
            key = (id(tokenizer), skel, appended)
            ent = self._tok_cache.get(key)
            if ent is None:
                sid = tokenizer(skel, return_tensors='pt')['input_ids'].reshape(-1)
                pi = (sid == self.img_context_token_id).nonzero().reshape(-1)
                pr = (sid == self.aligned_token_id).nonzero().reshape(-1)
                ent = False
                if pi.numel() == 1 and (not appended or (pr.numel() == 1 and int(pr[0]) > int(pi[0]))):
                    ent = (sid, int(pi[0]), int(pr[0]) if appended else None)
                if ent:
                    ref = full()
                    if not torch.equal(self._expand(ent, n_tiles, n_ref), ref):
                        ent = False
                    ids = ref
                if len(self._tok_cache) > 256:
                    self._tok_cache.clear()
                self._tok_cache[key] = ent
            if ent and ids is None:
                ids = self._expand(ent, n_tiles, n_ref)
        if ids is None:
            ids = full()
        self._tok_s += time.perf_counter() - t0
        return ids

    def _expand(self, ent, n_tiles, n_ref):
        sid, pi, pr = ent
        img = torch.full((self.num_image_token * n_tiles,), self.img_context_token_id, dtype=sid.dtype)
        if pr is None:
            return torch.cat([sid[:pi], img, sid[pi + 1:]])
        return torch.cat([sid[:pi], img, sid[pi + 1:pr], torch.full((n_ref,), self.aligned_token_id, dtype=sid.dtype), sid[pr + 1:]])

    def _ocr_embeds(self, tokenizer, detect_model, images, question, generation_config, boxes_list, use_p, drop_zero, hard_vq,
                    IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN, ALIGNED_TOKEN, tiles=None, errors='raise', mark=None, allow_returns=False):
        """Everything of chat_ocr_pages before the language model: the pages' prompt embeddings with both splices done, and
        meta = {n, ok: batch indices of the pages in `embeds`, failed: {index: exception}, max_new, eos, template}.  The host side (decode, boxes, tiles) is
        pageio.PageFeeder's; nothing on this thread's stream waits for a pageable copy."""
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        feeder = self._feeder()
        batch = tiles if tiles is not None else feeder.tiles(feeder.decode(images), boxes_list, detect_model, use_p, errors)
        template = get_conv_template(self.template)
        generation_config = dict(generation_config)
        generation_config['eos_token_id'] = tokenizer.convert_tokens_to_ids(template.sep)
        max_new, eos, sp = self._gen_args(generation_config, allow_beams=True, allow_returns=allow_returns)      # (the pipelines that call this have refused beams on entry)
        meta = {'n': len(images), 'ok': [], 'failed': dict(batch.failed), 'max_new': max_new, 'eos': eos, 'template': template, 'sampling': sp,
                'constraints': constraints_parse(generation_config, eos)}
        if not batch.ok:
            return [], meta
        feeder.hand_over(batch)
        if mark is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream())
            mark.append(('begin', e))
        feats = self.extract_feature(batch.page_px)
        if use_p:
            feat_c = self.extract_feature(batch.char_px)
            rs = self.resampler(feat_c)
            outs = self.engine.vq(rs, with_cos=hard_vq)
            idx, cos = outs if hard_vq else (outs, None)
        q = question if '<image>' in question else '<image>\n' + question
        refs, all_ids, coff = [], [], 0
        for k in range(len(batch.ok)):
            ref = None
            if use_p:
                sl = slice(coff, coff + batch.n_chars[k])
                ref = self.engine.denorm(rs[sl], idx[sl], cos[sl] if cos is not None else None, drop_zero=drop_zero, hard_vq=hard_vq)
                coff += batch.n_chars[k]
            refs.append(ref)
            all_ids.append(self._prompt_ids(tokenizer, q, batch.n_tiles[k], ref.shape[0] if use_p else None, IMG_START_TOKEN, IMG_END_TOKEN,
                                            IMG_CONTEXT_TOKEN, ALIGNED_TOKEN))
        ids_dev = torch.cat(all_ids).pin_memory().to(self.device, non_blocking=True)          # ONE asynchronous upload for the batch's prompts
        embeds, toff, ioff = [], 0, 0
        for k, i in enumerate(batch.ok):
            S = all_ids[k].numel()
            try:
                check_fits(S, max_new, self.max_tokens)                         # _generate's check, per page
            except ValueError as err:
                if errors == 'raise':
                    raise
                meta['failed'][i] = err
            else:
                embeds.append(self.engine.embed_splice(ids_dev[ioff:ioff + S], feats[toff:toff + batch.n_tiles[k]], refs[k], img_id=self.img_context_token_id,
                                                       ref_id=self.aligned_token_id))
                meta['ok'].append(i)
            toff += batch.n_tiles[k]
            ioff += S
        return embeds, meta

    def batch_chat(self, tokenizer, pixel_values, questions, generation_config, num_patches_list=None, history=None,
                   return_history=False, IMG_START_TOKEN='<img>', IMG_END_TOKEN='</img>', IMG_CONTEXT_TOKEN='<IMG_CONTEXT>',
                   verbose=False, image_counts=None, return_scores=False):
        """:903-951.  return_scores: returns (responses, [scores.ResponseScores per question]).  The reference left-pads and runs one padded batch; here every query is prefilled at its own
        length and the pages then decode together (cr_llm_decode), which gives each row exactly its unpadded result."""
        if history is not None or return_history:
            print('Now multi-turn chat is not supported in batch_chat.')
            raise NotImplementedError
        if image_counts is not None:
            num_patches_list = image_counts
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        generation_config, lpn = self._score_args(generation_config, return_scores)
        embeds, off = [], 0
        feats = self.extract_feature(pixel_values) if pixel_values is not None else None
        for idx, num_patches in enumerate(num_patches_list):
            question = questions[idx]
            if pixel_values is not None and '<image>' not in question:
                question = '<image>\n' + question
            query, template, _ = self._build_query(question, None, [num_patches], IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN)
            ids = tokenizer(query, return_tensors='pt')['input_ids'].reshape(-1)
            embeds.append(self.engine.embed_splice(ids, feats[off:off + num_patches] if feats is not None else None,
                                                   img_id=self.img_context_token_id))
            off += num_patches
        generation_config['eos_token_id'] = tokenizer.convert_tokens_to_ids(template.sep)
        max_new, eos, sp = self._gen_args(generation_config)
        outs = self.generate_pages(embeds, max_new, eos, generation_config.get('repetition_penalty', 1.0), sampling=sp,
                                   seeds=page_seeds(len(embeds)) if sp is not None else None, logprobs=lpn,
                                   constraints=constraints_parse(generation_config, eos))
        outs, tss = outs if lpn else (outs, None)
        responses = [reply_text(tokenizer, o, template.sep) for o in outs]
        return (responses, [ResponseScores.build(tokenizer, o, ts) for o, ts in zip(outs, tss)]) if return_scores else responses

    # ---- page-parallel generation (new: the reference decodes one page at a time) ---------------
    def page_pipeline(self, **kw):
        """A PagePipeline over this model: batches of pages with the decode of one batch beside the visual stage of the next."""
        return PagePipeline(self, **kw)

    def generate_pages(self, embeds_list, max_new_tokens=1024, eos_token_id=EOS_TOKEN_ID, repetition_penalty=1.0,
                       check_every=16, prefill_batch=16, sampling=None, seeds=None, logprobs=0, num_beams=1, length_penalty=1.0, early_stopping=False,
                       constraints=None, drafts=None, num_return_sequences=1, share_prompt=False):
        """Prefill every page, then decode all unfinished pages as ONE batch per step: the 14.7 GB of LLM weights are
        streamed once per step for all pages.  Per page the ids equal the single-page greedy result.
        sampling: None (every page greedy), one sampling.SamplingParams for every page, or a list with one entry (or None: greedy) per page;
        seeds: one 64-bit seed per page (default page_seeds(P)).  A sampled page's ids depend only on its prompt, its parameters and its seed.
        logprobs: 0 (the return value is the list of id lists), an int n in 1..8 for every page, or one int per page.  When any is non-zero the
        return value is (ids, scores): scores[i] is the page's scores.TokenScores with its n alternatives per id, cut like its ids, or None for a
        page with 0.  A page's scores, like its ids, do not depend on the batch it decodes in.
        num_beams > 1 (with length_penalty and early_stopping, validated as sampling.parse_beams does): beam search, every page's B beams as B rows of the one decode
        batch (P * B <= 64).  The return value is then (ids, sequences_scores): per page the best finished hypothesis, EOS included, and its score.  No
        sampling and no token scores with beams.
        constraints: None, one constraints.Constraints for every page, or a list with one entry (or None) per page: the page's picks choose among the
        ids its constraints leave (csrc/constrain.hip).  Greedy pages only; a page's ids do not depend on the batch it decodes in, and the other pages of
        the batch keep their ids bit for bit.
        drafts: None, or a list with one entry per page -- a list of ids that guesses the page's answer, or None -- checked several per decode step
        (generation.decode_rows_drafted); every page's ids are what they are without drafts.  Greedy pages on a bf16 cache, without scores, constraints
        or beams.
        num_return_sequences = n > 1: n sampled answers per page from ONE prefill of it (_generate_pages_fanout; P * n <= 64).  The return value nests:
        ids[i][j] is sample j of page i -- exactly what this call gives for page i alone with seeds=[seeds[i * n + j]] -- and with logprobs the scores
        nest the same way.  seeds: P * n entries (default page_seeds(P * n): sampling.fan_seeds).  Sampled pages on a bf16 cache, without constraints,
        drafts or beams.
        share_prompt=True: with beams or num_return_sequences > 1 the call's cache shares each page's prompt between its rows instead of copying it
        (KVCache.set_prefix_sharing: the fan-out copies the last < 256 positions only, and each decode step loads the shared part once per page); ids, scores
        and sequences_scores are the same, bit for bit.  With one row per page it is accepted and does nothing.  Not with drafts or an e4m3 cache."""
        share = parse_share(dict(share_prompt=share_prompt))
        if share and drafts is not None:
            refuse_share('drafts')
        if share and self.kv_cache_dtype != 'bf16':
            refuse_share("kv_cache_dtype='e4m3'")
        P = len(embeds_list)
        cons = constraints_per_page(constraints, P)
        beams = parse_beams(dict(num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping))
        sps = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling] * P
        nret = 1                                    # (1: today's path, nothing new is parsed)
        if not (num_return_sequences is None or (type(num_return_sequences) is int and num_return_sequences == 1)):
            nret = parse_returns(dict(num_return_sequences=num_return_sequences, num_beams=num_beams, do_sample=bool(sps) and all(sp is not None for sp in sps)))
        if nret > 1:
            if drafts is not None:
                drafting.refuse(f'num_return_sequences={nret} (sampled answers)')
            if any(c is not None for c in cons):
                raise NotImplementedError('generate_pages: logits constraints on a sampled page are not implemented (greedy decoding only)')
            return self._generate_pages_fanout(embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, sps, seeds,
                                               scores_per_page(logprobs, P), nret, share)
        if drafts is not None:
            if len(drafts) != P:
                raise ValueError(f'drafts: {len(drafts)} entries for {P} pages')
            if beams is not None:
                drafting.refuse(f'num_beams={beams.num_beams}')
            if sampling is not None:
                drafting.refuse('do_sample=True (sampling=)')
            if logprobs and any(scores_per_page(logprobs, P)):
                drafting.refuse('token scores (logprobs=)')
            if any(c is not None for c in cons):
                drafting.refuse('logits constraints')
            if self.kv_cache_dtype != 'bf16':
                drafting.refuse("an e4m3 KV cache (kv_cache_dtype='e4m3')")
        if beams is not None:
            if sampling is not None or (logprobs and any(scores_per_page(logprobs, P))):
                raise NotImplementedError('generate_pages: beam search takes neither sampling nor token scores')
            if any(c is not None for c in cons):
                raise NotImplementedError('generate_pages: logits constraints with beam search are not implemented (greedy decoding only)')
            return self._generate_pages_beams(embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, beams, share)
        per_page = per_page_sampling(sampling, seeds, P)
        lpn = scores_per_page(logprobs, P)
        kv, seqs = self.kv(P), list(range(P))
        admit(self.engine, kv, seqs, embeds_list, repetition_penalty, per_page, lpn, prefill_batch, constraints=cons)
        if drafts is not None:
            self.draft_stats = {}
            return decode_rows_drafted(self.engine, kv, seqs, max_new_tokens, eos_token_id, repetition_penalty, drafts, stats=self.draft_stats)
        outs = decode_rows(self.engine, kv, seqs, max_new_tokens, eos_token_id, repetition_penalty, check_every)
        return (outs, read_scores(kv, lpn, outs)) if any(lpn) else outs

    @torch.no_grad()
    def score_pages(self, embeds_list, answer_ids_list, repetition_penalty=1.0, logprobs=0, eos_token_id=EOS_TOKEN_ID, score_eos=True):
        """The batched twin of generate_pages for texts the caller brings: page i's prompt rows embeds_list[i] are followed by the embeddings of
        answer_ids_list[i], and ONE prefill-shaped pass (cr_llm_score_batch) scores every answer id -- and eos_token_id behind it unless score_eos is False
        or there is none -- by the definition of `logprobs=` in generate_pages: the log-softmax of the LM-head row after the repetition penalty over the
        answer ids before it.  Returns (ids, scores): per page the scored ids and a scores.TokenScores with `logprobs` (0..8) alternatives per id.
        A bf16 cache; nothing is generated."""
        P = len(embeds_list)
        if len(answer_ids_list) != P:
            raise ValueError(f'score_pages: {len(answer_ids_list)} answers for {P} pages')
        penalty, top_n = scoring.check_penalty(repetition_penalty), scoring.top_n_of(logprobs)
        if self.kv_cache_dtype != 'bf16':
            raise NotImplementedError("scoring continues a prefill in bf16: an e4m3 KV cache (kv_cache_dtype='e4m3') is not scored")
        es = [e.reshape(-1, e.shape[-1]) for e in embeds_list]
        plans = [scoring.plan(e.shape[0], a, eos_token_id, score_eos, self.dims.vocab) for e, a in zip(es, answer_ids_list)]
        for e, pl in zip(es, plans):
            scoring.check_fits(e.shape[0] + len(pl.feed), 0, self.max_tokens)
        kv, seqs = self.kv(P), list(range(P))
        for s in seqs:
            kv.reset(s)
        rows = [torch.cat([e, self.engine.embed_splice(torch.tensor(pl.feed, dtype=torch.long))], dim=0) if pl.feed else e for e, pl in zip(es, plans)]
        ts = self.engine.score_batch(kv, seqs, rows, [pl.targets for pl in plans], penalty=penalty, top_n=top_n)
        return [pl.ids for pl in plans], ts

    @torch.no_grad()
    def score_ocr(self, tokenizer, detect_model, img_path, question, answer, generation_config=None, repetition_penalty=1.5, top_logprobs=1, history=None,
                  use_p=True, drop_zero=False, hard_vq=False, boxes=None, score_eos=True, draft=None, verbose=False):
        """What the model thinks of `answer` (a string, or a list of ids) as the reply chat_ocr would give to `question` about the page: the visual stage and
        the prompt are chat_ocr's, the answer's ids and the end-of-turn id behind them (score_eos) are scored in one pass.  Returns a scores.ResponseScores
        as chat_ocr(return_scores=top_logprobs) does for a reply it generated -- for the ids chat_ocr generates the numbers agree to within the bf16 noise
        of two kernel paths -- with total_logprob for ranking candidates.  generation_config may carry nothing that steers a generation (do_sample,
        num_beams > 1, constraints) and there is no draft: ValueError."""
        gc = scoring.refuse_generation(generation_config, draft, 'score_ocr')
        top_n, penalty = scoring.top_n_of(top_logprobs), scoring.check_penalty(repetition_penalty)
        page, pixel_values = self._open_page(img_path)
        out_tokens = None
        if use_p:
            out_tokens, _ = self.calli_align(page, detect_model, drop_zero=drop_zero, use_hard_vector_quant=hard_vq, verbose=verbose, boxes=boxes)
        _, _, _, model_inputs, gc = self._ocr_prompt(tokenizer, question, history, len(pixel_values), out_tokens, use_p, None, gc, False)
        ids = model_inputs['input_ids'].reshape(-1)
        prompt = self.engine.embed_splice(ids, self.extract_feature(pixel_values), out_tokens if use_p else None,
                                          img_id=self.img_context_token_id, ref_id=self.aligned_token_id)
        toks, ts = self.score_pages([prompt], [scoring.answer_to_ids(tokenizer, answer)], penalty, top_n, eos_token_id=gc['eos_token_id'], score_eos=score_eos)
        return scoring.response_scores(tokenizer, toks[0], ts[0])

    @torch.no_grad()
    def ground_pages(self, embeds_list, answer_ids_list, spans_list, layers=None, repetition_penalty=1.0, logprobs=None, eos_token_id=EOS_TOKEN_ID,
                     score_eos=True):
        """The twin of score_pages that also says WHERE every scored id's row looked: spans_list[i] = [(start, end), ...] ranges of page i's prompt positions
        (grounding.spans_of finds the character boxes' pseudo-token runs), and ONE prefill-shaped pass (cr_llm_ground_batch) gives per scored id the
        attention probability its row put on every span, averaged over the heads and over `layers` = (layer0, layer1), None: all layers.  Which layers ground
        best can only be learned on a real checkpoint: no default is tuned here.  logprobs: None (no LM head runs), or 0..8 alternatives per id for the scores
        of the same pass.  Returns (ids, masses, scores): per page the scored ids, a float32 CPU tensor [T, spans] and a scores.TokenScores (None without
        logprobs).  A bf16 cache; nothing is generated."""
        P = len(embeds_list)
        if len(answer_ids_list) != P or len(spans_list) != P:
            raise ValueError(f'ground_pages: {len(answer_ids_list)} answers and {len(spans_list)} span lists for {P} pages')
        penalty = scoring.check_penalty(repetition_penalty)
        top_n = 0 if logprobs is None else scoring.top_n_of(logprobs)
        if self.kv_cache_dtype != 'bf16':
            raise NotImplementedError("grounding continues a prefill in bf16: an e4m3 KV cache (kv_cache_dtype='e4m3') is not grounded")
        es = [e.reshape(-1, e.shape[-1]) for e in embeds_list]
        plans = [scoring.plan(e.shape[0], a, eos_token_id, score_eos, self.dims.vocab) for e, a in zip(es, answer_ids_list)]
        spans = [grounding.check_spans(sp, e.shape[0] + len(pl.feed)) for sp, e, pl in zip(spans_list, es, plans)]
        layers = grounding.check_layers(layers, self.dims.llm_layers)
        for e, pl in zip(es, plans):
            scoring.check_fits(e.shape[0] + len(pl.feed), 0, self.max_tokens)
        kv, seqs = self.kv(P), list(range(P))
        for s in seqs:
            kv.reset(s)
        rows = [torch.cat([e, self.engine.embed_splice(torch.tensor(pl.feed, dtype=torch.long))], dim=0) if pl.feed else e for e, pl in zip(es, plans)]
        ts, ms = self.engine.ground_batch(kv, seqs, rows, [pl.targets for pl in plans], spans, layers=layers, penalty=penalty, top_n=top_n,
                                          want_scores=logprobs is not None)
        return [pl.ids for pl in plans], ms, ts

    @torch.no_grad()
    def ground_ocr(self, tokenizer, detect_model, img_path, question, answer=None, generation_config=None, layers=None, repetition_penalty=1.5,
                   top_logprobs=None, history=None, use_p=True, drop_zero=False, hard_vq=False, boxes=None, score_eos=True, draft=None, verbose=False):
        """Which character box every id of the reply came from.  answer (a string, or a list of ids): the text is the caller's, and the call works like
        score_ocr -- one pass over prompt ++ answer.  answer=None: the reply is generated greedily as chat_ocr generates it (one visual stage, one prompt
        prefill), the sequence is rolled back to the prompt's last row (cr_kv_truncate(seq, L - 1)) and the generated ids are grounded over the cached prompt
        by one continued prefill of T + 1 rows.  The boxes are taken here (`boxes=`, or ordering.acquire_boxes as calli_align takes them) and handed to
        calli_align, so the result carries the very boxes the pseudo-tokens were made from.  layers = (layer0, layer1), None: all layers -- which range
        grounds best can only be learned on a real checkpoint.  top_logprobs: None, or 0..8 for the scores of the same pass (Grounding.scores).
        Returns (response, grounding.Grounding).  Nothing that steers a generation (do_sample, num_beams > 1, constraints, a draft): ValueError; an e4m3 KV
        cache: NotImplementedError."""
        gc = scoring.refuse_generation(generation_config, draft, 'ground_ocr')
        penalty = scoring.check_penalty(repetition_penalty)
        top_n = None if top_logprobs is None else scoring.top_n_of(top_logprobs)
        if not use_p:
            raise ValueError('ground_ocr: use_p=False (the boxes reach the prompt as pseudo-tokens: there is nothing to ground on without them)')
        if self.kv_cache_dtype != 'bf16':
            raise NotImplementedError("grounding continues a prefill in bf16: an e4m3 KV cache (kv_cache_dtype='e4m3') is not grounded")
        n_layers = getattr(getattr(self, 'dims', None), 'llm_layers', None)
        if layers is not None and n_layers is not None:
            layers = grounding.check_layers(layers, n_layers)
        page, pixel_values = self._open_page(img_path)
        if boxes is None:
            from . import ordering
            boxes = ordering.acquire_boxes(detect_model, page, self.sorter)
        boxes = [[int(v) for v in b[:4]] for b in boxes]
        out_tokens, indices = self.calli_align(page, detect_model, drop_zero=drop_zero, use_hard_vector_quant=hard_vq, verbose=verbose, boxes=boxes)
        _, _, template, model_inputs, gc = self._ocr_prompt(tokenizer, question, history, len(pixel_values), out_tokens, use_p, None, gc, False)
        ids = model_inputs['input_ids'].reshape(-1)
        spans = grounding.check_spans(grounding.spans_of(ids, self.aligned_token_id, grounding.kept_per_box(indices) if drop_zero else 3))
        if len(spans) != len(boxes):
            raise ValueError(f'ground_ocr: the prompt holds the pseudo-tokens of {len(spans)} boxes, the page has {len(boxes)}')
        prompt = self.engine.embed_splice(ids, self.extract_feature(pixel_values), out_tokens, img_id=self.img_context_token_id, ref_id=self.aligned_token_id)
        if answer is not None:
            toks, ms, ts = self.ground_pages([prompt], [scoring.answer_to_ids(tokenizer, answer)], [spans], layers, penalty, top_n,
                                             eos_token_id=gc['eos_token_id'], score_eos=score_eos)
            y, mass, ts = toks[0], ms[0], ts[0]
            response = answer if isinstance(answer, str) else reply_text(tokenizer, torch.tensor([y], dtype=torch.long), template.sep)
        else:
            max_new, eos, _ = self._gen_args(gc)
            kv = self.kv(1)
            y = self._generate(prompt, max_new, eos, penalty, kv=kv, seq=0)[0].tolist()
            response = reply_text(tokenizer, torch.tensor([y], dtype=torch.long), template.sep)
            L = prompt.shape[0]
            scoring.check_fits(len(y), L - 1, self.max_tokens)
            kv.truncate(0, L - 1)
            rows = torch.cat([prompt[L - 1:], self.engine.embed_splice(torch.tensor(y[:-1], dtype=torch.long))], dim=0) if len(y) > 1 else prompt[L - 1:]
            tss, ms = self.engine.ground_batch(kv, [0], [rows], [y], [spans], layers=layers, penalty=penalty, top_n=top_n or 0, want_scores=top_n is not None)
            mass, ts = ms[0], tss[0]
        sc = scoring.response_scores(tokenizer, y, ts) if ts is not None else None
        return response, grounding.Grounding.build(y, mass.numpy(), spans, grounding.pieces_of(tokenizer, y), boxes,
                                                   layers if layers is not None else (0, n_layers or 0), grounding.special_ids_of(tokenizer), sc)

    def _generate_pages_fanout(self, embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, sps, seeds, lpn, n, share=False):
        """generate_pages with n > 1 sampled answers per page: page i is prefilled ONCE, into sequence fan_slots(i, n)[0] with the seed of its sample 0, and
        KVCache.fanout gives its other n - 1 sequences the cached prompt and each its own first id from the prefill's raw last row; the P * n rows then
        decode as one batch per step through decode_rows.  A decode row's bits do not depend on its batch and a draw depends only on (seed, step, row,
        history), so sample (i, j) is the lone call's answer for page i with seed seeds[i * n + j], id for id."""
        P = len(embeds_list)
        check_rows(P, n)
        if self.kv_cache_dtype != 'bf16':
            raise NotImplementedError(f"num_return_sequences={n} with kv_cache_dtype='e4m3': the fan-out copies bf16 rows (cr_kv_fanout); call the entry "
                                      'point n times, or use a bf16 cache')
        if seeds is None:
            seeds = [sd for row in fan_seeds(P, n) for sd in row]
        if len(seeds) != P * n:
            raise ValueError(f'seeds: {len(seeds)} entries for {P} pages x {n} returned sequences')
        for e in embeds_list:
            check_fits(e.shape[0], max_new_tokens, self.max_tokens)
        kv = self.kv(P * n)
        kv.reset()
        share_cache(kv, share)                     # share: fanout copies the last < 256 positions and the samples read the rest from sample 0's sequence
        try:
            return self._fanout_decode(kv, embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, sps, seeds, lpn, n)
        finally:
            if share:
                release_shared(kv, [fan_slots(i, n) for i in range(P)])

    def _fanout_decode(self, kv, embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, sps, seeds, lpn, n):
        """_generate_pages_fanout on a cache that has been reset: the prefills, the fan-outs, the decode, the read-back."""
        P = len(embeds_list)
        first = [fan_slots(i, n)[0] for i in range(P)]
        for i, sp in enumerate(sps):
            kv.set_sampling(first[i], sp.temperature, sp.top_k, sp.top_p, int(seeds[i * n]))
            if lpn[i]:
                kv.set_logprobs(first[i], lpn[i])
        for i0 in range(0, P, prefill_batch):
            idx = list(range(i0, min(P, i0 + prefill_batch)))
            rows = self.engine.prefill_batch(kv, [first[i] for i in idx], [embeds_list[i] for i in idx], penalty=repetition_penalty, want_logits=True)
            for k, i in enumerate(idx):
                kv.fanout(first[i], fan_slots(i, n)[1:], seeds[i * n + 1:(i + 1) * n], rows[k])
        outs = decode_rows(self.engine, kv, list(range(P * n)), max_new_tokens, eos_token_id, repetition_penalty, check_every)
        ids = [outs[i * n:(i + 1) * n] for i in range(P)]
        if not any(lpn):
            return ids
        ts = read_scores(kv, [m for m in lpn for _ in range(n)], outs)
        return ids, [ts[i * n:(i + 1) * n] for i in range(P)]

    def _generate_pages_beams(self, embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, beams, share=False):
        """generate_pages with beam search: page i is the beam group of sequences beam_slots(i, B); the done flags are read every check_every steps,
        where the greedy loop reads EOS."""
        P, Bn = len(embeds_list), beams.num_beams
        if P * Bn > 64:
            raise ValueError(f'{P} pages x {Bn} beams = {P * Bn} decode rows: at most 64 (the batched decode kernels)')
        kv = self.kv(P * Bn)
        for e in embeds_list:
            check_fits(e.shape[0], max_new_tokens, self.max_tokens)
        kv.reset()
        share_cache(kv, share)                     # share: a group's fan-out copies the last < 256 positions and its beams read the rest from its first sequence
        try:
            return self._beams_decode(kv, embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, beams)
        finally:
            if share:
                release_shared(kv, [beam_slots(i, Bn) for i in range(P)])

    def _beams_decode(self, kv, embeds_list, max_new_tokens, eos_token_id, repetition_penalty, check_every, prefill_batch, beams):
        """_generate_pages_beams on a cache that has been reset: the groups, the prefills, the decode, the results."""
        P, Bn = len(embeds_list), beams.num_beams
        for i in range(P):
            kv.set_beam(beam_slots(i, Bn)[0], Bn, beams.length_penalty, beams.early_stopping, eos_token_id, max_new_tokens)
        for i0 in range(0, P, prefill_batch):
            idx = list(range(i0, min(P, i0 + prefill_batch)))
            self.engine.prefill_batch(kv, [beam_slots(i, Bn)[0] for i in idx], [embeds_list[i] for i in idx], penalty=repetition_penalty)
        live, res, n = list(range(P)), {}, 1

        def collect():
            for i in list(live):
                ids, score, done = kv.beam_result(beam_slots(i, Bn)[0])
                if done:
                    res[i] = (ids, score)
                    live.remove(i)
        if max_new_tokens <= 1:
            collect()
        while n < max_new_tokens and live:
            steps = min(check_every, max_new_tokens - n)
            rows = [s for i in live for s in beam_slots(i, Bn)]
            for _ in range(steps):
                self.engine.decode(kv, rows, penalty=repetition_penalty)
            n += steps
            collect()
        if live:
            raise RuntimeError(f'beam groups of pages {live} are still running after {max_new_tokens} tokens')
        return [res[i][0] for i in range(P)], [res[i][1] for i in range(P)]


def beam_slots(page, num_beams):
    """Cache sequences of page `page` when every page of a batch runs `num_beams` beams: consecutive, the group's first sequence first."""
    return list(range(page * num_beams, (page + 1) * num_beams))


def fan_slots(page, n):
    """Cache sequences of page `page` when every page of a batch returns `n` sampled answers: consecutive, the prefilled one (sample 0) first."""
    return list(range(page * n, (page + 1) * n))


def load_boxes_json(path):
    from .preprocess import boxes_from_labelme
    with open(path, 'r', encoding='utf-8') as f:
        return boxes_from_labelme(json.load(f))

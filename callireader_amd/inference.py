"""`python inference.py --tgt ...` with the reference's flags (/root/reference/inference.py:65-130), on the HIP engine.

The detector is what the reference uses: `ultralytics.YOLO(<params>/best.pt)` (inference.py:98), handed to chat_ocr as
is; everything behind it (repeated passes, de-duplication, column merge, OrderFormer, reading order) runs in this
package (ordering.py).  ultralytics is third-party and not part of this image: without it, or with --boxes / a
labelme-style `<image>.json` next to the image (the format of examples/0.json), the ordered boxes are read from JSON.
The tokenizer is the engine's own reader of the reference's tokenizer files under --model
(callireader_amd/tokenization_internlm2.py, pinned against the sentencepiece library in tests/test_tokenizer.py).
"""
import argparse
import json
import os

import torch

from .modeling_internvl_chat import InternVLChatModel, load_boxes_json

IMG_EXT = ('.jpg', '.jpeg', '.png', '.bmp', '.webp')


def _sniff(p):
    """imghdr.what of the reference's utils/utils.py:493-512 (a file is an image when its header says so); the module left the standard library in 3.13: by extension then."""
    try:
        import imghdr
    except ImportError:
        return 'by-extension' if p.lower().endswith(IMG_EXT) else None
    try:
        return imghdr.what(p)
    except Exception:
        return None


def is_image(p):
    return os.path.isfile(p) and _sniff(p) is not None


def get_image_paths(folder_path):
    """utils/utils.py:493-503: every file under the folder (recursively) whose header is an image's; sorted here, so that the batches and the JSON are reproducible."""
    return sorted(os.path.join(root, f) for root, _, files in os.walk(folder_path) for f in files if _sniff(os.path.join(root, f)) is not None)


def load_detector(params_dir='./params'):
    """inference.py:98 `YOLO(YOLO_CHECKPOINT)` (config/configu.py: ./params/best.pt) when ultralytics and the weights
    are present, else None (boxes then come from JSON)."""
    path = os.path.join(params_dir, 'best.pt')
    try:
        from ultralytics import YOLO
    except Exception:
        return None
    return YOLO(path) if os.path.exists(path) else None


def boxes_for(image_path, boxes_arg=None, required=True):
    cand = boxes_arg or os.path.splitext(image_path)[0] + '.json'
    if not os.path.exists(cand):
        if not required:
            return None
        raise FileNotFoundError(f'character boxes for {image_path}: no detector (ultralytics + params/best.pt) and no {cand} '
                                '(labelme-style, see examples/0.json)')
    return load_boxes_json(cand)


def single_rec(model, tokenizer, detect_model, generation_config, image_path, prompt, use_p, hard_vq, drop_zero, repetition_penalty, verbose,
               boxes=None, quiet=False, scores=0, draft=None):
    """scores = n > 0 (--scores): the page's token scores are taken with n alternatives; prints one more line (`confidence <c> min <p> at token <k>
    (<piece>)`) and returns (response, scores.ResponseScores).
    draft = 'align' (--draft): the page's CalliAlign indices draft its answer (chat_ocr(draft='align')); the same response, one more line (`draft: <s> decode
    steps for <n> ids, <a> of <d> drafted ids accepted`).
    generation_config['num_return_sequences'] = N > 1 (--num_return_sequences, with --do_sample): the response is the list of N sampled responses, printed
    one `Assistant[j]:` line each -- with scores, `total logprob <t>` and the summary line behind each -- and the scores are a list of N."""
    bx = None
    if use_p and (boxes is not None or detect_model is None):
        bx = boxes_for(image_path, boxes)
    out = model.chat_ocr(tokenizer, detect_model, image_path, prompt, generation_config, use_p=use_p, hard_vq=hard_vq,
                         drop_zero=drop_zero, repetition_penalty=repetition_penalty, return_history=True,
                         verbose=verbose, boxes=bx, **(dict(return_scores=scores) if scores else {}), **(dict(draft=draft) if draft else {}))
    response = out[0]
    if not quiet and isinstance(response, list):
        print(f'User: {prompt}')
        print_samples(response, out[2] if scores else None)
        return (response, out[2]) if scores else response
    if not quiet:
        print(f'User: {prompt}\nAssistant: {response}')
        if draft:
            st = model.draft_stats
            print(f"draft: {st['steps']} decode steps for {st['steps'] + st['accepted'] + 1} ids, {st['accepted']} of {st['drafted']} drafted ids accepted")
        if scores:
            print(out[2].summary_line())
    return (response, out[2]) if scores else response


def print_samples(responses, scores=None):
    """The N sampled responses of one page, one `Assistant[j]: <response>` line each; with scores `  total logprob <t> | <summary line>` under each."""
    for j, r in enumerate(responses):
        print(f'Assistant[{j}]: {r}')
        if scores is not None:
            print(f'  total logprob {scores[j].total_logprob:.4f} | {scores[j].summary_line()}')


def scores_json(sc):
    """to_json of a page's ResponseScores; of a list of them (N sampled responses) the list, each with its total_logprob."""
    return [x.to_json(total=True) for x in sc] if isinstance(sc, list) else sc.to_json()


def answer_scores_name(save_name):
    """The file of --score_answer: `.answer_scores.json` in place of the results name's `json` ending."""
    if not save_name.endswith('json'):
        save_name += '_result.json'
    return save_name[:-len('json')].rstrip('.') + '.answer_scores.json'


def score_rec(model, tokenizer, detect_model, generation_config, image_path, prompt, answer, save_name, use_p, hard_vq, drop_zero, repetition_penalty, verbose,
              boxes=None, scores=0):
    """--score_answer TEXT on a single image: what the model thinks of TEXT as its reply to `prompt` (model.score_ocr).  Prints `Scored: TEXT`, the
    scores' summary line and `total logprob <t> over <k> tokens`, writes {imagePath, prompt, answer, scores: ResponseScores.to_json(total=True)} to
    `save_name`, and returns the ResponseScores."""
    bx = None
    if use_p and (boxes is not None or detect_model is None):
        bx = boxes_for(image_path, boxes)
    gc = {k: v for k, v in generation_config.items() if k not in ('max_new_tokens',) and not (k == 'num_beams' and v == 1) and not (k == 'do_sample' and not v)}
    sc = model.score_ocr(tokenizer, detect_model, image_path, prompt, answer, gc, repetition_penalty=repetition_penalty, top_logprobs=scores or 1, use_p=use_p,
                         hard_vq=hard_vq, drop_zero=drop_zero, boxes=bx, verbose=verbose)
    print(f'Scored: {answer}')
    print(sc.summary_line())
    print(f'total logprob {sc.total_logprob:.4f} over {len(sc.kept)} tokens')
    os.makedirs(os.path.dirname(save_name) or '.', exist_ok=True)
    with open(save_name, 'w', encoding='utf-8') as f:
        json.dump({'imagePath': image_path, 'prompt': prompt, 'answer': answer, 'scores': sc.to_json(total=True)}, f, ensure_ascii=False, indent=4)
    return sc


def grounding_name(save_name):
    """The file of --ground / --ground_answer: `.grounding.json` in place of the results name's `json` ending."""
    if not save_name.endswith('json'):
        save_name += '_result.json'
    return save_name[:-len('json')].rstrip('.') + '.grounding.json'


def ground_rec(model, tokenizer, detect_model, generation_config, image_path, prompt, answer, save_name, use_p, hard_vq, drop_zero, repetition_penalty, verbose,
               boxes=None):
    """--ground (answer=None: the recognition itself, generated once and grounded over its cached prompt) / --ground_answer TEXT on a single image
    (model.ground_ocr): which character box every piece of the reply came from.  Prints the recognition as single_rec does (or `Grounded: TEXT`), then one
    `<piece> -> [x1, y1, x2, y2] <mass>` line per piece, and writes {imagePath, prompt, response, grounding: [{piece, box, mass}, ...]} to `save_name`.
    Returns (response, grounding.Grounding)."""
    bx = None
    if boxes is not None or detect_model is None:
        bx = boxes_for(image_path, boxes)
    gc = {k: v for k, v in generation_config.items() if not (k == 'num_beams' and v == 1) and not (k == 'do_sample' and not v)}
    if answer is not None:
        gc.pop('max_new_tokens', None)
    response, g = model.ground_ocr(tokenizer, detect_model, image_path, prompt, answer, gc, repetition_penalty=repetition_penalty, use_p=use_p,
                                   hard_vq=hard_vq, drop_zero=drop_zero, boxes=bx, verbose=verbose)
    print(f'User: {prompt}\nAssistant: {response}' if answer is None else f'Grounded: {answer}')
    for piece, box, mass in g.pairs():
        print(f'{piece} -> {box} {mass:.4f}')
    os.makedirs(os.path.dirname(save_name) or '.', exist_ok=True)
    with open(save_name, 'w', encoding='utf-8') as f:
        json.dump({'imagePath': image_path, 'prompt': prompt, 'response': response, 'grounding': g.to_json()}, f, ensure_ascii=False, indent=4)
    return response, g


DEFAULT_BATCH_PAGES = 64       # pages per decode batch in folder mode: the most rows the batched decode kernels take, and the batch the headline is measured on


def folder_rec(model, tokenizer, detect_model, generation_config, folder_path, prompt, save_name, use_p, hard_vq, drop_zero, repetition_penalty,
               verbose, batch_pages=DEFAULT_BATCH_PAGES, continuous=False, scores=0, draft=None):
    """inference.py:47-62: every image of the folder -> results JSON [{imagePath, prompt, response}], an image that fails -> "ERROR!" for that entry only.
    The reference calls chat_ocr image after image; here the images go through `chat_ocr_stream` in batches of `batch_pages` (two batches in flight, files
    decoded ahead on threads): each response is the one the image's own chat_ocr call gives, pages/s is what changes (batch_pages <= 1: the serial loop).
    Failures stay per image: a page that cannot be read, has no boxes JSON / no box, or whose prompt is too long is reported alone; if a batch fails as a whole
    its pages are run one by one, each in its own try/except, as the reference does.
    continuous=True: the images go through `chat_ocr_continuous` instead (`batch_pages` decode rows, a row refilled as soon as its page stops);
    the same responses, JSON and console lines.
    scores = n > 0 (--scores): a second file, the results JSON's name with `.scores.json` in place of its `json` ending, holds per image
    {imagePath, scores: ResponseScores.to_json() with n alternatives per token, or null for an image whose entry is "ERROR!"}; the results JSON itself is
    byte-identical to a run without it.
    draft = 'align' (--draft): image after image through chat_ocr(draft='align') -- the serial loop, whatever batch_pages says (the pipelines take no draft)."""
    if draft:
        batch_pages = 1
    paths = get_image_paths(folder_path)
    responses, page_scores = {}, {}
    skw = dict(return_scores=scores) if scores else {}

    def put(pic_path, r, sc=None):
        """one page's outcome: a response, an exception, or with scores the pair (response, ResponseScores)"""
        if scores and isinstance(r, tuple):
            r, sc = r
        responses[pic_path] = r
        page_scores[pic_path] = sc

    def one(pic_path):
        try:
            return single_rec(model, tokenizer, detect_model, generation_config, pic_path, prompt, use_p, hard_vq, drop_zero, repetition_penalty, verbose,
                              quiet=True, scores=scores, draft=draft)
        except Exception as e:                               # inference.py:55-57
            return e

    def record(pic_path, response):
        if isinstance(response, BaseException):
            print(f'An error has occured:\n{response}')
            response = 'ERROR!'
        if isinstance(response, list):
            print(f'User: {prompt}')
            print_samples(response, page_scores.get(pic_path) if scores else None)
        else:
            print(f'User: {prompt}\nAssistant: {response}')
        responses[pic_path] = response

    beams = max(generation_config.get('num_beams', 1) or 1, generation_config.get('num_return_sequences', 1) or 1)
    if beams > 1 and batch_pages > 1:
        # beam search, or several sampled answers per page: the pipelines decode one row per page, so the images go through chat_ocr_pages, as many pages
        # per batch as fit the decode rows with `beams` rows each; a batch that fails as a whole runs page by page, like the other modes
        boxes, ready = {}, []
        for pic_path in paths:
            try:
                boxes[pic_path] = boxes_for(pic_path) if (use_p and detect_model is None) else None
                ready.append(pic_path)
            except Exception as e:
                responses[pic_path] = e
        per = max(1, min(batch_pages, DEFAULT_BATCH_PAGES) // beams)
        for i in range(0, len(ready), per):
            b = ready[i:i + per]
            try:
                res = model.chat_ocr_pages(tokenizer, detect_model, b, prompt, generation_config,
                                           boxes_list=[boxes[p] for p in b] if (use_p and detect_model is None) else None, use_p=use_p, drop_zero=drop_zero,
                                           hard_vq=hard_vq, repetition_penalty=repetition_penalty, errors='return', **skw)
                for pic_path, r in zip(b, zip(*res) if scores else res):      # (with scores: (responses, scores) -> one pair per page)
                    put(pic_path, r)
            except NotImplementedError:
                raise                                            # an option beams or samples do not take: not a page's failure
            except Exception as e:
                print(f'[folder_rec] a batch failed as a whole ({e}); its {len(b)} pages run one by one')
                for pic_path in b:
                    put(pic_path, one(pic_path))
        for pic_path in paths:
            record(pic_path, responses[pic_path])
    elif continuous and batch_pages > 1:
        boxes, ready = {}, []
        for pic_path in paths:
            try:
                boxes[pic_path] = boxes_for(pic_path) if (use_p and detect_model is None) else None
                ready.append(pic_path)
            except Exception as e:
                responses[pic_path] = e
        try:
            for i, r, *sc in model.chat_ocr_continuous(tokenizer, detect_model, ready, prompt, generation_config,
                                                  boxes_list=[boxes[p] for p in ready] if (use_p and detect_model is None) else None, use_p=use_p,
                                                  drop_zero=drop_zero, hard_vq=hard_vq, repetition_penalty=repetition_penalty, slots=batch_pages,
                                                  errors='return', **skw):
                put(ready[i], r, *sc)
        except Exception as e:
            left = [p for p in ready if p not in responses]
            print(f'[folder_rec] continuous batching failed ({e}); its {len(left)} remaining pages run one by one')
            for pic_path in left:
                put(pic_path, one(pic_path))
        for pic_path in paths:
            record(pic_path, responses[pic_path])
    elif batch_pages <= 1 or not hasattr(model, 'chat_ocr_stream'):
        for pic_path in paths:
            put(pic_path, one(pic_path))
            record(pic_path, responses[pic_path])
    else:
        # boxes from JSON where there is no detector (single_rec's rule); a page without them fails alone, before the batch is formed
        boxes, ready = {}, []
        for pic_path in paths:
            try:
                boxes[pic_path] = boxes_for(pic_path) if (use_p and detect_model is None) else None
                ready.append(pic_path)
            except Exception as e:
                responses[pic_path] = e
        batches = [ready[i:i + batch_pages] for i in range(0, len(ready), batch_pages)]
        done = 0
        while done < len(batches):
            stream = model.chat_ocr_stream(tokenizer, detect_model, batches[done:], prompt, generation_config,
                                           boxes_batches=[[boxes[p] for p in b] for b in batches[done:]] if (use_p and detect_model is None) else None,
                                           use_p=use_p, drop_zero=drop_zero, hard_vq=hard_vq, repetition_penalty=repetition_penalty, errors='return', **skw)
            try:
                for res in stream:
                    res, scs = res if scores else (res, [None] * len(batches[done]))
                    for pic_path, r, sc in zip(batches[done], res, scs):
                        put(pic_path, r, sc)
                    done += 1
            except Exception as e:
                print(f'[folder_rec] a batch failed as a whole ({e}); its {len(batches[done])} pages run one by one')
                for pic_path in batches[done]:
                    put(pic_path, one(pic_path))
                done += 1
        for pic_path in paths:                               # the reference's console output and order
            record(pic_path, responses[pic_path])
    results = [{'imagePath': p, 'prompt': prompt, 'response': responses[p]} for p in paths]
    if not save_name.endswith('json'):
        save_name += '_result.json'
    with open(save_name, 'w', encoding='utf-8') as f:
        json.dump(results, f, ensure_ascii=False, indent=4)           # utils/utils.py:59-62 save_json
    if scores:
        doc = [{'imagePath': p, 'scores': None if (responses[p] == 'ERROR!' or page_scores.get(p) is None) else scores_json(page_scores[p])} for p in paths]
        with open(scores_name(save_name), 'w', encoding='utf-8') as f:
            json.dump(doc, f, ensure_ascii=False, indent=4)
    return results


def scores_name(save_name):
    """The scores file of a results file: `.scores.json` in place of the name's `json` ending (recognition.json -> recognition.scores.json)."""
    return save_name[:-len('json')].rstrip('.') + '.scores.json'


def beam_config(args):
    """The beam entries of generation_config from --num_beams / --length_penalty / --early_stopping; {} without --num_beams (the config stays as it was)."""
    if args.num_beams == 1:
        return {}
    cfg = dict(num_beams=args.num_beams)
    if args.length_penalty is not None:
        cfg['length_penalty'] = args.length_penalty
    if args.early_stopping is not None:
        cfg['early_stopping'] = {'false': False, 'true': True, 'never': 'never'}[args.early_stopping]
    return cfg


def build_parser():
    parser = argparse.ArgumentParser(description='args for inference task')
    parser.add_argument('--tgt', type=str, help='Recognition target')
    parser.add_argument('--prompt', type=str, default='这幅书法作品内容是什么？', help='Prompt for recognition')
    parser.add_argument('--save_name', type=str, default='recognition.json')
    parser.add_argument('--use_p', type=bool, default=True)          # type=bool kept: any non-empty string is truthy, as upstream
    parser.add_argument('--hard_vq', type=bool, default=False)
    parser.add_argument('--drop_zero', type=bool, default=False)
    parser.add_argument('--verbose', type=bool, default=False)
    parser.add_argument('--repetition_penalty', type=float, default=1.0)
    parser.add_argument('--model', type=str, default='InternVL', help='checkpoint dir (INTERNVL_PATH)')
    parser.add_argument('--params', type=str, default='./params')
    parser.add_argument('--boxes', type=str, default=None, help='labelme-style JSON with ordered character boxes')
    parser.add_argument('--max_new_tokens', type=int, default=1024, help='generation_config.max_new_tokens (inference.py:92-96: 1024)')
    parser.add_argument('--batch_pages', type=int, default=DEFAULT_BATCH_PAGES,
                        help='folder mode: pages per batch through chat_ocr_stream (two batches in flight; same responses as the serial loop, which 1 selects)')
    parser.add_argument('--continuous', action='store_true',
                        help='folder mode: continuous batching (chat_ocr_continuous): --batch_pages decode rows, each refilled as soon as its page stops; same responses')
    parser.add_argument('--fp8_decode', action='store_true', help='e4m3 weights for the decode (cr_enable_fp8_decode; off by default: the reference computes in bf16)')
    parser.add_argument('--fp8_mfma', type=int, nargs='?', const=1, default=0, choices=(0, 1, 2),
                        help='e4m3 x e4m3 matrix-core linears (cr_enable_fp8_mfma; off by default; a throughput option, not parity-preserving): 1 = the norm-fed linears of the ViT / projector / prefill, 2 = also ViT fc2 and the prefill\'s wo / w2')
    parser.add_argument('--do_sample', action='store_true', help='sample instead of the greedy default (transformers semantics: do_sample=True alone is top-50 sampling)')
    parser.add_argument('--temperature', type=float, default=None, help='with --do_sample (default 1.0)')
    parser.add_argument('--top_k', type=int, default=None, help='with --do_sample (default 50; 0: off)')
    parser.add_argument('--top_p', type=float, default=None, help='with --do_sample (default 1.0: off)')
    parser.add_argument('--num_return_sequences', type=int, default=1, metavar='N',
                        help='with --do_sample: N sampled answers per page from one visual stage and one prefill (pages x N <= 64 decode rows); the console prints '
                             'the N answers (with --scores their total log-probabilities), the results JSON holds the list of N as `response` (only when N > 1)')
    parser.add_argument('--share_prompt', action='store_true',
                        help="with --num_beams > 1 or --num_return_sequences > 1: a page's beams / samples read ONE cached copy of its prompt in decode instead of one "
                             'each (less cache traffic per step, the same responses bit for bit; bf16 cache only); with one row per page it does nothing')
    parser.add_argument('--seed', type=int, default=None, help='torch.manual_seed before the run: --do_sample output becomes reproducible')
    parser.add_argument('--num_beams', type=int, default=1, help='beam search with this many beams (2..8; transformers\' deterministic beam search, on the device); 1: the greedy default')
    parser.add_argument('--length_penalty', type=float, default=None, help='with --num_beams > 1: exponent of the hypothesis length a finished score is divided by (default 1.0)')
    parser.add_argument('--early_stopping', type=str, default=None, choices=('false', 'true', 'never'), help="with --num_beams > 1: generation_config.early_stopping (default false)")
    parser.add_argument('--no_repeat_ngram_size', type=int, default=0, metavar='N', help='greedy decoding: no n-gram of N ids appears twice in a response (transformers\' no_repeat_ngram_size; 0: off)')
    parser.add_argument('--min_new_tokens', type=int, default=0, metavar='N', help='greedy decoding: a response has at least N ids before it may end (0: off)')
    parser.add_argument('--fp8_kv', action='store_true',
                        help='e4m3 KV cache for the decode (kv_cache_dtype="e4m3": 0.52x the cache bytes; off by default; a throughput option, not parity-preserving)')
    parser.add_argument('--scores', type=int, nargs='?', const=1, default=0, choices=range(0, 9), metavar='N',
                        help='per-token log-probabilities with the N (default 1, at most 8) most likely alternatives: single image prints one more line '
                             '(confidence, the least certain token); folder mode writes <save_name minus json>.scores.json next to the results JSON, which does not change')
    parser.add_argument('--draft', action='store_true',
                        help="draft-verified decoding: the page's CalliAlign indices (vocabulary ids of its character boxes, in reading order) draft the answer and several "
                             'ids are checked per decode step; the same response in fewer steps where the draft is right (greedy only; needs --use_p; folder mode runs image after image)')
    parser.add_argument('--score_answer', type=str, default=None, metavar='TEXT',
                        help='single image: besides the recognition, score TEXT as the reply to --prompt (per-token log-probabilities of a text you bring: a ground '
                             'truth, a candidate); prints its confidence line and total log-probability and writes results/<save_name minus json>.answer_scores.json')
    parser.add_argument('--ground', action='store_true',
                        help='single image: ground the recognition -- which character box every piece of the response came from (attention mass of the piece\'s '
                             'row on the box\'s pseudo-tokens, averaged over heads and layers); prints one line per piece and writes '
                             'results/<save_name minus json>.grounding.json with "grounding": [{"piece", "box": [x1, y1, x2, y2], "mass"}, ...] (greedy only; needs --use_p)')
    parser.add_argument('--ground_answer', type=str, default=None, metavar='TEXT', help='single image: the same for TEXT as the reply to --prompt (a text you bring)')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not isinstance(args.tgt, str):
        raise ValueError(f'The target should a string, not a instance of {type(args.tgt)}!')
    from .tokenization_internlm2 import InternLM2Tokenizer
    folder = os.path.isdir(args.tgt) and args.batch_pages > 1
    model = InternVLChatModel.from_pretrained(args.model, params_dir=args.params, torch_dtype=torch.bfloat16,
                                              **(dict(max_pages=args.batch_pages) if folder else {}),
                                              **(dict(kv_cache_dtype='e4m3') if args.fp8_kv else {})).eval().cuda()
    if args.fp8_mfma:
        model.engine.enable_fp8_mfma(True, level=args.fp8_mfma)
    if args.fp8_decode:
        model.engine.enable_fp8_decode(True)
    # the engine's own reader of tokenizer.model (+ tokenizer_config.json / added_tokens.json): the reference's
    # AutoTokenizer path needs sentencepiece==0.2.0; any HF-style tokenizer object works with chat_ocr as well
    tokenizer = InternLM2Tokenizer.from_pretrained(args.model)
    # the reference hard-codes the pseudo-token placeholder's id (92537, modeling_internvl_chat.py:1100); read from the tokenizer it is the same number on the
    # reference's files and the right one on any other vocabulary
    tid = tokenizer.convert_tokens_to_ids('[UNUSED_TOKEN_140]')
    if isinstance(tid, int) and 0 < tid < model.dims.vocab and tid != tokenizer.sp_model.unk_id:
        model.aligned_token_id = tid
    generation_config = dict(num_beams=1, max_new_tokens=args.max_new_tokens, do_sample=False)
    if args.do_sample:
        generation_config['do_sample'] = True
        generation_config.update({k: getattr(args, k) for k in ('temperature', 'top_k', 'top_p') if getattr(args, k) is not None})
    if args.num_return_sequences != 1:
        generation_config['num_return_sequences'] = args.num_return_sequences
    generation_config.update(beam_config(args))
    generation_config.update(constraint_config(args))
    if args.share_prompt and (args.num_beams > 1 or args.num_return_sequences > 1):      # (one row per page: nothing to share, and the pipelines do not take the keyword)
        generation_config['share_prompt'] = True
    if args.seed is not None:
        torch.manual_seed(args.seed)
    detect_model = load_detector(args.params)
    if is_image(args.tgt) and (args.ground or args.ground_answer is not None):
        print('Single image recognition mode.')
        ground_rec(model, tokenizer, detect_model, generation_config, args.tgt, args.prompt, args.ground_answer,
                   grounding_name(os.path.join('results', args.save_name)), args.use_p, args.hard_vq, args.drop_zero, args.repetition_penalty, args.verbose, args.boxes)
    elif is_image(args.tgt):
        print('Single image recognition mode.')
        single_rec(model, tokenizer, detect_model, generation_config, args.tgt, args.prompt, args.use_p, args.hard_vq, args.drop_zero,
                   args.repetition_penalty, args.verbose, args.boxes, scores=args.scores, draft='align' if args.draft else None)
        if args.score_answer is not None:
            score_rec(model, tokenizer, detect_model, generation_config, args.tgt, args.prompt, args.score_answer,
                      answer_scores_name(os.path.join('results', args.save_name)), args.use_p, args.hard_vq, args.drop_zero, args.repetition_penalty, args.verbose,
                      args.boxes, scores=args.scores)
    elif os.path.isdir(args.tgt):
        if args.score_answer is not None:
            raise ValueError('--score_answer works on a single image')
        if args.ground or args.ground_answer is not None:
            raise ValueError('--ground / --ground_answer work on a single image')
        print('Multiple images recognition mode')
        os.makedirs('results', exist_ok=True)
        folder_rec(model, tokenizer, detect_model, generation_config, args.tgt, args.prompt, os.path.join('results', args.save_name),
                   args.use_p, args.hard_vq, args.drop_zero, args.repetition_penalty, args.verbose, batch_pages=args.batch_pages,
                   continuous=args.continuous, scores=args.scores, draft='align' if args.draft else None)
    else:
        raise ValueError('The target should be either a image path or a folder that contain images!')


def constraint_config(args):
    """The generation_config entries of --no_repeat_ngram_size / --min_new_tokens (none without them)."""
    return {k: getattr(args, k) for k in ('no_repeat_ngram_size', 'min_new_tokens') if getattr(args, k, 0)}


if __name__ == '__main__':
    main()

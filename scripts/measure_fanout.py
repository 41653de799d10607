#!/usr/bin/env python3
"""What n sampled answers per page cost, measured in one process: (a) one chat_ocr call with num_return_sequences=n, (b) n lone chat_ocr calls -- what
there was before cr_kv_fanout -- and (c) cr_kv_fanout alone, for n in {1, 2, 4, 8}; and the unchanged path: a sampled generate_pages at n = 1 of 13 pages
x 32 ids (run it with --unchanged-only on the parent commit too, twice, for the noise).

Setup as scripts/session_turns.py: seeded random weights at full InternVL2-8B dims, tests/golden/example0.jpg with its 96 boxes (a prompt of ~3 164
rows), benchlib.api's tokenizer stand-in, 32 new ids, the median of three passes after a warm-up, device events.  Writes profiles/fanout/fanout.json
(--out); --unchanged-only prints the 13-page figure as one JSON line and writes nothing."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW, REPEATS, NS = 32, 3, (1, 2, 4, 8)


def device_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def median_ms(fn):
    fn()                                                    # warm-up
    return round(statistics.median(device_ms(fn)[1] for _ in range(REPEATS)), 3)


def unchanged(m, page_embeds):
    """a sampled generate_pages at n = 1: 13 pages x 32 ids"""
    from callireader_amd.sampling import SamplingParams
    pages = [page_embeds[:512]] * 13
    return median_ms(lambda: m.generate_pages(pages, NEW, None, 1.5, sampling=SamplingParams(), seeds=list(range(13))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fanout', 'fanout.json'))
    ap.add_argument('--unchanged-only', action='store_true')
    args = ap.parse_args()
    import torch
    from session_turns import FIRST, setup
    from callireader_amd.sampling import SamplingParams
    m, tok, img, boxes = setup()
    m.max_tokens = 3712
    gc = dict(num_beams=1, max_new_tokens=NEW, do_sample=True, eos_token_id=None)
    page, px = m._open_page(img)
    ref, _ = m.calli_align(page, None, boxes=boxes)
    _, _, _, inputs, _ = m._ocr_prompt(tok, FIRST, None, len(px), ref, True, None, gc, False)
    embeds = m.engine.embed_splice(inputs['input_ids'].reshape(-1), m.extract_feature(px), ref, img_id=m.img_context_token_id, ref_id=m.aligned_token_id)
    rec = {'unchanged_generate_pages_13x32_ms': unchanged(m, embeds)}
    if args.unchanged_only:
        print(json.dumps(rec))
        return
    rec.update(prompt_rows=int(embeds.shape[0]), new_ids=NEW, repeats=REPEATS, by_n={})
    sp = SamplingParams()
    for n in NS:
        torch.manual_seed(n)
        one = median_ms(lambda: m.chat_ocr(tok, None, img, FIRST, dict(gc, **({'num_return_sequences': n} if n > 1 else {})), boxes=boxes))
        lone = median_ms(lambda: [m.chat_ocr(tok, None, img, FIRST, gc, boxes=boxes) for _ in range(n)])
        kv = m.kv(n + 1)

        def fan():
            kv.reset()
            kv.set_sampling(0, sp.temperature, sp.top_k, sp.top_p, 1)
            row = m.engine.prefill_batch(kv, [0], [embeds], penalty=1.5, want_logits=True)
            return device_ms(lambda: kv.fanout(0, list(range(1, n + 1)), list(range(2, n + 2)), row[0]))[1]
        fan()
        rec['by_n'][str(n)] = dict(one_call_ms=one, lone_calls_ms=lone, ratio=round(one / lone, 4),
                                   fanout_alone_ms=round(statistics.median(fan() for _ in range(REPEATS)), 4))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    main()

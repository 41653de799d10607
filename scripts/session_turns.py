#!/usr/bin/env python3
"""What a second turn about a page costs, measured: through chat_ocr(history=...) as before page sessions, through a session.PageSession, and as
PageSession.ask_many of 1, 4 and 8 questions.

Model: seeded random weights at full InternVL2-8B dims (InternVLChatModel.from_synthetic).  Page: tests/golden/example0.jpg with its 96 boxes (11 page
tiles + 96 character tiles = 107 ViT tiles, a first prompt of ~3 164 tokens); tokenizer: benchlib.api's sentencepiece stand-in with the reference's added
ids.  Turn 1 asks for the transcription (FIRST_NEW ids), turn 2 puts a question on that history and generates SECOND_NEW = 32 ids.  Random weights give
random text: the answer rarely re-tokenises to the generated ids, so the session's prefix usually ends at the first prompt -- what the record shows is
the cost structure, not what a trained model's turn would keep.

Every GPU step is a child process of its own under its own time limit; a step that fails or runs out of time ends the run (nothing more is started on
the GPU) and the record says which.  Writes profiles/session/turns.json (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIRST, SECOND = '这幅书法作品内容是什么？', '这幅作品表达了作者怎样的意图？'
QUESTIONS = [SECOND, '作者是谁？', '这是什么书体？', '作品的章法如何？', '请翻译成英文。', '写于什么年代？', '共有多少个字？', '内容出自哪里？']
FIRST_NEW, SECOND_NEW, REPEATS = 16, 32, 3
STEP_LIMIT_S = {'history': 420, 'session': 420, 'ask_many': 420}


def timed(fn):
    """(result, wall ms, device-event ms) of fn() between two synchronisations"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 2), round(a.elapsed_time(b), 2)


def med(rows, k):
    return round(statistics.median(r[k] for r in rows), 2)


def setup():
    import torch  # noqa: F401
    from PIL import Image
    from benchlib.api import make_tokenizer_dir
    from callireader_amd import preprocess
    from callireader_amd.config import ModelDims
    from callireader_amd.modeling_internvl_chat import InternVLChatModel
    from callireader_amd.tokenization_internlm2 import InternLM2Tokenizer
    work = tempfile.mkdtemp(prefix='cr_session_')
    make_tokenizer_dir(work)
    tok = InternLM2Tokenizer.from_pretrained(work)
    gold = os.path.join(ROOT, 'tests', 'golden')
    img = Image.open(os.path.join(gold, 'example0.jpg')).convert('RGB')
    boxes = preprocess.boxes_from_labelme(json.load(open(os.path.join(gold, 'example0_boxes.json'), encoding='utf-8')))
    m = InternVLChatModel.from_synthetic(ModelDims.full(), seed=0, max_tokens=3712, max_pages=1)
    return m, tok, img, boxes


class Probe:
    """Counts, while installed, the tiles that go through the ViT (extract_feature) and the rows of every prefill."""

    def __init__(self, model):
        self.eng, self.tiles, self.rows = model.engine, 0, []

    def __enter__(self):
        eng = self.eng
        self.saved = (eng.extract_feature, eng.prefill, eng.prefill_batch)

        def extract_feature(px):
            self.tiles += int(px.shape[0])
            return self.saved[0](px)

        def prefill(kv, seq, embeds, **k):
            self.rows.append(int(embeds.reshape(-1, embeds.shape[-1]).shape[0]))
            return self.saved[1](kv, seq, embeds, **k)

        def prefill_batch(kv, seqs, embeds_list, **k):
            self.rows.append(sum(int(e.reshape(-1, e.shape[-1]).shape[0]) for e in embeds_list))
            return self.saved[2](kv, seqs, embeds_list, **k)
        eng.extract_feature, eng.prefill, eng.prefill_batch = extract_feature, prefill, prefill_batch
        return self

    def __exit__(self, *exc):
        self.eng.extract_feature, self.eng.prefill, self.eng.prefill_batch = self.saved


def gen(n):
    return dict(num_beams=1, max_new_tokens=n, do_sample=False)


def step_history():
    """turn 2 as before sessions: chat_ocr on the same image with history= (visual stage again, the whole prompt prefilled again)"""
    m, tok, img, boxes = setup()
    rows = []
    for i in range(REPEATS + 1):                                   # the first pass warms up
        (_, hist), w1, d1 = timed(lambda: m.chat_ocr(tok, None, img, FIRST, gen(FIRST_NEW), boxes=boxes, return_history=True, repetition_penalty=1.0))
        with Probe(m) as pr:
            (r2, h2), w2, d2 = timed(lambda: m.chat_ocr(tok, None, img, SECOND, gen(SECOND_NEW), boxes=boxes, history=hist, return_history=True,
                                                       repetition_penalty=1.0))
        if i:
            rows.append(dict(turn1_wall_ms=w1, turn1_device_ms=d1, turn2_wall_ms=w2, turn2_device_ms=d2, rows_prefilled_turn2=pr.rows[0],
                             tiles_through_the_vit_turn2=pr.tiles, ids_generated_turn2=len(m.kv().generated(0)[:SECOND_NEW])))
    return dict(runs=rows, turn1_wall_ms=med(rows, 'turn1_wall_ms'), turn1_device_ms=med(rows, 'turn1_device_ms'), turn2_wall_ms=med(rows, 'turn2_wall_ms'),
                turn2_device_ms=med(rows, 'turn2_device_ms'), rows_prefilled_turn2=rows[0]['rows_prefilled_turn2'],
                tiles_through_the_vit_turn2=rows[0]['tiles_through_the_vit_turn2'], ids_generated_turn2=rows[0]['ids_generated_turn2'])


def step_session():
    """the same two turns on a PageSession, and the fork kernel alone"""
    import torch
    m, tok, img, boxes = setup()
    rows = []
    for i in range(REPEATS + 1):
        s, wo, do = timed(lambda: m.open_page(tok, None, img, boxes=boxes, max_branches=8))
        (_, hist), w1, d1 = timed(lambda: s.chat_ocr(FIRST, gen(FIRST_NEW), return_history=True, repetition_penalty=1.0))
        cached = len(s.cached_ids)
        with Probe(m) as pr:
            (r2, h2), w2, d2 = timed(lambda: s.chat_ocr(SECOND, gen(SECOND_NEW), history=hist, return_history=True, repetition_penalty=1.0))
        if i:
            rows.append(dict(open_wall_ms=wo, turn1_wall_ms=w1, turn1_device_ms=d1, turn2_wall_ms=w2, turn2_device_ms=d2, rows_prefilled_turn1=s.rows_prefilled[0],
                             rows_prefilled_turn2=pr.rows[0], cached_positions_before_turn2=cached, tiles_through_the_vit_turn2=pr.tiles,
                             prefix_kept_turn2=s.kv.length(0) - (len(s.kv.generated(0)) - 1) - pr.rows[0],      # S2 - rows: the trunk holds S2 + ids - 1
                             ids_generated_turn2=len(s.kv.generated(0)[:SECOND_NEW])))
        if i < REPEATS:
            s.close()
    n = s.kv.length(0)
    fork = []
    for n_dst in (1, 4, 8):
        s.kv.fork(0, list(range(1, 1 + n_dst)), n)                  # warm
        _, w, d = timed(lambda: s.kv.fork(0, list(range(1, 1 + n_dst)), n))
        read = m.dims.llm_layers * 16 * n * 256
        fork.append(dict(branches=n_dst, tokens=n, bytes_read=read, bytes_written=read * n_dst, device_ms=d, wall_ms=w,
                         gb_per_s=round(read * (1 + n_dst) / (d * 1e-3) / 1e9, 1) if d > 0 else None))
    s.close()
    return dict(runs=rows, open_page_wall_ms=med(rows, 'open_wall_ms'), turn1_wall_ms=med(rows, 'turn1_wall_ms'), turn2_wall_ms=med(rows, 'turn2_wall_ms'),
                turn2_device_ms=med(rows, 'turn2_device_ms'), rows_prefilled_turn1=rows[0]['rows_prefilled_turn1'], rows_prefilled_turn2=rows[0]['rows_prefilled_turn2'],
                prefix_kept_turn2=rows[0]['prefix_kept_turn2'], tiles_through_the_vit_turn2=rows[0]['tiles_through_the_vit_turn2'],
                ids_generated_turn2=rows[0]['ids_generated_turn2'], turn1_device_ms=med(rows, 'turn1_device_ms'), fork=fork)


def step_ask_many():
    """ask_many of 1, 4 and 8 second-turn questions on the first turn's history"""
    m, tok, img, boxes = setup()
    s = m.open_page(tok, None, img, boxes=boxes, max_branches=8)
    _, hist = s.chat_ocr(FIRST, gen(FIRST_NEW), return_history=True, repetition_penalty=1.0)
    out = []
    for k in (1, 4, 8):
        rows = []
        for i in range(REPEATS + 1):
            before = len(s.rows_prefilled)
            res, w, d = timed(lambda: s.ask_many(QUESTIONS[:k], gen(SECOND_NEW), history=hist, repetition_penalty=1.0))
            assert len(res) == k and len(s.rows_prefilled) == before + 1
            if i:
                rows.append(dict(wall_ms=w, device_ms=d, rows_prefilled=s.rows_prefilled[-1]))
        out.append(dict(questions=k, wall_ms=med(rows, 'wall_ms'), device_ms=med(rows, 'device_ms'), wall_ms_per_question=round(med(rows, 'wall_ms') / k, 2),
                        rows_prefilled=rows[0]['rows_prefilled'], runs=rows))
    s.close()
    return dict(batches=out)


STEPS = {'history': step_history, 'session': step_session, 'ask_many': step_ask_many}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'session', 'turns.json'))
    ap.add_argument('--step', choices=sorted(STEPS), help='(internal) run one step in this process and print its JSON')
    a = ap.parse_args()
    if a.step:
        print('RESULT ' + json.dumps(STEPS[a.step]()))
        return 0
    rec = {'what': __doc__.split('\n\n')[1].replace('\n', ' '), 'weights': 'seeded random (no checkpoint): times and row counts, not text',
           'first_new_tokens': FIRST_NEW, 'second_new_tokens': SECOND_NEW, 'repeats': REPEATS, 'times': 'median of the repeats after one warm-up pass'}
    status = 0
    for name in ('history', 'session', 'ask_many'):                 # a fresh process per step: none inherits a GPU another one left in a bad state
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=STEP_LIMIT_S[name],
                               cwd=ROOT)
        except subprocess.TimeoutExpired:
            rec[name] = {'error': f'time limit of {STEP_LIMIT_S[name]} s'}
            status = 1
            break
        line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            rec[name] = {'error': f'exit status {r.returncode}', 'stderr_tail': r.stderr.decode()[-800:]}
            status = 1
            break                                                    # nothing more is started on the GPU after a failed step
        rec[name] = json.loads(line[-1][7:])
        print(name, json.dumps({k: v for k, v in rec[name].items() if k not in ('runs', 'batches', 'fork')}), flush=True)
    if status == 0:
        h, s = rec['history'], rec['session']
        rec['turn2_session_over_history_wall'] = round(s['turn2_wall_ms'] / h['turn2_wall_ms'], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w', encoding='utf-8') as f:
        json.dump(rec, f, ensure_ascii=False, indent=1)
    print('wrote', a.out)
    return status


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""tests/golden/internlm2_tokenizer/ from the reference's tokenizer files (its InternVL/ directory, given on the command line).

The whole tokenizer.model is too large to keep in the repository.  pieces.json holds what tests/test_tokenizer.py needs to rebuild
a model that encodes and decodes everything those tests give it exactly as the whole one does (test_tokenizer.rebuild_real_model):
  * the model without its pieces (normaliser and trainer specs), base64, and the number of pieces;
  * the pieces kept, as [id, piece, score, type]: every normal piece that is a substring of a text the tests encode (sentencepiece BPE
    starts from characters and only merges into pieces that are substrings of its input), the piece holding a NUL byte, every special
    and byte piece, and every id that tests/golden/tokenizer_vectors.json holds.
The three JSON files of the checkpoint's tokenizer are copied as they are.  Only data is written.
Usage: python scripts/make_golden_tokenizer_fixture.py <reference>/InternVL
"""
import base64
import importlib.util
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'internlm2_tokenizer')
GOLD = os.path.join(ROOT, 'tests', 'golden', 'tokenizer_vectors.json')


def main(ref):
    from sentencepiece import sentencepiece_model_pb2 as pb
    spec = importlib.util.spec_from_file_location('test_tokenizer', os.path.join(ROOT, 'tests', 'test_tokenizer.py'))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)

    gold = json.load(open(GOLD, encoding='utf-8'))
    texts = tt.fixture_texts()
    ids = set()

    def collect(x):
        if isinstance(x, int):
            ids.add(x)
        elif isinstance(x, list):
            for y in x:
                collect(y)
        elif isinstance(x, dict):
            for y in x.values():
                collect(y)
    collect(gold)

    m = pb.ModelProto()
    m.ParseFromString(open(os.path.join(ref, 'tokenizer.model'), 'rb').read())
    assert m.normalizer_spec.name == 'identity' and not m.normalizer_spec.add_dummy_prefix and m.trainer_spec.model_type == pb.TrainerSpec.BPE
    joined = '￿'.join(t.replace(' ', '▁') if m.normalizer_spec.escape_whitespaces else t for t in texts)
    kept = [[i, p.piece, p.score, p.type] for i, p in enumerate(m.pieces)
            if p.type != pb.ModelProto.SentencePiece.NORMAL or p.piece in joined or '\x00' in p.piece or i in ids]
    assert not any(tt.placeholder_piece(i) in joined for i in range(len(m.pieces)))
    n = len(m.pieces)
    del m.pieces[:]
    os.makedirs(OUT, exist_ok=True)
    out = {'_how': 'scripts/make_golden_tokenizer_fixture.py from the reference\'s InternVL/tokenizer.model', 'n_pieces': n, 'texts_sha256': tt.texts_sha256(texts),
           'model_without_pieces': base64.b64encode(m.SerializeToString()).decode('ascii'), 'pieces': kept}
    with open(os.path.join(OUT, 'pieces.json'), 'w', encoding='utf-8') as f:
        json.dump(out, f, ensure_ascii=False, separators=(',', ':'))
    for name in ('tokenizer_config.json', 'added_tokens.json', 'special_tokens_map.json'):
        shutil.copy(os.path.join(ref, name), OUT)
    print(f'{len(kept)} of {n} pieces kept, {os.path.getsize(os.path.join(OUT, "pieces.json"))} bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])

"""Drafts through the public entry points on a real MI355X: the reduced whole model, checkpoint and tokenizer of test_gpu_boundary.py.  A draft never
changes an answer: every call here is made once without a draft and once with one, and the two results are compared with ==."""
import pytest
import torch

from test_gpu_boundary import YoloLike, ckpt, setup      # noqa: F401  (the module-scoped fixtures of that file)

pytestmark = pytest.mark.gpu

Q = '这幅书法作品内容是什么？'
GEN = dict(num_beams=1, max_new_tokens=12, do_sample=False)


def test_chat_ocr_with_the_align_draft_returns_chat_ocrs_response(setup):
    m, tok, img = setup['model'], setup['tok'], setup['img']
    want = m.chat_ocr(tok, YoloLike(setup['raw']), img, Q, GEN, repetition_penalty=1.2)
    got = m.chat_ocr(tok, YoloLike(setup['raw']), img, Q, GEN, repetition_penalty=1.2, draft='align')
    assert got == want
    assert m.draft_stats['steps'] >= 1
    with pytest.raises(NotImplementedError, match='not implemented with a draft'):
        m.chat_ocr(tok, YoloLike(setup['raw']), img, Q, dict(GEN, do_sample=True), repetition_penalty=1.2, draft='align')


def test_generate_pages_with_drafts_returns_generate_pages_ids(setup):
    m = setup['model']
    g = torch.Generator().manual_seed(5)
    V = setup['dims'].vocab
    embeds = [m.engine.embed_splice(torch.randint(3, V - 8, (S,), generator=g)) for S in (40, 300)]
    want = m.generate_pages(embeds, max_new_tokens=20, eos_token_id=None, repetition_penalty=1.2)
    assert [len(w) for w in want] == [20, 20]
    wrong = [(t + 1) % V for t in want[1]]
    for drafts, most in (([want[0], want[1]], 3), ([want[0], None], 19), ([wrong, want[1]], 19), ([[], want[1][3:]], 19)):
        assert m.generate_pages(embeds, max_new_tokens=20, eos_token_id=None, repetition_penalty=1.2, drafts=drafts) == want, drafts
        assert m.draft_stats['steps'] <= most, (drafts, m.draft_stats)


def test_a_sessions_second_turn_drafted_by_its_first_answer(setup):
    m, tok, img = setup['model'], setup['tok'], setup['img']
    answers = []
    for draft in (None, 'previous', 'align'):
        with m.open_page(tok, YoloLike(setup['raw']), img) as s:
            first, hist = s.chat_ocr(Q, GEN, repetition_penalty=1.2, return_history=True)
            answers.append((first, s.chat_ocr('再读一遍。', GEN, history=hist, repetition_penalty=1.2, **(dict(draft=draft) if draft else {}))))
    assert answers[1] == answers[0] and answers[2] == answers[0]

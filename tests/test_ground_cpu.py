"""The host side of grounding (callireader_amd/grounding.py and the entry points' refusals): no GPU."""
import numpy as np
import pytest
import torch

from callireader_amd import grounding as G

from engine_stubs import REF, make_model, make_session, RoundTripTokenizer


def test_spans_of_finds_the_boxes():
    assert G.spans_of([1, 2, 3], REF) == []                                                      # no box
    assert G.spans_of([1, REF, REF, REF, 2], REF) == [(1, 4)]                                    # one
    ids = [7, 7] + [REF] * 9 + [5, 6]
    assert G.spans_of(ids, REF) == [(2, 5), (5, 8), (8, 11)]                                     # several, in reading order
    assert G.spans_of(torch.tensor([ids]), REF) == [(2, 5), (5, 8), (8, 11)]                     # a tokenizer's [1, S] tensor
    assert G.spans_of([REF] * 4, REF, per_box=2) == [(0, 2), (2, 4)]
    for bad in ([REF] * 4, [REF, REF, 9, REF]):                                                  # not a multiple of 3; a box that is not one run
        with pytest.raises(ValueError):
            G.spans_of(bad, REF)


def test_spans_of_with_drop_zero_counts():
    ids = [7] + [REF] * 5 + [8]
    assert G.spans_of(ids, REF, per_box=[3, 0, 2]) == [(1, 4), (4, 4), (4, 6)]                   # a box that kept nothing: an empty span in its place
    assert G.spans_of(ids, REF, per_box=[0, 3, 2, 0]) == [(1, 1), (1, 4), (4, 6), (6, 6)]
    assert G.spans_of([1, 2], REF, per_box=[0, 0]) == [(0, 0), (0, 0)]
    with pytest.raises(ValueError):
        G.spans_of(ids, REF, per_box=[3, 3])
    assert G.kept_per_box(torch.tensor([[4, 0, 9], [0, 0, 0], [1, 2, 3]])) == [2, 0, 3] and G.kept_per_box(np.array([5, 0, 0])) == [1]


def test_span_validation():
    assert G.check_spans([(0, 2), (2, 2), (2, 5)], limit=5) == [(0, 2), (2, 2), (2, 5)]
    for bad in ([(3, 5), (0, 2)], [(0, 3), (2, 5)], [(4, 2)], [(-1, 2)]):                        # unsorted, overlapping, reversed, below 0
        with pytest.raises(ValueError):
            G.check_spans(bad)
    with pytest.raises(ValueError):
        G.check_spans([(0, 2), (4, 7)], limit=6)                                                 # out of range
    with pytest.raises(ValueError):
        G.check_spans([(i, i + 1) for i in range(G.MAX_SPANS + 1)])
    assert G.check_layers(None, 32) == (0, 32) and G.check_layers((8, 16), 32) == (8, 16)
    for bad in ((-1, 2), (0, 33), (4, 4), (5, 4)):
        with pytest.raises(ValueError):
            G.check_layers(bad, 32)


def test_grounding_from_a_mass_matrix():
    mass = np.array([[0.10, 0.30, 0.30, 0.0],      # a tie: the lower box
                     [0.00, 0.00, 0.00, 0.0],
                     [0.05, 0.02, 0.60, 0.1]], dtype=np.float32)
    spans = [(2, 5), (5, 8), (8, 11)]
    boxes = [(0, 0, 10, 10), (10, 0, 20, 10), (20, 0, 30, 10.7)]
    g = G.Grounding.build([11, 12, 99], mass, spans, pieces=['a', 'b', '<eos>'], boxes=boxes, layers=(0, 2), special_ids=[99])
    assert [t.box for t in g.tokens] == [1, 0, 2] and g.tokens[0].box_mass == pytest.approx(0.3) and g.tokens[2].box_mass == pytest.approx(0.6)
    assert g.tokens[0].elsewhere == pytest.approx(0.3) and g.tokens[1].elsewhere == 1.0 and g.tokens[2].elsewhere == pytest.approx(0.33)
    assert g.mass.shape == (3, 3) and g.kept == [0, 1] and g.boxes[2] == [20, 0, 30, 10]        # the padding column is dropped
    assert g.pairs() == [('a', [10, 0, 20, 10], pytest.approx(0.3)), ('b', [0, 0, 10, 10], 0.0)]
    assert g.to_json()[0] == {'piece': 'a', 'box': [10, 0, 20, 10], 'mass': pytest.approx(0.3)}
    # a page without a span: box -1, nothing claimed
    e = G.Grounding.build([11], np.zeros((1, 1), np.float32), [], pieces=['a'], boxes=[])
    assert e.tokens[0].box == -1 and e.tokens[0].box_mass == 0.0 and e.tokens[0].elsewhere == 1.0 and e.pairs() == [('a', None, 0.0)]
    with pytest.raises(ValueError):
        G.Grounding.build([11], mass[:1], spans, boxes=boxes[:2])


def test_entry_points_refuse_what_steers_a_generation():
    """model.ground_ocr / ground_pages and PageSession.ground on the stubs: every refusal comes before any engine call"""
    m = make_model()
    tok = RoundTripTokenizer()
    for kw in (dict(generation_config=dict(do_sample=True)), dict(generation_config=dict(num_beams=2)), dict(generation_config=dict(no_repeat_ngram_size=2)),
               dict(draft='align'), dict(draft=[1, 2]), dict(top_logprobs=9), dict(repetition_penalty=0), dict(use_p=False)):
        for answer in (None, 'abc'):
            with pytest.raises(ValueError):
                m.ground_ocr(tok, None, None, 'q', answer, **kw)
    emb = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        m.ground_pages([emb], [[1]], [[(0, 1)], []])
    with pytest.raises(ValueError):
        m.ground_pages([emb], [[1]], [[(0, 1)]], repetition_penalty=-1)
    m8 = make_model(kv_cache_dtype='e4m3')
    with pytest.raises(NotImplementedError):
        m8.ground_ocr(tok, None, None, 'q')
    with pytest.raises(NotImplementedError):
        m8.ground_pages([emb], [[1]], [[(0, 1)]])
    assert m.engine.log == [] and m8.engine.log == []

    sess, eng = make_session()
    for kw in (dict(generation_config=dict(do_sample=True)), dict(generation_config=dict(num_beams=2)), dict(draft='align'), dict(top_logprobs=9)):
        with pytest.raises(ValueError):
            sess.ground('q', **kw)
    assert eng.log == []

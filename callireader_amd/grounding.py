"""Grounding a transcription (cr_llm_ground_batch in include/callireader_hip.h): the host side, which needs no GPU.

CalliAlign puts every detected character box into the prompt as a run of pseudo-token rows -- three per box, in reading order, at the positions of the
aligned-token id -- so box b is a contiguous range of cache positions, a SPAN [start, end).  A grounding call is a scoring call (scoring.py) that also
reports, per scored id, the attention probability its row put on every span, averaged over heads and layers: a soft alignment of the id to the boxes.
Here the spans are found and validated, and the device's mass matrix becomes a Grounding: per id its row, its best box and what the boxes did not get."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

MAX_SPANS = 1024          # GROUND_MAX_SPANS of csrc/ground.hpp


def kept_per_box(indices, per_box=3):
    """The pseudo-token rows `drop_zero` keeps of every box: the entries of calli_align's indices [boxes, per_box] that are not 0."""
    a = np.asarray(indices.cpu() if hasattr(indices, 'cpu') else indices).reshape(-1, per_box)
    return [int(n) for n in (a != 0).sum(axis=1)]


def spans_of(prompt_ids, aligned_token_id, per_box=3):
    """The boxes' spans [(start, end), ...] in a prompt's ids: the positions of aligned_token_id, grouped per box in reading order.  per_box: an int (every box
    has that many pseudo-tokens), or the list of kept counts per box (drop_zero: kept_per_box), where a box with 0 gets an empty span at the place it would
    have had.  ValueError when the positions do not add up to the boxes, or a box's positions are not one run."""
    ids = prompt_ids.reshape(-1).tolist() if hasattr(prompt_ids, 'reshape') else [int(t) for t in prompt_ids]
    pos = [i for i, t in enumerate(ids) if t == aligned_token_id]
    if isinstance(per_box, (int, np.integer)) and not isinstance(per_box, bool):
        if per_box < 1:
            raise ValueError(f'per_box has to be >= 1, got {per_box}')
        if len(pos) % per_box:
            raise ValueError(f'{len(pos)} pseudo-token positions are no multiple of per_box={per_box}')
        counts = [int(per_box)] * (len(pos) // per_box)
    else:
        counts = [int(c) for c in per_box]
        if any(c < 0 for c in counts) or sum(counts) != len(pos):
            raise ValueError(f'per_box counts {counts} do not add up to the {len(pos)} pseudo-token positions of the prompt')
    spans, k, at = [], 0, (pos[0] if pos else 0)
    for c in counts:
        if c == 0:
            spans.append((at, at))
            continue
        run = pos[k:k + c]
        if run[-1] - run[0] != c - 1:
            raise ValueError(f'the pseudo-tokens of box {len(spans)} sit at {run}: not one run of positions')
        spans.append((run[0], run[-1] + 1))
        at, k = run[-1] + 1, k + c
    return spans


def check_spans(spans, limit=None):
    """[(start, end), ...] as ints, validated as the library validates them: sorted by start, not overlapping, not reversed, inside [0, limit), at most
    MAX_SPANS.  ValueError otherwise."""
    out, prev = [], 0
    if len(spans) > MAX_SPANS:
        raise ValueError(f'{len(spans)} spans (at most {MAX_SPANS} per sequence)')
    for b, sp in enumerate(spans):
        s, e = int(sp[0]), int(sp[1])
        if e < s:
            raise ValueError(f'span {b} = ({s}, {e}) is reversed')
        if s < prev:
            raise ValueError(f'span {b} = ({s}, {e}) starts before {prev}: spans have to be sorted by start and must not overlap')
        if limit is not None and e > limit:
            raise ValueError(f'span {b} = ({s}, {e}) leaves [0, {limit})')
        out.append((s, e))
        prev = e
    return out


def check_layers(layers, n_layers):
    """layers=None: all; or (layer0, layer1), a non-empty range inside [0, n_layers)."""
    if layers is None:
        return 0, int(n_layers)
    l0, l1 = (int(v) for v in layers)
    if l0 < 0 or l1 > n_layers or l0 >= l1:
        raise ValueError(f'layers={layers!r}: want a non-empty range inside [0, {n_layers})')
    return l0, l1


@dataclass
class GroundedToken:
    id: int
    piece: str
    mass: np.ndarray           # [spans] float32: the id's row
    box: int                   # argmax of the row (a tie goes to the lower box), -1 when there is no span
    box_mass: float            # the row's entry there, 0.0 without a span
    elsewhere: float           # 1 - sum(row): what the boxes did not get (the page's tiles, the question, the answer so far)


@dataclass
class Grounding:
    """Per scored id, in order: where its row looked.  boxes: the page's character boxes [x1, y1, x2, y2] in reading order, one per span (None when the
    caller brought spans without boxes)."""
    tokens: List[GroundedToken]
    spans: List[Tuple[int, int]]
    boxes: Optional[list] = None
    layers: Tuple[int, int] = (0, 0)
    scores: object = None      # scores.ResponseScores of the same pass, when asked for
    kept: List[int] = field(default_factory=list)      # indices of the tokens that are no special token

    @property
    def mass(self):
        return np.stack([t.mass for t in self.tokens]) if self.tokens else np.zeros((0, len(self.spans)), np.float32)

    @classmethod
    def build(cls, ids, mass, spans, pieces=None, boxes=None, layers=(0, 0), special_ids=(), scores=None):
        """ids [T], mass [T, >= len(spans)] (numpy or a CPU tensor; the columns past the spans are dropped)."""
        m = np.asarray(mass, dtype=np.float32).reshape(len(ids), -1)[:, :len(spans)]
        if boxes is not None and len(boxes) != len(spans):
            raise ValueError(f'{len(boxes)} boxes for {len(spans)} spans')
        pieces = [str(t) for t in ids] if pieces is None else list(pieces)
        toks = []
        for j, t in enumerate(ids):
            row = m[j].copy()
            b = int(np.argmax(row)) if len(spans) else -1          # np.argmax: the first maximum
            toks.append(GroundedToken(int(t), pieces[j], row, b, float(row[b]) if b >= 0 else 0.0, float(1.0 - row.astype(np.float64).sum())))
        sp = set(int(s) for s in special_ids)
        return cls(toks, [(int(s), int(e)) for s, e in spans], None if boxes is None else [[int(v) for v in bx[:4]] for bx in boxes], tuple(layers), scores,
                   [j for j, t in enumerate(ids) if int(t) not in sp])

    def pairs(self):
        """[(piece, box [x1, y1, x2, y2] or None, box_mass)] of the kept tokens: "character -> box"."""
        out = []
        for j in self.kept:
            t = self.tokens[j]
            out.append((t.piece, self.boxes[t.box] if (self.boxes is not None and t.box >= 0) else None, t.box_mass))
        return out

    def to_json(self):
        return [{'piece': p, 'box': b, 'mass': m} for p, b, m in self.pairs()]


def pieces_of(tokenizer, ids):
    """The decoded piece of every id (the tokenizer's token strings where it has them, else the id as text)."""
    if hasattr(tokenizer, 'convert_ids_to_tokens'):
        return [str(p) for p in tokenizer.convert_ids_to_tokens([int(t) for t in ids])]
    return [str(int(t)) for t in ids]


def special_ids_of(tokenizer):
    return list(getattr(tokenizer, 'all_special_ids', None) or [])

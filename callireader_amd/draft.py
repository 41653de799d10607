"""Draft-verified greedy decoding, host side: where a draft comes from and which window of it the next step checks.

A draft is a list of vocabulary ids that guesses what a sequence is about to generate.  cr_llm_decode_draft (Engine.decode_draft) checks up to WINDOW of
them in one weight pass and keeps a drafted id only where it equals the greedy pick, so the ids returned never depend on the draft: a wrong one costs
rows in a step, never an id, and every step appends at least the one id a plain step appends.

Two sources cost nothing: the rows of the LLM's own token-embedding table that CalliAlign's VQ step snaps every character box's three pseudo-tokens to
(`indices` of calli_align, in reading order: `from_indices`), and an earlier answer about the same page (session.PageSession).

Plain Python: nothing here touches a tensor between two decode steps."""

WINDOW = 7            # drafted ids per sequence and step (csrc/draft.hpp DRAFT_MAX)
MAX_ROWS = 64         # rows per step, sequences + drafted ids (csrc/draft.hpp DRAFT_MAX_ROWS)
LOOKAHEAD = 32        # how far ahead of the cursor a lost draft is searched for the id just generated

DRAFT_NOT_WITH = ('draft-verified decoding is greedy, one row per page and without per-token records: {what} is not implemented with a draft '
                  '(leave draft / draft_ids / drafts off)')


def refuse(what):
    """The NotImplementedError of an option that does not combine with a draft."""
    raise NotImplementedError(DRAFT_NOT_WITH.format(what=what))


def from_indices(indices):
    """The draft ids of calli_align's `indices` -- (T, 3) rows of the token-embedding table per character box, or the squeezed (3,) of a single box; a
    tensor, an array or nested lists -- flattened row-major, 0 entries dropped (as drop_zero drops their pseudo-tokens)."""
    if indices is None:
        return []
    rows = indices.tolist() if hasattr(indices, 'tolist') else list(indices)
    flat = []
    for r in rows:
        flat.extend(r if isinstance(r, (list, tuple)) else [r])
    return [int(t) for t in flat if int(t) != 0]


class DraftCursor:
    """A position in one sequence's draft.  `feed(ids)` takes the ids the sequence has just appended, in order: while the cursor is in step each of them
    either equals the drafted id under it (the cursor moves on) or does not -- then, and for every later id until it succeeds, the cursor looks for that id
    within `lookahead` ids ahead of itself (an insertion in the output leaves it where it is, a deletion makes it jump) and is in step again behind the
    match.  `window(room)` is the next guess: up to `size` ids from the cursor, at most `room` of them, none while the cursor is out of step."""

    def __init__(self, ids, size=WINDOW, lookahead=LOOKAHEAD):
        self.ids = [int(t) for t in ids]
        self.size, self.lookahead = min(int(size), WINDOW), int(lookahead)
        self.pos, self.in_step = 0, True

    def feed(self, new_ids):
        ids, n = self.ids, len(self.ids)
        for t in new_ids:
            if self.in_step and self.pos < n and ids[self.pos] == t:
                self.pos += 1
                continue
            self.in_step = False
            for j in range(self.pos, min(n, self.pos + self.lookahead)):
                if ids[j] == t:
                    self.pos, self.in_step = j + 1, True
                    break

    def window(self, room):
        if not self.in_step:
            return []
        return self.ids[self.pos:self.pos + max(0, min(self.size, room))]


def fit_rows(windows, max_rows=MAX_ROWS):
    """The windows of one step shortened, the longest first, until sequences + drafted ids are at most max_rows (len(windows) <= max_rows)."""
    windows = [list(w) for w in windows]
    over = sum(len(w) + 1 for w in windows) - max_rows
    while over > 0:
        longest = max(len(w) for w in windows)
        if longest == 0:
            break
        for w in windows:
            if over > 0 and len(w) == longest and longest > 0:
                w.pop()
                over -= 1
    return windows

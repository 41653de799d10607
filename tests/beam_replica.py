"""Host replica of the engine's beam search, in plain torch: the seven steps of DESIGN 13 (transformers' deterministic GenerationMixin._beam_search with
do_sample=False, one returned sequence, driven with inputs_embeds only, so the processors see the generated ids).  A test helper: it is not imported from
the package, and the package does not import it.  tests/test_beam_cpu.py holds it against the installed transformers; the GPU tests hold the device
against it."""
import torch

NEG = -1.0e9


class Beam:
    """One beam group.  step(logits) consumes the fp32 next-token logits of the B running beams ([B, V]; [1, V] at step 0, where every beam is the prompt)
    and advances: run (fp32 [B], descending), seqs (the beams' generated ids), fin (finished slots, best first: dicts score / ids), heur, done, g."""

    def __init__(self, num_beams, max_new_tokens, eos_token_id=None, length_penalty=1.0, early_stopping=False, repetition_penalty=1.0):
        assert early_stopping in (False, True, 'never')
        self.B, self.max_new, self.eos = int(num_beams), int(max_new_tokens), eos_token_id
        self.lp, self.early, self.pen = float(length_penalty), early_stopping, float(repetition_penalty)
        self.run = torch.full((self.B,), NEG, dtype=torch.float32)
        self.run[0] = 0.0
        self.seqs = [[] for _ in range(self.B)]
        self.fin = []
        self.heur, self.done, self.g = True, False, 0
        self.src = list(range(self.B))        # source beam of every running beam in the last step
        self.min_gap = float('inf')           # smallest float64 gap between neighbours of any step's top K + 1 candidates (0: an exact tie)
        self.stopped_by = None                # 'heuristic' | 'early' | 'length'
        self.alive_at_stop = False            # a running beam was still alive (score > -1e8) when the group stopped
        self.cands = []                       # per step: the K candidates' (source beam, id, acc), best first

    def log_probs(self, logits):
        """Step 1: log-softmax in fp32, then the repetition penalty over each beam's own ids ON the log-probabilities."""
        lp = torch.log_softmax(logits.to(torch.float32), dim=-1)
        if lp.shape[0] == 1:
            lp = lp.expand(self.B, -1)
        lp = lp.clone()
        if self.pen != 1.0:
            for b, ids in enumerate(self.seqs):
                if ids:
                    i = torch.tensor(ids, dtype=torch.long)
                    s = lp[b, i]
                    lp[b, i] = torch.where(s < 0, s * self.pen, s / self.pen)
        return lp

    def step(self, logits):
        assert not self.done
        B, K, g = self.B, 2 * self.B, self.g
        lp = self.log_probs(logits)
        V = lp.shape[1]
        acc = (lp + self.run[:, None]).reshape(-1)                                   # step 2
        sv, si = torch.sort(acc, descending=True, stable=True)                       # stable: the lower flattened index first on an exact tie
        d = sv[:K + 1].double()
        gaps = (d[:-1] - d[1:])[torch.isfinite(d[:-1]) & torch.isfinite(d[1:])]
        if gaps.numel():
            self.min_gap = min(self.min_gap, float(gaps.min()))
        topv, topb, topi = sv[:K], (si[:K] // V).tolist(), (si[:K] % V).tolist()
        self.cands.append(list(zip(topb, topi, topv.tolist())))
        lim = g + 1 >= self.max_new
        fin = [lim or (self.eos is not None and i == self.eos) for i in topi]        # step 3
        eligible = not (len(self.fin) == B and self.early is True) and self.heur
        denom = (g + 1) ** self.lp
        nxt = []
        for k in range(K):
            if not fin[k]:
                if len(nxt) < B:
                    nxt.append((topv[k], topb[k], topi[k]))                          # step 4
            elif k < B and eligible:                                                 # step 5
                score = topv[k] / denom
                if not bool(score > NEG):
                    continue
                hyp = {'score': score, 'ids': self.seqs[topb[k]] + [topi[k]]}
                if len(self.fin) < B:
                    self.fin.append(hyp)
                elif bool(score > self.fin[-1]['score']):
                    self.fin[-1] = hyp
                else:
                    continue
                self.fin.sort(key=lambda h: -float(h['score']))                      # (stable: an equal score stays behind the older one)
        for k in range(K):                                                           # the length limit: finishing candidates fill up, as acc - 1e9 ranks them
            if len(nxt) < B and fin[k]:
                nxt.append((topv[k] + torch.tensor(NEG), topb[k], topi[k]))
        self.run = torch.stack([v for v, _, _ in nxt]).to(torch.float32)
        self.src = [b for _, b, _ in nxt]
        self.seqs = [self.seqs[b] + [i] for _, b, i in nxt]
        self.ids = [i for _, _, i in nxt]
        L = self.max_new if (self.early == 'never' and self.lp > 0.0) else g + 1     # step 6
        best = self.run[0] / (L ** self.lp)
        worst = self.fin[-1]['score'] if len(self.fin) == B else torch.tensor(NEG)
        self.heur = self.heur and bool(best > worst)
        self.g = g + 1
        if not self.heur:
            self.done, self.stopped_by = True, 'length' if all(fin) else 'heuristic'
        elif len(self.fin) == B and self.early is True:
            self.done, self.stopped_by = True, 'early'
        elif all(fin):
            self.done, self.stopped_by = True, 'length'
        if self.done:
            self.alive_at_stop = bool(self.run[0] > -1.0e8)
        return self.done

    def result(self):
        """Step 7: (ids of the best finished hypothesis, EOS included; its score)."""
        if not self.fin:
            return [], NEG
        return list(self.fin[0]['ids']), float(self.fin[0]['score'])


def beam_search(logits_fn, num_beams, max_new_tokens, **kw):
    """Run a group to its end.  logits_fn(seqs) -> fp32 [len(seqs), V]: the next-token logits after the prompt followed by each id list.  Returns the Beam."""
    bm = Beam(num_beams, max_new_tokens, **kw)
    while not bm.done:
        bm.step(logits_fn([bm.seqs[0]]) if bm.g == 0 else logits_fn(bm.seqs))
    return bm

"""Test-only restatement of dlsg_seq_logprob (the log-probability of GIVEN captions) in float64 on top of
tests/emul_ensemble.py: `seq_logprob_f64` gives the values and, per position, how close another class comes to the target's
combined value, so that a comparison of the float32 kernel's ranks can leave near-ties out; `SeqScoreEmul.seq_logprob` is the
binding's method for the host tests (float32 results of the float64 values)."""
import math

import torch

from dlsg_amd.hip import normalised_weights
from emul_ensemble import EnsembleEmul, combined_logp

INF = float('inf')
NAN = float('nan')


def combined_rows(rows, weights, mode):
    """(N, V) float64 combined values of N positions from the members' (N, V) rows.  Rows without a NaN and with a finite entry:
    `combined_logp`.  A member row that is all -inf or holds a NaN has lse = NaN, so its log-probs are all NaN: one member, or
    mode 1, gives NaN; mode 0 takes the maximum over the members' v = l + log w with fmaxf, which skips a NaN -- NaN where another
    member gives the class a value above -inf, -inf where none does."""
    M = len(rows)
    c = combined_logp(rows, weights, mode)
    bad = torch.stack([x.isnan().any(1) | (x == -INF).all(1) for x in rows])            # (M, N)
    w = normalised_weights(weights)
    for i in bad.any(0).nonzero().flatten().tolist():
        if M == 1 or mode == 1:
            c[i] = NAN
            continue
        v = torch.stack([torch.full_like(x[i], NAN, dtype=torch.float64) if bad[m, i]
                         else torch.log_softmax(x[i].double(), 0) + math.log(w[m]) for m, x in enumerate(rows)])
        mx = torch.where(v.isnan(), torch.full_like(v, -INF), v).max(0).values
        c[i] = torch.where(mx == -INF, mx, torch.full_like(mx, NAN))
    return c


def caption_lens(ids, lens, end):
    R, L = ids.shape
    if lens is not None:
        return lens.clamp(0, L).to(torch.int64)
    is_end = ids == end
    return torch.where(is_end.any(1), is_end.int().argmax(1) + 1, torch.full((R,), L))


def seq_logprob_f64(logits_list, weights, mode, ids, lens=None, alpha=0.0, end=-1):
    """-> dict(tok_lp (R, L) float64, tok_rank (R, L) int64, lp (R) float64, scores (R) float64, lens (R) int64, margin (R, L)
    float64: the distance from the target's value to the nearest other class's (inf behind the caption and for a bad target)).
    logits_list: (L, R, V) views, as the binding takes them."""
    R, L = ids.shape
    V = logits_list[0].shape[2]
    M = len(logits_list)
    ln = caption_lens(ids, lens, end)
    tok = torch.zeros(R, L, dtype=torch.float64)
    rank = torch.full((R, L), -1, dtype=torch.int64)
    margin = torch.full((R, L), INF, dtype=torch.float64)
    pos = [(r, t) for r in range(R) for t in range(int(ln[r]))]
    ok = [(r, t) for r, t in pos if 0 <= int(ids[r, t]) < V]
    for r, t in pos:
        tok[r, t] = NAN                                          # a target outside [0, V): NaN, rank -1
    if ok:
        rr = torch.tensor([p[0] for p in ok])
        tt = torch.tensor([p[1] for p in ok])
        rows = [x[tt, rr] for x in logits_list]                     # (N, V) each
        c = combined_rows(rows, weights, mode)
        tgt = ids[rr, tt]
        ct = c.gather(1, tgt.unsqueeze(1))
        tok[rr, tt] = ct[:, 0]
        key = rows[0].double() if M == 1 else c                    # one model ranks on the raw logits
        kt = key.gather(1, tgt.unsqueeze(1))
        j = torch.arange(V).unsqueeze(0)
        rank[rr, tt] = ((key > kt) | ((key == kt) & (j < tgt.unsqueeze(1)))).sum(1)
        gap = (key - kt).abs()
        gap[j == tgt.unsqueeze(1)] = INF
        gap[gap.isnan()] = INF
        margin[rr, tt] = gap.min(1).values
    lp = torch.zeros(R, dtype=torch.float64)
    for r in range(R):
        for t in range(int(ln[r])):
            lp[r] = tok[r, t] + lp[r]
    scores = torch.where(ln > 0, lp / ln.double().clamp(min=1) ** alpha, torch.zeros_like(lp))
    return dict(tok_lp=tok, tok_rank=rank, lp=lp, scores=scores, lens=ln, margin=margin)


class SeqScoreEmul(EnsembleEmul):
    def rows_repeat(self, x, y, n):
        """the fan-out of a clip's memories to its n caption rows (several candidates per clip on one encoder pass)"""
        assert y.shape[0] == x.shape[0] * n and y.shape[1:] == x.shape[1:]
        y.copy_(x.repeat_interleave(n, 0))

    def seq_logprob(self, logits_list, weights, mode, ids, lens=None, length_penalty=0.0, want_tokens=False, want_ranks=False, end=-1):
        assert len(logits_list) == len(weights) and mode in (0, 1) and ids.dtype == torch.int64
        for x in logits_list:
            assert x.dim() == 3 and x.shape[0] >= ids.shape[1] and x.shape[1] == ids.shape[0], (x.shape, ids.shape)
        out = seq_logprob_f64(logits_list, weights, mode, ids, lens, length_penalty, end)
        return (out['scores'].float(), out['lens'], out['lp'].float(), out['tok_lp'].float() if want_tokens else None,
                out['tok_rank'].int() if want_ranks else None)

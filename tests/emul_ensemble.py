"""Test-only restatement of the ensemble beam step (dlsg_beam_select_ens) on top of tests/emul_beam.py: the combined values in
float64 from torch.log_softmax, the selection by the rules of BeamEmul.beam_select_hist, and per clip the gap -- how far the
step was from choosing differently -- so that a comparison with the float32 kernel can leave near-ties out."""
import math

import torch

from dlsg_amd.hip import normalised_weights
from emul_beam import BeamEmul, banned_classes

INF = float('inf')


def combined_logp(logits_list, weights, mode):
    """(R, V) float64: mode 0 the log of the weighted mean probability, mode 1 the weighted mean log-probability"""
    w = normalised_weights(weights)
    logp = [torch.log_softmax(x.double(), 1) for x in logits_list]
    if mode == 0:
        return torch.logsumexp(torch.stack([l + math.log(wm) for l, wm in zip(logp, w)]), 0)
    out = torch.zeros_like(logp[0])
    for l, wm in zip(logp, w):
        out = out + wm * l
    return out


def neighbour_gap(values):
    """the smallest difference of two neighbours of a descending list, -inf entries left out"""
    fin = [v for v in values if v > -INF]
    return min([INF] + [a - b for a, b in zip(fin, fin[1:])])


class EnsembleEmul(BeamEmul):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gap = None                                        # of the last beam_select_ens call: (B,) float64

    def beam_select_ens(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                        no_repeat_ngram=0, min_len=0, ended_count=None):
        assert len(logits_list) == len(weights) and mode in (0, 1)
        R, V = logits_list[0].shape
        B = R // k
        first = t == 0
        c = combined_logp(logits_list, weights, mode)            # of the whole rows: a ban does not renormalise
        live = [first or int(last[r]) != end for r in range(R)]
        for r in range(R):
            if live[r]:
                for cls in banned_classes(hist_in[r, :t].tolist(), t, no_repeat_ngram, min_len, end):
                    c[r, cls] = -INF
            else:
                c[r] = -INF
                c[r, end] = 0.0
        nbeam = 1 if first else k
        base = torch.zeros(R, dtype=torch.float64) if first else last_lp.double()
        node_lp, node_cls = c.sort(dim=1, descending=True, stable=True)             # ties to the lower class
        gap = torch.full((B,), INF, dtype=torch.float64)
        for b in range(B):
            cand = []                                                            # (value, parent, class) in candidate-index order
            for j in range(nbeam):
                r = b * k + j
                if live[r]:
                    gap[b] = min(float(gap[b]), neighbour_gap(node_lp[r, :k + 1].tolist()))
                cand += [(float(node_lp[r, q] + base[r]), j, int(node_cls[r, q])) for q in range(k)]
            order = sorted(range(len(cand)), key=lambda i: (-cand[i][0], i))
            gap[b] = min(float(gap[b]), neighbour_gap([cand[i][0] for i in order[:k + 1]]))
            for q, i in enumerate(order[:k]):
                o = b * k + q
                pred[o], new_lp[o], back[o], rows[o] = cand[i][2], cand[i][0], cand[i][1], b * k + cand[i][1]
        self.gap = gap
        h = hist_in[rows].clone() if t else torch.empty_like(hist_out)
        h[:, t] = pred
        h[:, t + 1:] = end
        hist_out.copy_(h)
        if ended_count is not None:
            ended_count += int((pred == end).sum())

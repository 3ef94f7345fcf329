"""Test-only restatement of the beam step with exclusions (dlsg_beam_select_excl) on top of tests/emul_ensemble.py: the ensemble
emulation -- combined values in float64, selection by the rules of EnsembleEmul.beam_select_ens, the per-clip gap -- with the ban
set of a live row extended by the last words of the excluded entries its history leads up to.  `excluded_word` states that rule
once more for one row and one entry on plain lists; the emulator does not call it."""
import torch

from emul_beam import banned_classes
from emul_ensemble import INF, EnsembleEmul, combined_logp, neighbour_gap

NO_CLASS = 0x7fffffff                                          # the class of a slot of a row that offers nothing


def excluded_word(h, entry, V):
    """The word that `entry` (a list of ids, P long) bans for a live row with history h (a list, the t words so far), or None:
    the entry is the ids before the first one outside [0, V); its last word is banned iff the words before it are the last words
    of h.  Lists and integers only."""
    e = []
    for i in entry:
        if not 0 <= i < V:
            break
        e.append(i)
    if not e:
        return None
    context = e[:-1]
    if len(context) > len(h):
        return None
    for back in range(1, len(context) + 1):
        if h[-back] != context[-back]:
            return None
    return e[-1]


def table_entries(shared, per_clip, B, V):
    """per clip the tuples of its entries, the shared ones first, each cut to its run of ids in [0, V); absent entries left out"""
    def cut(row):
        ok = [0 <= i < V for i in row]
        return tuple(row[:ok.index(False)] if False in ok else row)
    sh = [] if shared is None else [cut(r) for r in shared.tolist()]
    out = []
    for b in range(B):
        own = [] if per_clip is None else [cut(r) for r in per_clip[b].tolist()]
        out.append([e for e in sh + own if e])
    return out


class ExclEmul(EnsembleEmul):
    def beam_select_excl(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                         excl_shared=None, excl_clip=None, no_repeat_ngram=0, min_len=0, ended_count=None):
        assert len(logits_list) == len(weights) and mode in (0, 1)
        R, V = logits_list[0].shape
        B = R // k
        first = t == 0
        entries = table_entries(excl_shared, excl_clip, B, V)
        # of the whole rows: a ban does not renormalise.  One member of weight 1: x - lse in float32, the value the one-model step
        # (BeamEmul.beam_select_hist) ranks by and adds in float32 -- the float64 sum of two float32, stored as float32, is that sum
        c = torch.log_softmax(logits_list[0], 1).double() if len(logits_list) == 1 else combined_logp(logits_list, weights, mode)
        live = [first or int(last[r]) != end for r in range(R)]
        dead = [False] * R                                       # a live row with a NaN: its log-sum-exp is NaN, it offers nothing
        for r in range(R):
            if live[r]:
                if bool(torch.isnan(c[r]).any()):
                    dead[r] = True
                    c[r] = -INF
                    continue
                h = tuple(hist_in[r, :t].tolist())
                for cls in banned_classes(list(h), t, no_repeat_ngram, min_len, end):
                    c[r, cls] = -INF
                for e in entries[r // k]:
                    if len(e) - 1 <= t and h[t - (len(e) - 1):] == e[:-1]:
                        c[r, e[-1]] = -INF
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
                if live[r] and not dead[r]:
                    gap[b] = min(float(gap[b]), neighbour_gap(node_lp[r, :k + 1].tolist()))
                cand += [(float(node_lp[r, q] + base[r]), j, NO_CLASS if dead[r] else int(node_cls[r, q])) for q in range(k)]
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

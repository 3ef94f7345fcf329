"""Test-only restatement of the diverse beam step (dlsg_beam_select_groups) on top of tests/emul_ensemble.py: phase 1 as
EnsembleEmul.beam_select_ens takes it (combined values in float64, the bans, stable sorts), phase 2 -- the groups in order with the
Hamming penalty -- on Python lists in float64.  Per clip the gap: the smallest neighbour difference among each live row's k + 1 best
values and each group's k' + 1 best keys, so that a comparison with the float32 kernel can leave near-ties out."""
import torch

from emul_beam import banned_classes
from emul_ensemble import EnsembleEmul, combined_logp, neighbour_gap

INF = float('inf')


def group_choice(cand, live, kg, cnt, penalty):
    """One group's choice.  cand: [(lp, parent, class)] in candidate order, live[parent]; cnt {class: count}.  Returns (picks, keys):
    picks kg entries (candidate index, lp or -inf for a slot left over, counted?), keys the descending list of the finite keys."""
    keys = []
    for lp, parent, cls in cand:
        c = cnt.get(cls, 0)
        if not live[parent] or c == 0:
            keys.append(lp)
        else:
            keys.append(-INF if penalty == INF else lp - penalty * c)
    order = [i for i in sorted(range(len(cand)), key=lambda i: (-keys[i], i)) if keys[i] > -INF]     # stable: ties to the lower index
    picks = [(i, cand[i][0], live[cand[i][1]]) for i in order[:kg]]
    picks += [(q, -INF, False) for q in range(len(picks), kg)]                  # a -inf key is no candidate: slot q, not counted
    return picks, [keys[i] for i in order]


class GroupsEmul(EnsembleEmul):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.changed = None        # of the last beam_select_groups call: [(clip, group >= 1, chose differently than with penalty 0)]

    def beam_select_groups(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                           no_repeat_ngram=0, min_len=0, num_groups=1, diversity_penalty=0.0, ended_count=None):
        assert len(logits_list) == len(weights) and mode in (0, 1)
        G, penalty = int(num_groups), float(diversity_penalty)
        assert G >= 1 and k % G == 0 and penalty >= 0.0
        kg = k // G
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
        base = torch.zeros(R, dtype=torch.float64) if first else last_lp.double()
        node_lp, node_cls = c.sort(dim=1, descending=True, stable=True)             # ties to the lower class
        gap = torch.full((B,), INF, dtype=torch.float64)
        changed = []
        for b in range(B):
            for j in range(1 if first else k):
                if live[b * k + j]:
                    gap[b] = min(float(gap[b]), neighbour_gap(node_lp[b * k + j, :k + 1].tolist()))
            lists = {j: [(float(node_lp[b * k + j, q] + base[b * k + j]), int(node_cls[b * k + j, q])) for q in range(k)]
                     for j in range(1 if first else k)}
            clip_live = [live[b * k + j] for j in range(k)]
            cnt = {}
            for y in range(G):
                if first:                                                         # the clip's one list, parent = the group's first row
                    cand = [(lp, y * kg, cls) for lp, cls in lists[0]]
                else:
                    cand = [(lp, j, cls) for j in range(y * kg, (y + 1) * kg) for lp, cls in lists[j]]
                picks, keys = group_choice(cand, clip_live, kg, cnt, penalty)
                gap[b] = min(float(gap[b]), neighbour_gap(keys[:kg + 1]))
                if y:
                    plain = group_choice(cand, clip_live, kg, {}, 0.0)[0]
                    changed.append((b, y, [p[0] for p in plain] != [p[0] for p in picks]))
                for q, (i, lp, counted) in enumerate(picks):
                    o = b * k + y * kg + q
                    pred[o], new_lp[o], back[o], rows[o] = cand[i][2], lp, cand[i][1], b * k + cand[i][1]
                for i, lp, counted in picks:                                     # after the group has chosen
                    if counted:
                        cnt[cand[i][2]] = cnt.get(cand[i][2], 0) + 1
        self.gap, self.changed = gap, changed
        h = hist_in[rows].clone() if t else torch.empty_like(hist_out)
        h[:, t] = pred
        h[:, t + 1:] = end
        hist_out.copy_(h)
        if ended_count is not None:
            ended_count += int((pred == end).sum())

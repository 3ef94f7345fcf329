"""Test-only restatement of the lexically constrained beam step (dlsg_beam_select_cons) on top of tests/emul_beam.py: `cons_step`
works on numpy arrays -- the log-softmax is torch's float32 one, as in BeamEmul.beam_select_hist, every rule of the step is
written out per row and per clip -- and returns, per clip, the GAP: the smallest difference the outcome rests on.  `ConsEmul` puts
it behind the signature of `HipOps.beam_select_cons`; the host tests run `beam.constrained_nbest` through it and the GPU tests
compare the kernel with it."""
import numpy as np
import torch

from emul_beam import BeamEmul, banned_classes

INF = float('inf')


def valid_sets(cons_b, V):
    """the valid entries of a clip's constraints: a list of C sets (an empty set: the constraint is absent)"""
    return [{int(i) for i in row if 0 <= int(i) < V} for row in cons_b]


def mask_of(sets, cls):
    return sum(1 << c for c, s in enumerate(sets) if cls in s)


def cons_step(x, last, last_lp, hist_in, k, end, t, g, min_len, cons):
    """x (R, V) float32 logits (torch), the other inputs numpy; cons (B, C, W) int64 numpy or None.  -> dict of pred, new_lp, back,
    rows, hist_out, met_out, n_end, gap (B,), stats"""
    R, V = x.shape
    B, L = R // k, hist_in.shape[1]
    logp = torch.log_softmax(x, 1).numpy()                            # float32, of the whole row
    raw = x.numpy()
    C = 0 if cons is None else cons.shape[1]
    nbeam = 1 if t == 0 else k
    out = dict(pred=np.zeros(R, np.int64), new_lp=np.zeros(R, np.float32), back=np.zeros(R, np.int64), rows=np.zeros(R, np.int64),
               hist_out=np.full((R, L), end, np.int64), met_out=np.zeros(R, np.int32), gap=np.full(B, INF))
    stats = dict(list_b=0, dedup=0, multi_bank=0, end_blocked=0, leftover=0, mixed_met=0)
    n_end = 0
    for b in range(B):
        sets = valid_sets(cons[b], V) if C else []
        present = sum(1 << c for c, s in enumerate(sets) if s)
        gap = INF
        A, Bl, mets = [], [], []                                      # candidates: (value, class, parent)
        for w in range(nbeam):
            r = b * k + w
            h = [int(v) for v in hist_in[r, :t]]
            met = 0
            for tok in h:
                met |= mask_of(sets, tok)
            mets.append(met)
            unmet = present & ~met
            base = np.float32(0.0) if t == 0 else np.float32(last_lp[r])
            if t > 0 and int(last[r]) == end:
                A.append((base, end, w))
                A += [(np.float32(-INF), (q - 1 if q - 1 < end else q), w) for q in range(1, k)]
                Bl += [(np.float32(-INF), 0, w)] * C
                continue
            banned = banned_classes(h, t, g, min_len, end)
            if unmet:
                if end not in banned and not np.isnan(raw[r, end]):
                    sel0 = np.where(np.isnan(raw[r]), -INF, raw[r]).copy()
                    for c in banned:
                        sel0[c] = -INF
                    stats['end_blocked'] += int((sel0 > sel0[end]).sum() < k and sel0[end] > -INF)
                banned = banned | {end}
            sel = raw[r].astype(np.float64).copy()
            nan = np.isnan(sel)
            for c in banned:
                sel[c] = -INF
            sel[nan] = -INF
            order = np.lexsort((np.arange(V), -sel))                 # larger value first, ties to the lower class
            order = [int(c) for c in order if not nan[c]][:k + 1]
            assert len(order) >= k, 'fewer than k classes that are not NaN'
            rowA = order[:k]
            ok_row = not np.isnan(logp[r]).all()                     # a NaN in the row: its log-sum-exp, hence every value, is NaN
            if ok_row and len(order) > k and sel[order[k - 1]] > -INF:
                gap = min(gap, sel[order[k - 1]] - sel[order[k]])
            for c in rowA:
                A.append((np.float32(-INF) if sel[c] == -INF and ok_row else np.float32(logp[r, c]) + base, c, w))
            taken = []
            for c in range(C):
                slot = (np.float32(-INF), 0, w)
                if unmet >> c & 1:
                    words = sorted((i for i in sets[c] if i not in banned and raw[r, i] > -INF), key=lambda i: (-raw[r, i], i))
                    if words:
                        if ok_row and len(words) > 1:
                            gap = min(gap, float(raw[r, words[0]]) - float(raw[r, words[1]]))
                        if words[0] in rowA or words[0] in taken:
                            stats['dedup'] += ok_row
                        else:
                            taken.append(words[0])
                            slot = (np.float32(logp[r, words[0]]) + base, words[0], w)
                Bl.append(slot)
        stats['mixed_met'] += len({bin(m).count('1') for m in mets}) > 1
        # ---- banks and allocation
        cands = []                                                    # (bank, value, index, class, parent, mask)
        for lst, first in ((A, 0), (Bl, 64)):
            for i, (v, cls, w) in enumerate(lst):
                if v > -INF:                                          # (a NaN is no candidate)
                    m = mets[w] | mask_of(sets, cls)
                    cands.append((bin(m).count('1'), float(v), first + i, cls, w, m))
        for bank in {c[0] for c in cands}:
            vals = sorted(c[1] for c in cands if c[0] == bank)
            if len(vals) > 1:
                gap = min(gap, float(np.diff(vals).min()))
        picks, left = [], list(cands)
        while len(picks) < k and left:
            for bank in range(C, -1, -1):
                inb = [c for c in left if c[0] == bank]
                if not inb or len(picks) == k:
                    continue
                inb.sort(key=lambda c: (-c[1], c[2]))
                if len(inb) > 1:
                    gap = min(gap, inb[0][1] - inb[1][1])
                picks.append(inb[0])
                left.remove(inb[0])
        stats['multi_bank'] += len({p[0] for p in picks}) > 1
        stats['list_b'] += sum(p[2] >= 64 for p in picks)
        stats['leftover'] += k - len(picks)
        for q in range(k):
            o = b * k + q
            if q < len(picks):
                _, v, _, cls, w, m = picks[q]
            else:
                v, cls, w, m = -INF, A[q][1], 0, 0
            out['pred'][o], out['new_lp'][o], out['back'][o], out['rows'][o], out['met_out'][o] = cls, v, w, b * k + w, m
            out['hist_out'][o, :t] = hist_in[b * k + w, :t]
            out['hist_out'][o, t] = cls
            n_end += cls == end
        out['gap'][b] = gap
    out['n_end'], out['stats'] = n_end, stats
    return out


class ConsEmul(BeamEmul):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.gap, self.stats = None, None                              # of the last beam_select_cons call

    def beam_select_cons(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, cons, no_repeat_ngram=0,
                         min_len=0, ended_count=None, met_out=None):
        if cons is not None and cons.shape[1] == 0:
            cons = None
        out = cons_step(logits.float(), last.numpy(), last_lp.numpy(), hist_in.numpy(), k, end, t, no_repeat_ngram, min_len,
                        None if cons is None else cons.numpy())
        pred.copy_(torch.from_numpy(out['pred'])); new_lp.copy_(torch.from_numpy(out['new_lp']))
        back.copy_(torch.from_numpy(out['back'])); rows.copy_(torch.from_numpy(out['rows']))
        hist_out.copy_(torch.from_numpy(out['hist_out']))
        if met_out is not None:
            met_out.copy_(torch.from_numpy(out['met_out']))
        if ended_count is not None:
            ended_count += int(out['n_end'])
        self.gap, self.stats = torch.from_numpy(out['gap']), out['stats']

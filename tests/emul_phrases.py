"""Test-only restatement of the constrained beam step with multi-word phrases (dlsg_beam_select_phrases, the rules of include/dlsg.h)
on top of tests/emul_constrained.py: `phrase_step` works on numpy arrays as `cons_step` does -- the log-softmax is torch's float32
one, every rule is written out per row and per clip, and what a history has met and how far into a phrase it is are computed from
the definitions, on the whole history of every candidate -- and returns, per clip, the GAP: the smallest margin any choice of the
step rests on.  `PhraseEmul` puts it behind the signature of `HipOps.beam_select_phrases`; the host tests run
`beam.constrained_nbest` through it and the GPU tests compare the kernel with it."""
import numpy as np
import torch

from emul_beam import banned_classes
from emul_constrained import INF, ConsEmul

PHRASE_MAX = 4                                                         # DLSG_PHRASE_MAX


def alternatives(phr_b, V):
    """a clip's constraints as C lists of phrases (tuples): the leading run of ids in [0, V) of every alternative, absent ones left out"""
    out = []
    for con in phr_b:
        alts = []
        for row in con:
            a = []
            for i in row:
                if not 0 <= int(i) < V:
                    break
                a.append(int(i))
            if a:
                alts.append(tuple(a))
        out.append(alts)
    return out


def occurs(h, a):
    return any(tuple(h[i:i + len(a)]) == a for i in range(len(h) - len(a) + 1))


def progress(h, a):
    """the largest j <= min(n - 1, t) such that the last j tokens of h are the first j words of a"""
    return max(j for j in range(min(len(a) - 1, len(h)) + 1) if j == 0 or tuple(h[len(h) - j:]) == a[:j])


def row_state(h, alts):
    """(met mask, progress q) of a history"""
    met = sum(1 << c for c, al in enumerate(alts) if any(occurs(h, a) for a in al))
    q = max([progress(h, a) for c, al in enumerate(alts) if not met >> c & 1 for a in al] + [0])
    return met, q


def phrase_step(x, last, last_lp, hist_in, k, end, t, g, min_len, phr):
    """x (R, V) float32 logits (torch), the other inputs numpy; phr (B, C, W, P) int64 numpy or None.  -> dict of pred, new_lp, back,
    rows, hist_out, met_out, bank_out, n_end, gap (B,), stats"""
    R, V = x.shape
    B, L = R // k, hist_in.shape[1]
    logp = torch.log_softmax(x, 1).numpy()                            # float32, of the whole row
    raw = x.numpy()
    C = 0 if phr is None else phr.shape[1]
    P = 1 if phr is None else phr.shape[3]
    nbeam = 1 if t == 0 else k
    out = dict(pred=np.zeros(R, np.int64), new_lp=np.zeros(R, np.float32), back=np.zeros(R, np.int64), rows=np.zeros(R, np.int64),
               hist_out=np.full((R, L), end, np.int64), met_out=np.zeros(R, np.int32), bank_out=np.zeros(R, np.int32),
               gap=np.full(B, INF))
    stats = dict(list_b=0, dedup=0, multi_bank=0, end_blocked=0, leftover=0, completes=0, progress_bank=0, gain_decides=0)
    n_end = 0
    for b in range(B):
        alts = alternatives(phr[b], V) if C else []
        present = sum(1 << c for c, al in enumerate(alts) if al)
        gap = INF
        A, Bl, hists, states = [], [], [], []                         # candidates: (value, class, parent)
        for w in range(nbeam):
            r = b * k + w
            h = [int(v) for v in hist_in[r, :t]]
            met, q = row_state(h, alts)
            hists.append(h)
            states.append((met, q))
            unmet = present & ~met
            base = np.float32(0.0) if t == 0 else np.float32(last_lp[r])
            if t > 0 and int(last[r]) == end:
                A.append((base, end, w))
                A += [(np.float32(-INF), (i - 1 if i - 1 < end else i), w) for i in range(1, k)]
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
                    props = {}                                        # class -> its largest gain
                    for a in alts[c]:
                        p = progress(h, a)
                        u = a[p]
                        if u not in banned and raw[r, u] > -INF:
                            props[u] = max(props.get(u, 0), P if p + 1 == len(a) else p + 1)
                    if props:
                        top = max(props.values())
                        words = sorted((u for u, s in props.items() if s == top), key=lambda u: (-raw[r, u], u))
                        if ok_row and len(words) > 1:
                            gap = min(gap, float(raw[r, words[0]]) - float(raw[r, words[1]]))
                        best_any = min(props, key=lambda u: (-raw[r, u], u))
                        stats['gain_decides'] += ok_row and best_any != words[0]
                        if words[0] in rowA or words[0] in taken:
                            stats['dedup'] += ok_row
                        else:
                            taken.append(words[0])
                            slot = (np.float32(logp[r, words[0]]) + base, words[0], w)
                Bl.append(slot)
        # ---- banks and allocation
        cands = []                                                    # (bank, value, index, class, parent, mask)
        for lst, first in ((A, 0), (Bl, 64)):
            for i, (v, cls, w) in enumerate(lst):
                if v > -INF:                                          # (a NaN is no candidate)
                    m, q = states[w] if cls == end else row_state(hists[w] + [cls], alts)
                    cands.append((bin(m).count('1') * PHRASE_MAX + q, float(v), first + i, cls, w, m))
        for bank in {c[0] for c in cands}:
            vals = sorted(c[1] for c in cands if c[0] == bank)
            if len(vals) > 1:
                gap = min(gap, float(np.diff(vals).min()))
        picks, left = [], list(cands)
        while len(picks) < k and left:
            for bank in sorted({c[0] for c in left}, reverse=True):
                inb = [c for c in left if c[0] == bank]
                if len(picks) == k:
                    break
                inb.sort(key=lambda c: (-c[1], c[2]))
                if len(inb) > 1:
                    gap = min(gap, inb[0][1] - inb[1][1])
                picks.append(inb[0])
                left.remove(inb[0])
        stats['multi_bank'] += len({p[0] for p in picks}) > 1
        stats['list_b'] += sum(p[2] >= 64 for p in picks)
        stats['leftover'] += k - len(picks)
        stats['completes'] += sum(p[3] != end and bin(p[5]).count('1') > bin(states[p[4]][0]).count('1') for p in picks)
        stats['progress_bank'] += sum(p[0] % PHRASE_MAX > 0 for p in picks)
        for i in range(k):
            o = b * k + i
            if i < len(picks):
                bank, v, _, cls, w, m = picks[i]
            else:
                bank, v, cls, w, m = 0, -INF, A[i][1], 0, 0
            out['pred'][o], out['new_lp'][o], out['back'][o], out['rows'][o] = cls, v, w, b * k + w
            out['met_out'][o], out['bank_out'][o] = m, bank
            out['hist_out'][o, :t] = hist_in[b * k + w, :t]
            out['hist_out'][o, t] = cls
            n_end += cls == end
        out['gap'][b] = gap
    out['n_end'], out['stats'] = n_end, stats
    return out


class PhraseEmul(ConsEmul):
    def beam_select_phrases(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, phr, no_repeat_ngram=0,
                            min_len=0, ended_count=None, met_out=None, bank_out=None):
        if phr is not None and phr.shape[1] == 0:
            phr = None
        out = phrase_step(logits.float(), last.numpy(), last_lp.numpy(), hist_in.numpy(), k, end, t, no_repeat_ngram, min_len,
                          None if phr is None else phr.numpy())
        pred.copy_(torch.from_numpy(out['pred'])); new_lp.copy_(torch.from_numpy(out['new_lp']))
        back.copy_(torch.from_numpy(out['back'])); rows.copy_(torch.from_numpy(out['rows']))
        hist_out.copy_(torch.from_numpy(out['hist_out']))
        if met_out is not None:
            met_out.copy_(torch.from_numpy(out['met_out']))
        if bank_out is not None:
            bank_out.copy_(torch.from_numpy(out['bank_out']))
        if ended_count is not None:
            ended_count += int(out['n_end'])
        self.gap, self.stats = torch.from_numpy(out['gap']), out['stats']

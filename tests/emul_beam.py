"""Test-only torch / numpy restatement of the two n-best beam-search kernels (dlsg_beam_select_hist, dlsg_beam_finalize) on top of
tests/emul_ops.py; the host tests run `beam.beam_nbest` through it, the GPU tests compare the kernels with it."""
import torch

from emul_ops import EmulOps


def banned_classes(h, t, g, min_len, end):
    """the classes a live beam with history h[0..t-1] may not choose at step t"""
    banned = set()
    if g > 0 and t >= g:
        tail = h[t - g + 1:t]
        for i in range(t - g + 1):
            if h[i:i + g - 1] == tail:
                banned.add(h[i + g - 1])
    if t < min_len:
        banned.add(end)
    return banned


class BeamEmul(EmulOps):
    def beam_select_hist(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram=0,
                         min_len=0, ended_count=None):
        R, V = logits.shape
        B = R // k
        first = t == 0
        logp = torch.log_softmax(logits, 1)                      # of the whole row: a ban does not renormalise
        for r in range(R):
            if first or int(last[r]) != end:
                for c in banned_classes(hist_in[r, :t].tolist(), t, no_repeat_ngram, min_len, end):
                    logp[r, c] = float('-inf')
        if first:
            lp, cls = logp.view(B, k, V)[:, 0].topk(k)
            pred.copy_(cls.reshape(R)); new_lp.copy_(lp.reshape(R)); back.zero_()
            rows.copy_((torch.arange(B).unsqueeze(1) * k).expand(B, k).reshape(R))
        else:
            after_end = torch.full((R, V), float('-inf'))
            after_end[:, end] = 0.0
            cleaned = torch.where((last == end).unsqueeze(-1), after_end, logp)
            node_lp, node_cls = cleaned.topk(k)
            summed = (node_lp + last_lp.reshape(R, 1)).reshape(B, k * k)
            best_lp, best_idx = summed.topk(k)
            pred.copy_(node_cls.reshape(B, k * k).gather(1, best_idx).reshape(R))
            new_lp.copy_(best_lp.reshape(R))
            bk = (best_idx / k).type(torch.int64)
            back.copy_(bk.reshape(R))
            rows.copy_((torch.arange(B).unsqueeze(1) * k + bk).reshape(R))
        h = hist_in[rows].clone() if t else torch.empty_like(hist_out)
        h[:, t] = pred
        h[:, t + 1:] = end
        hist_out.copy_(h)
        if ended_count is not None:
            ended_count += int((pred == end).sum())

    def beam_finalize(self, hist, lp, k, end, alpha, ids, scores, lens):
        R, L = hist.shape
        B, n = R // k, ids.shape[1]
        is_end = hist == end
        ln = torch.where(is_end.any(1), is_end.int().argmax(1) + 1, torch.full((R,), L))
        sc = (lp.double() / ln.double() ** alpha).float().view(B, k)
        top, order = sc.sort(dim=1, descending=True, stable=True)
        order = order[:, :n]
        ids.copy_(hist.view(B, k, L).gather(1, order.unsqueeze(2).expand(B, n, L)))
        scores.copy_(top[:, :n])
        lens.copy_(ln.view(B, k).gather(1, order))

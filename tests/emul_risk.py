"""Test-only numpy emulation of the two launches of the minimum-risk loss (csrc/risk.hip, include/addons/dlsg_risk.h), following the
kernels' own steps and number formats -- float32 row maximum, exponential sum, lse and token term; float64 per clip, the token
terms summed over t ascending; float32 weight c and gradient row -- and the ops mixin on top of it (`RiskOps`).  Only the order
inside the float32 row sums differs from the device's (numpy's pairwise sum against the workgroup's strided one)."""
import numpy as np
import torch

MAX_N, MAX_L = 32, 64


def _rows_view(a, rows, L, time_major):
    """(rows, L, ...) view of an array stored in the logits' row order"""
    a = a.reshape((L, rows) + a.shape[1:]) if time_major else a.reshape((rows, L) + a.shape[1:])
    return np.swapaxes(a, 0, 1) if time_major else a


def emul_risk_rows(logits, targets, lens, time_major):
    """-> (lse, tok_lp), float32 arrays of rows * L in the logits' row order"""
    if time_major:
        L, rows, V = logits.shape
    else:
        rows, L, V = logits.shape
    x = _rows_view(np.asarray(logits, dtype=np.float32).reshape(rows * L, V), rows, L, time_major)
    lse = np.zeros((rows, L), dtype=np.float32)
    tok = np.zeros((rows, L), dtype=np.float32)
    for r in range(rows):
        for t in range(min(int(lens[r]), L)):
            row = x[r, t]
            m = row.max()
            with np.errstate(divide='ignore', invalid='ignore'):
                l = np.float32(np.log(np.exp(row - m, dtype=np.float32).sum(dtype=np.float32))) + m
            tgt = int(targets[r, t])
            bad = tgt < 0 or tgt >= V
            lse[r, t] = np.nan if bad else l
            tok[r, t] = np.nan if bad else row[tgt] - l
    back = (lambda a: np.ascontiguousarray(a.T).reshape(-1)) if time_major else (lambda a: a.reshape(-1))
    return back(lse), back(tok)


def emul_risk_grad(logits, targets, lens, lse, tok_lp, rewards, valid, n, time_major, alpha, length_penalty):
    """-> dict(dlogits (as logits, float32), Q, s (rows,), R (rows / n,), loss (float32), stats (4,))"""
    if time_major:
        L, rows, V = logits.shape
    else:
        rows, L, V = logits.shape
    B = rows // n
    x = _rows_view(np.asarray(logits, dtype=np.float32).reshape(rows * L, V), rows, L, time_major)
    lse2, tok2 = _rows_view(np.asarray(lse), rows, L, time_major), _rows_view(np.asarray(tok_lp), rows, L, time_major)
    ln = np.minimum(np.asarray(lens, dtype=np.int64), L)
    rewards = np.asarray(rewards, dtype=np.float64)
    Q, S, R = np.zeros(rows), np.zeros(rows), np.zeros(B)
    c = np.zeros(rows, dtype=np.float32)
    counted = np.zeros(rows, dtype=bool)
    with np.errstate(all='ignore'):
        for b in range(B):
            cr = np.arange(b * n, b * n + n)
            s = np.zeros(n)
            for i in range(n):
                for t in range(int(ln[cr[i]])):
                    s[i] += np.float64(tok2[cr[i], t])
            v = (ln[cr] >= 1) & (s != -np.inf)
            if valid is not None:
                v &= np.asarray(valid)[cr].astype(bool)
            a = np.where(v, alpha / np.maximum(ln[cr], 1).astype(np.float64) ** length_penalty, 0.0)
            z = np.where(v, a * np.where(v, s, 0.0), -np.inf)
            m = np.fmax.reduce(z) if n else -np.inf
            e = np.where(v, np.exp(np.where(v, z - m, 0.0)), 0.0)
            q = np.where(v, e / e.sum(), 0.0)
            rew = np.where(v, rewards[cr], 0.0)
            Rb = (q * rew).sum()
            Q[cr], S[cr], R[b] = q, s, Rb
            c[cr] = np.where(v, a * q * (rew - Rb) / B, 0.0).astype(np.float32)
            counted[cr] = v
        dl = np.zeros((rows, L, V), dtype=np.float32)
        for r in range(rows):
            if c[r] == 0:                            # (NaN is not 0: a NaN clip's rows go through the arithmetic)
                continue
            for t in range(max(int(ln[r]), 0)):
                p = np.exp(x[r, t] - lse2[r, t], dtype=np.float32)
                tgt = int(targets[r, t])
                if 0 <= tgt < V:
                    p[tgt] -= np.float32(1)
                dl[r, t] = c[r] * p
    N = counted.sum()
    ER = R.sum() / B
    stats = np.array([-ER, rewards[counted].sum() / N if N else 0.0, ln[counted].sum() / N if N else 0.0, ER])
    dl = np.ascontiguousarray(np.swapaxes(dl, 0, 1)) if time_major else dl
    return dict(dlogits=dl, Q=Q, s=S, R=R, loss=np.float32(-ER), stats=stats)


class RiskOps(object):
    """mixin for an emulated ops object: the two entry points as `HipOps` offers them, refusing what the launchers refuse"""

    @staticmethod
    def _risk_refuse(what, logits, n, time_major):
        rows, L, V = (logits.shape[1], logits.shape[0], logits.shape[2]) if time_major else logits.shape
        if not (1 <= n <= MAX_N and L <= MAX_L and rows % n == 0 and V >= 1):
            raise RuntimeError('%s failed with code -1' % what)

    def risk_rows(self, logits, targets, lens, lse, tok_lp, n, time_major):
        self._risk_refuse('risk_rows', logits, n, time_major)
        a, b = emul_risk_rows(logits.numpy(), targets.numpy(), lens.numpy(), time_major)
        lse.copy_(torch.from_numpy(a))
        tok_lp.copy_(torch.from_numpy(b))

    def risk_grad(self, logits, targets, lens, lse, tok_lp, rewards, valid, dlogits, Q, s, R, loss, stats, n, time_major, alpha,
                  length_penalty=0.0):
        self._risk_refuse('risk_grad', logits, n, time_major)
        assert rewards.dtype == torch.float64 and (valid is None or valid.dtype == torch.bool)
        out = emul_risk_grad(logits.numpy(), targets.numpy(), lens.numpy(), lse.numpy(), tok_lp.numpy(), rewards.numpy(),
                             None if valid is None else valid.numpy(), n, time_major, alpha, length_penalty)
        dlogits.copy_(torch.from_numpy(out['dlogits']))
        Q.view(-1).copy_(torch.from_numpy(out['Q']))
        s.view(-1).copy_(torch.from_numpy(out['s']))
        R.copy_(torch.from_numpy(out['R']))
        loss.fill_(float(out['loss']))
        stats.copy_(torch.from_numpy(out['stats']))

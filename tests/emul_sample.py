"""Test-only float64 restatement of the filters of dlsg_sample_filter_embed (include/dlsg.h): bans, top-k with ties, the nucleus.
The host tests sample through it (tests/test_sample_filter_host.py), the GPU tests compare the kernel with it."""
import numpy as np

from emul_beam import banned_classes

AMBIGUOUS = 1e-5        # a cumulative-mass boundary this close to top_p: float32 mass sums cannot decide it


def tempered(x, temperature):
    """the kernel's z = x * (1 / temperature) in float32 (temperature 0: x), as float64; x a float32 torch tensor"""
    import torch
    sc = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(temperature), dtype=torch.float32) if temperature > 0 else 1.0
    return (x.float() * sc).double().numpy()


def apply_bans(z, hist, t, no_repeat_ngram, min_len, end):
    """z (rows, V) float64 -> a copy with NaN and the banned classes at -inf; hist: (>= t, rows) earlier words or None"""
    z = np.where(np.isnan(z), -np.inf, z)
    for r in range(z.shape[0]):
        h = [int(hist[i][r]) for i in range(t)] if hist is not None else []
        for c in banned_classes(h, t, no_repeat_ngram if hist is not None else 0, min_len, end):
            if 0 <= c < z.shape[1]:
                z[r, c] = -np.inf
    return z


def kept_row(z, top_k, top_p):
    """one row of banned z (float64, -inf = out) -> (kept mask, larger candidate mask, ambiguous): the kept set of the header's
    rules; when a cumulative-mass boundary lies within AMBIGUOUS of top_p the row is ambiguous and `larger` is the bigger of the
    two sets float32 sums may arrive at (else `larger` is the kept set)."""
    keep = z > -np.inf
    nf = int(keep.sum())
    if nf == 0:
        return keep, keep, False
    if 0 < top_k < nf:
        keep = keep & (z >= np.sort(z[keep])[::-1][top_k - 1])
    if top_p >= 1.0:
        return keep, keep, False
    vals = np.unique(z[keep])[::-1]                                   # distinct kept values, descending
    m = vals[0]
    order = np.argsort(-np.where(keep, z, -np.inf), kind='stable')[:int(keep.sum())]
    cum_all = np.cumsum(np.exp(z[order] - m))
    total = cum_all[-1]
    last = np.searchsorted(-z[order], -vals, side='right') - 1        # last position of each distinct value
    cum = cum_all[last] / total                                       # mass{z >= vals[i]} / mass(kept by top-k)
    i = int(np.argmax(cum >= top_p))                                  # cum[-1] == 1 >= top_p
    ambiguous = bool((np.abs(cum - top_p) <= AMBIGUOUS).any())
    small = keep & (z >= vals[i])
    larger = small
    if ambiguous and abs(cum[i] - top_p) <= AMBIGUOUS and i + 1 < len(vals):
        larger = keep & (z >= vals[i + 1])
    return small, larger, ambiguous


def kept_sets(z, top_k, top_p):
    """rows of banned z -> (kept (rows, V) bool, larger (rows, V) bool, ambiguous (rows,) bool)"""
    out = [kept_row(row, top_k, top_p) for row in z]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])

"""Test-only restatement of the stochastic beam step (dlsg_beam_select_gumbel) in float64 numpy: `gumbel_step` works on arrays, all
clips at once (a seed per clip is allowed, so that many searches of one small model run as one batch), and `SbsEmul` plugs it into
the kernel emulation the host tests drive host code with.  The noise is the counter hash of tests/test_scst_host.py, the bans are
`emul_beam.banned_classes`.  Per clip the step reports a gap: the smallest neighbour difference among each live row's k + 1 best
keys and the clip's k + 1 best perturbed values, so that a comparison with the float32 kernel can leave near-ties out."""
import numpy as np
import torch

from emul_beam import banned_classes
from emul_consensus import ConsensusEmul
from test_scst_host import counter_hash

INF = float('inf')


def gumbel_noise(seed, site, idx):
    """-log(-log u), u = ((h >> 8) + 1/2) 2^-24, float64; seed a scalar or an array that broadcasts against idx"""
    u = ((counter_hash(seed, site, idx) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    return -np.log(-np.log(u))


def root_values(seed, site, R, V):
    """(R,): the perturbed value of the empty prefix, Gumbel(0) noise keyed as class 0 of the row one step before step 0 (row b * k
    is the one a clip reads); seed a scalar or (R, 1)"""
    return gumbel_noise(seed, site, (np.arange(R, dtype=np.uint64) * np.uint64(V))[:, None])[:, 0]


def log1mexp(a):
    """log(1 - exp(a)) for a <= 0: log(-expm1(a)) above -ln 2, log1p(-exp(a)) below"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(a > -np.log(2.0), np.log(-np.expm1(a)), np.log1p(-np.exp(a)))


def conditioned(T, g, Z):
    """the children's perturbed values given that their maximum is T; g -inf stays -inf, the child with g == Z gets T exactly"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        v = T - g + log1mexp(g - Z)
        out = T - np.maximum(0.0, v) - np.log1p(np.exp(-np.abs(v)))
    return np.where(g > -INF, out, -INF)


def neighbour_gaps(a):
    """(rows,): the smallest difference of two neighbours of each descending row of a, -inf entries left out (inf: fewer than two)"""
    with np.errstate(invalid='ignore'):
        d = a[:, :-1] - a[:, 1:]
    d = np.where(np.isfinite(d), d, INF)
    return d.min(1) if d.shape[1] else np.full(a.shape[0], INF)


def gumbel_step(logits, last, last_lp, hist_in, k, end, t, G_in, temperature, seed, site, g=0, min_len=0):
    """One step on numpy arrays.  logits (R, V) float32, last (R,), last_lp (R,) and G_in (R,) float64, hist_in (R, >= t); seed an
    int or a (B,) uint64 array, one per clip.  Returns a dict: pred, back, rows (R,) int64, new_lp, G (R,) float64, gap (B,), and
    clip_gap (B,), the part of the gap that comes from the clip's k + 1 best perturbed values alone."""
    logits = np.asarray(logits, dtype=np.float32)
    R, V = logits.shape
    B = R // k
    first = t == 0
    z = (logits * np.float32(np.float32(1.0) / np.float32(temperature))).astype(np.float64)
    live = np.ones(R, dtype=bool) if first else np.asarray(last) != end
    dead = ~(z > -INF)
    if g > 0 or t < min_len:
        for r in np.nonzero(live)[0]:
            for c in banned_classes([int(x) for x in hist_in[r, :t]], t, g, min_len, end):
                dead[r, c] = True
    sd = np.repeat(np.asarray(seed, dtype=np.uint64).reshape(-1), k)[:, None] if np.ndim(seed) else seed
    phi = np.zeros(R) if first else np.asarray(last_lp, dtype=np.float64)
    T = root_values(sd, site, R, V) if first else np.asarray(G_in, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        zl = np.where(dead, -INF, z)
        mx = zl.max(1, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0.0)
        lse = np.log(np.exp(zl - mx).sum(1)) + mx[:, 0]
    idx = ((np.uint64(t + 1) * np.uint64(R) + np.arange(R, dtype=np.uint64))[:, None] * np.uint64(V)
           + np.arange(V, dtype=np.uint64)[None, :])
    noise = gumbel_noise(sd, site, idx)
    key = np.where(dead, -INF, z + noise)
    order = np.argsort(-key, axis=1, kind='stable')[:, :min(k + 1, V)]               # ties to the lower class
    top = np.take_along_axis(key, order, 1)
    row_gap = np.where(live, neighbour_gaps(top), INF)
    cls = order[:, :k]
    alive = top[:, :k] > -INF
    with np.errstate(invalid='ignore'):
        lp = np.where(alive, phi[:, None] + (np.take_along_axis(z, cls, 1) - lse[:, None]), -INF)
        gj = np.where(alive, lp + np.take_along_axis(noise, cls, 1), -INF)
    Gc = conditioned(T[:, None], gj, gj.max(1, keepdims=True))
    # a beam that has ended: <end> with its phi and its T, the other slots -inf with classes that are distinct and not <end>
    if not live.all():
        slot = np.arange(k)
        ended_cls = np.where(slot == 0, end, np.where(slot - 1 < end, slot - 1, slot))
        e = ~live
        cls = np.where(e[:, None], ended_cls[None, :], cls)
        lp = np.where(e[:, None], np.where(slot == 0, phi[:, None], -INF), lp)
        Gc = np.where(e[:, None], np.where(slot == 0, T[:, None], -INF), Gc)
    nb = 1 if first else k
    cG = Gc.reshape(B, k, k)[:, :nb].reshape(B, nb * k)
    c_lp = lp.reshape(B, k, k)[:, :nb].reshape(B, nb * k)
    c_cls = cls.reshape(B, k, k)[:, :nb].reshape(B, nb * k)
    pick = np.argsort(-cG, axis=1, kind='stable')[:, :min(k + 1, nb * k)]            # ties to the lower candidate (row, then rank)
    bestG = np.take_along_axis(cG, pick, 1)
    clip_gap = neighbour_gaps(bestG)
    gap = np.minimum(row_gap.reshape(B, k)[:, :nb].min(1), clip_gap)
    pick = pick[:, :k]
    G = bestG[:, :k]
    back = pick // k
    return dict(pred=np.take_along_axis(c_cls, pick, 1).reshape(R).astype(np.int64),
                new_lp=np.where(G > -INF, np.take_along_axis(c_lp, pick, 1), -INF).reshape(R), G=G.reshape(R),
                back=back.reshape(R).astype(np.int64), rows=(np.arange(B)[:, None] * k + back).reshape(R).astype(np.int64), gap=gap,
                clip_gap=clip_gap)


class SbsEmul(ConsensusEmul):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gap = None                                        # of the last beam_select_gumbel call: (B,) float64

    def beam_select_gumbel(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, G_in, G_out,
                           temperature=1.0, seed=0, site_sample=0, no_repeat_ngram=0, min_len=0, ended_count=None):
        assert temperature > 0 and G_in.dtype == G_out.dtype == torch.float64 and G_in.data_ptr() != G_out.data_ptr()
        if torch.is_tensor(seed):
            seed = int(seed.item())
        out = gumbel_step(logits.numpy(), last.numpy(), last_lp.numpy(), hist_in.numpy(), k, end, t, G_in.numpy(), temperature, seed,
                          site_sample, no_repeat_ngram, min_len)
        pred.copy_(torch.from_numpy(out['pred'])); back.copy_(torch.from_numpy(out['back'])); rows.copy_(torch.from_numpy(out['rows']))
        new_lp.copy_(torch.from_numpy(out['new_lp']).float()); G_out.copy_(torch.from_numpy(out['G']))
        self.gap = torch.from_numpy(out['gap'])
        h = hist_in[rows].clone() if t else torch.empty_like(hist_out)
        h[:, t] = pred
        h[:, t + 1:] = end
        hist_out.copy_(h)
        if ended_count is not None:
            ended_count += int((pred == end).sum())

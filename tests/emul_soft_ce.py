"""Test-only restatement of dlsg_ce_ragged_soft in float64 (`soft_ce_reference`, on whatever device its inputs live) and the
emulated op on top of it (`SoftCeEmul`): ClipEmul's launch log, SeqEmul's seq_per_clip kernels and `ce_ragged_soft`."""
import torch

from emul_ensemble import combined_logp
from test_grad_clip_host import ClipEmul
from test_seq_per_clip_host import SeqEmul


def teacher_rows(teacher_rows_2d, weights, mode):
    """q (R, V) float64 from the members' (R, V) logits: mode 0 the weighted mean probability, mode 1 the weighted geometric
    mean, renormalised"""
    c = combined_logp(teacher_rows_2d, weights, mode)
    return c.exp() if mode == 0 else torch.softmax(c, 1)


def soft_ce_reference(logits, targets, lens, time_major, smoothing=0.0, weights=None, teachers=(), teacher_weights=None, mode=0,
                      alpha=0.0):
    """-> (dlogits in the layout of `logits`, rows (3, B, L), sums (3,)), float64: the mixed loss, the NLL of the targets and the
    CrossEntropy against the teachers' row q, each times weights[b] / ntot; a counted row whose target is outside [0, V) is NaN"""
    lg = (logits.transpose(0, 1) if time_major else logits).double()          # (B, L, V)
    B, L, V = lg.shape
    dev = lg.device
    lens_c = lens.clamp(max=L)
    valid = torch.arange(L, device=dev).unsqueeze(0) < lens_c.unsqueeze(1)      # (B, L)
    ntot = float(lens_c.sum())
    bad = ((targets < 0) | (targets >= V)) & valid
    tg = targets.clamp(0, V - 1)
    lsm = torch.log_softmax(lg, -1)
    r = (1.0 - smoothing) * torch.nn.functional.one_hot(tg, V).double() + smoothing / V
    q = torch.zeros_like(lg)
    if len(teachers):
        rows = [(x.transpose(0, 1) if time_major else x).reshape(B * L, V) for x in teachers]
        w = [1.0] * len(rows) if teacher_weights is None else teacher_weights
        q = teacher_rows(rows, w, mode).view(B, L, V)
        r = (1.0 - alpha) * r + alpha * q
    scale = valid.double() / ntot
    if weights is not None:
        scale = scale * weights.double().view(B, 1)
    scale = torch.where(bad, torch.full_like(scale, float('nan')), scale)
    d = (lsm.exp() - r) * scale.unsqueeze(2)
    rows3 = torch.stack([-(r * lsm).sum(-1), -lsm.gather(2, tg.unsqueeze(2)).squeeze(2), -(q * lsm).sum(-1)]) * scale
    return (d.transpose(0, 1) if time_major else d), rows3, rows3.sum((1, 2))


class SoftCeEmul(ClipEmul, SeqEmul):
    """`last_soft` keeps the outputs of the last ce_ragged_soft launch: (dlogits, loss)"""

    last_soft = None

    def ce_ragged_soft(self, logits, targets, lens, dlogits, row_loss, loss, time_major, smoothing=0.0, weights=None, teachers=(),
                       teacher_weights=None, mode=0, alpha=0.0):
        assert 0.0 <= smoothing < 1.0 and 0.0 <= alpha <= 1.0 and (alpha > 0.0) == (len(teachers) > 0) and mode in (0, 1)
        assert loss.numel() == 3 and row_loss.numel() >= 3 * lens.numel() * targets.shape[1]
        d, rows3, sums = soft_ce_reference(logits, targets, lens, time_major, smoothing, weights, teachers, teacher_weights, mode, alpha)
        dlogits.copy_(d)
        n = rows3[0].numel()
        for k in range(3):
            row_loss[k * n:(k + 1) * n].copy_((rows3[k].t() if time_major else rows3[k]).reshape(-1))
        loss.copy_(sums)
        self.last_soft = (dlogits, loss)

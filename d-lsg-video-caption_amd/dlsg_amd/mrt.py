"""Minimum-risk training (MRT; Shen et al. 2016, the sequence-level risk of Edunov et al. 2018): fine-tuning on the expected
reward over a candidate list per clip.

One step: decode n candidate captions per clip in eval mode -- an ordered sample without replacement
(`sample_without_replacement`, captured as `StochasticBeamGraph`), an n-best list of a beam search (`beam_search`, captured as
`NBestBeamGraph`; groups, exclusions and prefixes included) or whatever a callable returns --, score them with the reward (on the
host with `scoring.CiderD`, on the GPU with `scoring.DeviceCiderD`), and take the Trainer's fused step teacher-forced on the
candidates with the minimum-risk loss in the CrossEntropy's place (`Trainer.step(risk=...)`):
    Q_bi = exp(alpha s_bi / len_bi^length_penalty) / sum_j exp(alpha s_bj / len_bj^length_penalty),   loss = -mean_b sum_i Q_bi r_bi
with s_bi the candidate's log-probability in the train pass.  The list is fixed when the train pass runs, so nothing here has
to be on-policy: the train pass draws its own dropout masks.
"""
import numpy as np
import torch

from .graphs import NBestBeamGraph, StochasticBeamGraph
from .model import Trainer
from .scst import SCSTTrainer


def risk_loss_reference(logits, targets, lens, rewards, n, mask=None, alpha=1.0, length_penalty=0.0, time_major=False,
                        return_parts=False):
    """The minimum-risk loss in float64 torch, differentiable in `logits`: what `Trainer.step(risk=...)` computes on the device
    (include/addons/dlsg_risk.h).  logits (rows, L, V) or, time_major, (L, rows, V); targets (rows, L) int64; lens (rows,) counting the
    <end> (clipped to L); rewards (rows,); mask (rows,) bool or None; clip b's n candidates are rows b*n .. b*n+n-1.  A candidate
    counts when its mask is set, its length is at least 1 and its log-probability is above -inf; a clip without one contributes 0.
    return_parts=True: (loss, {'Q' (B, n), 's' (B, n), 'R' (B,)}).  Targets must lie in [0, V)."""
    x = logits.double()
    if time_major:
        x = x.transpose(0, 1)
    rows, L, V = x.shape
    lens = torch.as_tensor(lens, device=x.device).long().clamp(max=L)
    lp = torch.log_softmax(x, -1).gather(2, targets.long().unsqueeze(-1)).squeeze(-1)
    live = torch.arange(L, device=x.device)[None, :] < lens[:, None]
    s = torch.where(live, lp, torch.zeros_like(lp)).sum(1)
    v = (lens >= 1) & ~torch.isneginf(s.detach())
    if mask is not None:
        v = v & torch.as_tensor(mask, device=x.device).bool()
    a = float(alpha) / lens.clamp(min=1).double() ** float(length_penalty)
    z = torch.where(v, a * torch.where(v, s, torch.zeros_like(s)), torch.full_like(s, -float('inf'))).view(-1, n)
    vb = v.view(-1, n)
    m = torch.where(vb.any(1, keepdim=True), z.detach().max(1, keepdim=True)[0], torch.zeros_like(z[:, :1]))
    e = torch.where(vb, torch.exp(torch.where(vb, z - m, torch.zeros_like(z))), torch.zeros_like(z))
    Z = e.sum(1, keepdim=True)
    Q = e / torch.where(Z > 0, Z, torch.ones_like(Z))
    r = torch.where(vb, torch.as_tensor(rewards, device=x.device).double().view(-1, n), torch.zeros_like(Q))
    R = (Q * r).sum(1)
    loss = -R.mean()
    return (loss, {'Q': Q, 's': s.view(-1, n), 'R': R}) if return_parts else loss


class MRTTrainer(object):
    """reward: as in `SCSTTrainer` -- an object with `scores(vids, hyps) -> np.ndarray`, or one that also has `index(vids)` and
    `scores_device(ids, clip_idx, end_id)`: the reward is then computed on the GPU and nothing is read back.
    n_candidates: captions per clip (1..32; the two searches give at most 8).
    candidates: 'swor' -- `model.sample_without_replacement(frames, regions, n, temperature, seed, **candidate_options)`, n
      distinct captions, counted where their log-probability is finite; 'beam' -- `model.beam_search(frames, regions, n_best=n,
      **candidate_options)` (beam_size, length_penalty, num_groups, diversity_penalty, exclude, prefix, ...), counted where their
      score is finite; or a callable (model, frames, regions, seed) -> (ids (B, n, L) int64, lens (B, n) int64, valid (B, n) bool or
      None).  Both searches decode in eval mode; with the Trainer's use_graphs they are captured graphs.  'sample' is refused: a
      caption drawn twice would be counted twice in the renormalised distribution.
    alpha: the sharpness of the renormalised distribution (0: uniform, no gradient); length_penalty: its exponent divides each
      caption's log-probability by len^length_penalty (1.0: the mean word log-probability).
    share_encoder=True (CapGnnModel): the train pass runs the encoder once per clip (`Trainer.step(seq_per_clip=n)`) instead of on
      the clips repeated n times.
    The remaining keywords go to the owned `Trainer` (lr, use_graphs, clipping, weight decay, averaged weights, data parallel)."""

    def __init__(self, model, reward, n_candidates=5, candidates='swor', candidate_options=None, alpha=1.0, length_penalty=1.0,
                 temperature=1.0, share_encoder=False, **trainer_kwargs):
        if hasattr(model, 'members'):
            raise ValueError('an Ensemble in MRTTrainer: an ensemble decodes in eval mode and trains none of its members; the risk '
                             'loss needs one model whose train pass scores the candidates')
        if trainer_kwargs.get('label_smoothing') or trainer_kwargs.get('teacher') is not None or trainer_kwargs.get('distill_weight'):
            raise ValueError('label_smoothing / teacher / distill_weight are options of the CrossEntropy step (Trainer): the '
                             'minimum-risk loss has no target row to smooth or to mix with a teacher\'s')
        if candidates == 'sample':
            raise ValueError("candidates='sample' is not covered in MRTTrainer: a caption drawn twice would be counted twice in the "
                             "renormalised distribution; 'swor' draws distinct captions")
        if not (candidates in ('swor', 'beam') or callable(candidates)):
            raise ValueError("candidates must be 'swor', 'beam' or a callable (model, frames, regions, seed) -> (ids, lens, valid), "
                             'not %r' % (candidates,))
        if not 1 <= int(n_candidates) <= Trainer.RISK_MAX_N or int(n_candidates) != n_candidates:
            raise ValueError('n_candidates must be in 1..%d, not %r' % (Trainer.RISK_MAX_N, n_candidates))
        if not (float(alpha) >= 0.0 and np.isfinite(float(alpha)) and np.isfinite(float(length_penalty))):
            raise ValueError('alpha must be finite and >= 0 and length_penalty finite, not %r, %r' % (alpha, length_penalty))
        self.candidate_options = dict(candidate_options or {})
        if self.candidate_options and callable(candidates):
            raise ValueError('candidate_options belong to the two searches; a callable takes its own')
        taken = {'swor': ('n', 'temperature', 'seed', 'return_threshold'), 'beam': ('n_best',)}.get(candidates, ())
        clash = sorted(set(self.candidate_options) & set(taken))
        if clash:
            raise ValueError('candidate_options: %s are set by MRTTrainer itself' % clash)
        self.model, self.reward = model, reward
        self.n, self.candidates = int(n_candidates), candidates
        self.alpha, self.length_penalty, self.temperature = float(alpha), float(length_penalty), float(temperature)
        self.share_encoder = bool(share_encoder)
        self.trainer = Trainer(model, **trainer_kwargs)
        self._decoder = None

    _expanded_inputs = SCSTTrainer._expanded_inputs
    _with_grad_norm = SCSTTrainer._with_grad_norm

    def _candidates(self, frames, regions, seed):
        """(ids (B*n, L) int64, lens (B*n,) int64, mask (B*n,) bool or None) of this step's lists"""
        model, n = self.model, self.n
        if callable(self.candidates):
            ids, lens, valid = self.candidates(model, frames, regions, seed)
        else:
            was_training = model.training
            # (an eager eval-mode search draws a seed it has no use for and a replayed one does not: the counter is put back, so
            #  that both forms leave the train passes the same seeds)
            drawn = model.seed_counter
            model.eval()
            try:
                swor = self.candidates == 'swor'
                if self.trainer.use_graphs:
                    model.flatten_parameters_()
                    if self._decoder is None or not self._decoder.valid_for(frames, regions):
                        self._decoder = StochasticBeamGraph(model, frames, regions, n, self.temperature, **self.candidate_options) \
                            if swor else NBestBeamGraph(model, frames, regions, n_best=n, **self.candidate_options)
                    ids, score, lens = self._decoder(frames, regions, seed) if swor else self._decoder(frames, regions)
                elif swor:
                    ids, score, lens = model.sample_without_replacement(frames, regions, n, self.temperature, seed,
                                                                        **self.candidate_options)
                else:
                    ids, score, lens = model.beam_search(frames, regions, n_best=n, **self.candidate_options)
            finally:
                model.train(was_training)
                model.seed_counter = drawn
            valid = torch.isfinite(score)
        B = frames.shape[0]
        if ids.dim() != 3 or tuple(ids.shape[:2]) != (B, n) or tuple(lens.shape) != (B, n):
            raise ValueError('candidates: ids %s and lens %s for %d clips x %d candidates' % (tuple(ids.shape), tuple(lens.shape), B, n))
        return ids.reshape(B * n, -1).contiguous(), lens.reshape(-1).contiguous(), \
            None if valid is None else valid.reshape(-1).bool().contiguous()

    @torch.no_grad()
    def step(self, frames, regions, vids):
        """One minimum-risk step on clips `vids` (B ids of the reward's corpus).  Returns {'loss', 'expected_reward' (mean_b R_b = -loss),
        'reward_mean', 'mean_len' (over the counted candidates)}, and 'grad_norm' when the Trainer clips.  Device reward: nothing is
        read back, every entry is a 0-d device tensor.  Host reward: the one host synchronisation is the copy of the candidates to
        the host, where they are scored; 'reward_mean' and 'mean_len' are then floats."""
        model, n = self.model, self.n
        B = frames.shape[0]
        assert len(vids) == B, (len(vids), B)
        ids, lens, mask = self._candidates(frames, regions, model.next_seed())
        L = ids.shape[1]
        vids_x = [v for v in vids for _ in range(n)]
        host_stats = {}
        if hasattr(self.reward, 'scores_device'):
            r = self.reward.scores_device(ids, self.reward.index(vids_x), end_id=model.decoder.vocab('<end>'))
        else:
            host = torch.cat([ids, lens.unsqueeze(1)] + ([mask.long().unsqueeze(1)] if mask is not None else []), 1).cpu()
            rh = np.asarray(self.reward.scores(vids_x, [model.decoder.decode_tokens(row) for row in host[:, :L]]), dtype=np.float64)
            keep = host[:, L + 1].bool().numpy() if mask is not None else np.ones(B * n, dtype=bool)
            keep &= host[:, L].numpy() >= 1
            r = torch.from_numpy(rh).to(ids.device, non_blocking=True)
            if keep.any():
                host_stats = {'reward_mean': float(rh[keep].mean()), 'mean_len': float(host[:, L].clamp(max=L).double().numpy()[keep].mean())}
            else:
                host_stats = {'reward_mean': 0.0, 'mean_len': 0.0}
        risk = dict(rewards=r, n=n, mask=mask, alpha=self.alpha, length_penalty=self.length_penalty)
        if self.share_encoder:
            loss = self.trainer.step(frames, regions, ids, lens, 1.0, max_len=L, seq_per_clip=n, risk=risk)
        else:
            fx, rx = self._expanded_inputs(frames, regions)
            loss = self.trainer.step(fx, rx, ids, lens, 1.0, max_len=L, risk=risk)
        st = self.trainer.last_risk['stats']
        stats = {'loss': loss, 'expected_reward': st[3].clone(), 'reward_mean': st[1].clone(), 'mean_len': st[2].clone()}
        stats.update(host_stats)
        return self._with_grad_norm(stats)

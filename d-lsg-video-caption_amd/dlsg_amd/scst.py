"""Self-critical sequence training (SCST): fine-tuning on the metric the model is judged by, after cross-entropy.

One step: draw n captions per clip in train mode (`CapGnnModel.sample`, or its captured form `SampleGraph`), score them with
CIDEr-D (on the host with `scoring.CiderD`, on the GPU with `scoring.DeviceCiderD`), subtract a baseline, and take the
policy-gradient step
    loss = -sum_b A_b sum_{t < len_b} log p(w_bt) / sum_b len_b,   A_b = reward_b - baseline_b
as the Trainer's fused step teacher-forced on the sampled words with the CrossEntropy weighted per caption by A_b
(`ce_ragged_weighted`).  The train pass uses the sampling pass's seed and rows, hence its dropout masks: the gradient is
on-policy up to the tiling of the vocabulary product.
"""
import numpy as np
import torch

from .beam import check_exclusions
from .engine import check_sample_options
from .graphs import GreedyGraph, SampleGraph, expand_rows
from .model import Trainer, _h2d


class SCSTTrainer(object):
    """reward: an object with `scores(vids, hyps) -> np.ndarray` (a `scoring.CiderD` over the training references), or one that
    also has `index(vids)` and `scores_device(ids, clip_idx, end_id)` (a `scoring.DeviceCiderD`): the reward is then computed on
    the GPU (see `step`).  `scoring.MixedReward` / `scoring.DeviceMixedReward` are the two forms of a weighted sum of CIDEr-D,
    BLEU-1..4 and ROUGE_L.
    baseline: 'mean' -- the leave-one-out mean of the clip's other n - 1 rewards (needs n_samples >= 2); 'greedy' -- the reward
    of the clip's eval-mode greedy caption.  The remaining keywords go to the owned `Trainer` (lr, use_graphs, data parallel,
    clipping, weight_decay / decay_filter / ema_decay, ...), whose Adam state, gradient buckets and graphs the step reuses;
    `self.trainer.averaged()` and `self.trainer.ema_state_dict()` give the averaged weights.
    share_encoder=True: the n samples and the train pass run the encoder once per clip -- `sample(..., share_encoder=True)`,
    then `Trainer.step(frames, regions, ids, lens, ..., seq_per_clip=n)` on the B clips and their B*n sampled captions -- instead
    of on the clips repeated n times.  The encoder's dropout masks are then shared by a clip's n samples (keyed by the clip
    row), in the sampling pass and in the train pass alike, so the step stays on-policy; the masks differ from those of the
    unshared step, which is why it is opt-in.
    sample_options: a dict of `CapGnnModel.sample`'s sampling controls (top_k, top_p, min_len, no_repeat_ngram), forwarded to
    `sample` / `SampleGraph`: the captions are then drawn from the truncated policy (the `train_sample_method = top<k> / top<p>`
    recipe of the usual captioning toolkits).  The train pass is unchanged: it differentiates the FULL-softmax log-probabilities
    of the words drawn from the truncated policy -- the usual, biased, estimator.  Without the keyword the step is the plain one.
    sample_options may also hold exclude=X, an `Exclusions` (`beam.pack_exclusions`) without a per-clip part (a captured step has no
    per-batch table input): the captions are drawn under it -- no `<unk>`, no bad ending, none of the words and phrases listed --
    and with baseline='greedy' the baseline is the eval-mode greedy caption under the same exclusions (`sample(n=1,
    temperature=0, exclude=X)` with dropout off, captured as a `SampleGraph` when the Trainer uses graphs): the caption
    `evaluate(decode=dict(exclude=X))` scores at beam size 1.  The train pass is unchanged here too.  `sample`'s prefix= is
    refused: the train pass would differentiate words the policy did not choose."""

    def __init__(self, model, reward, n_samples=5, baseline='mean', temperature=1.0, share_encoder=False, sample_options=None,
                 **trainer_kwargs):
        if hasattr(model, 'members'):
            raise ValueError('an Ensemble in SCSTTrainer: an ensemble samples in eval mode and trains none of its members; the policy '
                             'gradient needs one model whose train pass reproduces the draw')
        if baseline not in ('mean', 'greedy'):
            raise ValueError("baseline must be 'mean' or 'greedy', not %r" % (baseline,))
        if baseline == 'mean' and n_samples < 2:
            raise ValueError("the 'mean' baseline needs n_samples >= 2 (leave-one-out over the clip's samples)")
        self.model, self.reward = model, reward
        self.n, self.baseline, self.temperature = int(n_samples), baseline, float(temperature)
        self.share_encoder = bool(share_encoder)
        self.sample_options = dict(sample_options or {})
        if 'prefix' in self.sample_options:
            raise ValueError('sample_options: prefix is not covered in SCSTTrainer (the train pass would differentiate words the '
                             'policy did not choose)')
        # the keys the model's ops can run: `exclude` needs the sampled step under exclusions
        # (an ops object written before that step existed does not take the key; the ops are looked at only when it is given)
        can_exclude = 'exclude' not in self.sample_options or hasattr(model.ops, 'sample_excl_embed')
        known = ['top_k', 'top_p', 'min_len', 'no_repeat_ngram'] + ['exclude'] * can_exclude
        unknown = sorted(set(self.sample_options) - set(known))
        if unknown:
            raise ValueError('sample_options: unknown keys %s (%s)' % (unknown, ', '.join(known)))
        self.exclude = self.sample_options.get('exclude')
        check_sample_options(model.decoder.max_words, vocab_size=model.decoder.vocab_size,
                             **{k: v for k, v in self.sample_options.items() if k != 'exclude'})
        if self.exclude is not None:
            pair = self.exclude if isinstance(self.exclude, tuple) and len(self.exclude) == 2 else (None, None)
            if pair[1] is not None:
                raise ValueError('sample_options: exclude with a per-clip part is not covered in SCSTTrainer (a captured step has no '
                                 'per-batch table input): pass an Exclusions without one')
            # (anything but an Exclusions, or a shared table the steps cannot take: ValueError here, not at the first step)
            if check_exclusions(self.exclude, 0, pair[0].device if torch.is_tensor(pair[0]) else None)[0] is None:
                self.exclude = None                                 # nothing to exclude: the plain step, the plain greedy baseline
        if trainer_kwargs.get('label_smoothing') or trainer_kwargs.get('teacher') is not None or trainer_kwargs.get('distill_weight'):
            raise ValueError('label_smoothing / teacher / distill_weight are options of the CrossEntropy step (Trainer): the '
                             'policy gradient against a smoothed or a teacher\'s target row is not one')
        self.trainer = Trainer(model, **trainer_kwargs)
        self._sampler = self._greedy = None

    def _graph_ok(self, g, frames, regions):
        return g is not None and g.valid_for(frames, regions)

    def _sample(self, frames, regions, seed):
        model = self.model
        if not self.trainer.use_graphs:
            return model.sample(frames, regions, self.n, self.temperature, seed, self.share_encoder, **self.sample_options)
        model.flatten_parameters_()
        if not self._graph_ok(self._sampler, frames, regions):
            self._sampler = SampleGraph(model, frames, regions, self.n, self.temperature, self.share_encoder, **self.sample_options)
        return self._sampler(frames, regions, seed)

    def _greedy_ids(self, frames, regions):
        """eval-mode greedy captions of the B clips (no dropout, so the seed is immaterial)"""
        model = self.model
        model.flatten_parameters_()
        if self.exclude is not None:
            return self._greedy_excluding(frames, regions)
        if self.trainer.use_graphs:
            if not self._graph_ok(self._greedy, frames, regions):
                self._greedy = GreedyGraph(model, frames, regions)
            return self._greedy(frames, regions)
        return model._greedy_ids(frames, regions, 0)[0]

    def _greedy_excluding(self, frames, regions):
        """the greedy captions under the exclusions: the sampled step at temperature 0, one row per clip, in eval mode"""
        model = self.model
        was_training = model.training
        model.eval()
        try:
            if not self.trainer.use_graphs:
                return model.sample(frames, regions, 1, 0.0, 0, exclude=self.exclude)[0]
            if not self._graph_ok(self._greedy, frames, regions):
                self._greedy = SampleGraph(model, frames, regions, 1, 0.0, exclude=self.exclude)
            return self._greedy(frames, regions, 0)[0]
        finally:
            model.train(was_training)

    def _expanded_inputs(self, frames, regions):
        """the batch repeated n times, written straight into the Trainer's static graph inputs when they have that shape"""
        n = self.n
        st = self.trainer.static_inputs()
        B = frames.shape[0]
        if st is not None and st[0].shape == (B * n,) + tuple(frames.shape[1:]) and st[1].shape == (B * n,) + tuple(regions.shape[1:]):
            fx, rx = st[0], st[1]
            fx.view(B, n, *frames.shape[1:]).copy_(frames.unsqueeze(1).expand(B, n, *frames.shape[1:]))
            rx.view(B, n, *regions.shape[1:]).copy_(regions.unsqueeze(1).expand(B, n, *regions.shape[1:]))
            return fx, rx
        return expand_rows(frames, n), expand_rows(regions, n)

    @torch.no_grad()
    def step(self, frames, regions, vids):
        """One SCST step on clips `vids` (B ids of the reward's corpus).  Returns {'loss' (device scalar), 'reward_mean',
        'baseline_mean', 'mean_len'}, and 'grad_norm' (0-d device tensor) when the Trainer clips (`max_grad_norm=` / `clip_grad_value=`).
        Host reward (an object with `scores` only, e.g. `scoring.CiderD`): the one host synchronisation is the copy of the sampled
        words to the host, where the reward, the baseline and the advantages are computed; the three statistics are floats.
        Device reward (an object with `scores_device`, e.g. `scoring.DeviceCiderD`): the sampled rows -- and for the greedy
        baseline the greedy rows -- are scored on the GPU (`dlsg_cider_d`), the baseline and advantages come from
        `dlsg_scst_advantage` and go to the Trainer's step as they are: the step makes no device-to-host transfer of its own, and
        'reward_mean', 'baseline_mean' and 'mean_len' are 0-d float64 device tensors, like 'loss'."""
        model = self.model
        dec = model.decoder
        n, B = self.n, frames.shape[0]
        assert len(vids) == B, (len(vids), B)
        seed = model.next_seed()
        ids, _, lens = self._sample(frames, regions, seed)
        greedy = self._greedy_ids(frames, regions) if self.baseline == 'greedy' else None
        if hasattr(self.reward, 'scores_device'):
            return self._device_reward_step(frames, regions, vids, seed, ids, lens, greedy)
        host = torch.cat([ids, lens.unsqueeze(1)] + ([expand_rows(greedy, n)] if greedy is not None else []), 1).cpu()
        L = ids.shape[1]
        vids_x = [v for v in vids for _ in range(n)]
        r = np.asarray(self.reward.scores(vids_x, [dec.decode_tokens(row) for row in host[:, :L]]), dtype=np.float64)
        if greedy is not None:
            g = np.asarray(self.reward.scores(list(vids), [dec.decode_tokens(row) for row in host[::n, L + 1:]]), dtype=np.float64)
            b = np.repeat(g, n)
        else:
            R = r.reshape(B, n)
            b = ((R.sum(1, keepdims=True) - R) / (n - 1)).reshape(-1)
        adv = (r - b).astype(np.float32)
        loss = self._train_step(frames, regions, ids, lens, L, seed, _h2d(adv, torch.float32, ids.device))
        return self._with_grad_norm({'loss': loss, 'reward_mean': float(r.mean()), 'baseline_mean': float(b.mean()),
                                     'mean_len': float(host[:, L].double().mean())})

    def _train_step(self, frames, regions, ids, lens, L, seed, adv):
        """the policy-gradient step on the sampled words: on the clips repeated n times, or (share_encoder) on the B clips with
        their B*n captions"""
        if self.share_encoder:
            return self.trainer.step(frames, regions, ids, lens, 1.0, max_len=L, seed=seed, seq_weights=adv, seq_per_clip=self.n)
        fx, rx = self._expanded_inputs(frames, regions)
        return self.trainer.step(fx, rx, ids, lens, 1.0, max_len=L, seed=seed, seq_weights=adv)

    def _with_grad_norm(self, stats):
        """with gradient clipping on (Trainer's max_grad_norm / clip_grad_value): 'grad_norm', a 0-d device tensor, joins the stats"""
        norm = self.trainer.last_grad_norm
        if norm is not None:
            stats['grad_norm'] = norm.clone()
        return stats

    def _device_reward_step(self, frames, regions, vids, seed, ids, lens, greedy):
        model, reward = self.model, self.reward
        n, B = self.n, len(vids)
        L = ids.shape[1]
        end = model.decoder.vocab('<end>')
        # the clip indices of the B*n sampled rows, then of the B greedy rows: one asynchronous copy
        cidx = reward.index([v for v in vids for _ in range(n)] + (list(vids) if greedy is not None else []))
        r = reward.scores_device(ids, cidx[:B * n], end_id=end)
        g = reward.scores_device(greedy.contiguous(), cidx[B * n:], end_id=end) if greedy is not None else None
        adv = torch.empty(B * n, dtype=torch.float32, device=ids.device)
        stats = torch.empty(3, dtype=torch.float64, device=ids.device)
        model.ops.scst_advantage(r, lens, g, n, adv, stats)
        loss = self._train_step(frames, regions, ids, lens, L, seed, adv)
        return self._with_grad_norm({'loss': loss, 'reward_mean': stats[0], 'baseline_mean': stats[1], 'mean_len': stats[2]})

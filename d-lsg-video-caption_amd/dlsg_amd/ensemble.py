"""Ensemble decoding: several trained models -- seeds of one configuration, CapGnnModel beside a baseline, the checkpoints a GAN run
and an SCST run leave behind -- decode one caption per clip in ONE beam search.  Every member runs its own encoder and decode
step; `dlsg_beam_select_ens` combines their logit rows on the device at every word (`beam.ensemble_nbest`), so the search has the
launches of the members' searches plus nothing that touches the host.  An ensemble decodes, it samples -- `sample` draws captions
from the members' combined distribution, one `dlsg_sample_ens` launch per word (`beam.ensemble_sample`) -- and it teaches:
`teacher_logits` gives a `Trainer(teacher=...)` the members' teacher-forced rows, which `dlsg_ce_ragged_soft` combines by the same rule into the
word distribution a student is distilled towards; its own members it does not train."""
import torch

from .graphs import expand_rows
from .hip import ENS_MAX, normalised_weights

MODES = {'prob': 0, 'logprob': 1}


class Ensemble(object):
    """`Ensemble([m1, m2, m3], weights=None, mode='prob')`: up to 8 generator models with one vocabulary, one max_words and one
    device.  mode 'prob': the log of the weighted mean of the members' word probabilities (fairseq, self-critical.pytorch);
    'logprob': the weighted mean of their log-probabilities, not renormalised (OpenNMT).  weights: positive, default uniform;
    `.weights` holds them normalised to sum 1.  `.decoder` and `.ops` are the first member's, which is what
    `scoring.gather_results` / `scoring.evaluate` need to caption a loader with an ensemble."""

    def __init__(self, members, weights=None, mode='prob'):
        members = list(members)
        if not 1 <= len(members) <= ENS_MAX:
            raise ValueError('an ensemble takes 1 to %d members, not %d' % (ENS_MAX, len(members)))
        if mode not in MODES:
            raise ValueError("mode %r: 'prob' or 'logprob'" % (mode,))
        weights = [1.0] * len(members) if weights is None else list(weights)
        if len(weights) != len(members):
            raise ValueError('%d weights for %d members' % (len(weights), len(members)))
        first = members[0].decoder
        for i, m in enumerate(members[1:], 1):
            v0, v = first.vocab, m.decoder.vocab
            if len(v0) != len(v) or v0.word2idx != v.word2idx or v0.idx2word != v.idx2word:
                raise ValueError('member %d: its vocabulary differs from the first member\'s' % i)
            if m.decoder.max_words != first.max_words:
                raise ValueError('member %d: max_words %d, the first member has %d' % (i, m.decoder.max_words, first.max_words))
            if _device(m) != _device(members[0]):
                raise ValueError('member %d is on %s, the first member on %s' % (i, _device(m), _device(members[0])))
        self.members, self.weights, self.mode = members, normalised_weights(weights), mode

    @property
    def decoder(self):
        return self.members[0].decoder

    @property
    def ops(self):
        return self.members[0].ops

    def beam_search(self, visual_feats, region_feats, beam_size=None, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0,
                    num_groups=1, diversity_penalty=0.0, exclude=None, prefix=None):
        """`model.beam_search` of the ensemble: (ids (B, n, L), scores (B, n), lens (B, n)), device tensors, nothing read back.
        beam_size None: the first member's; no member's decoder.beam_size is changed.  num_groups, diversity_penalty: diverse
        beam search on the combined values, as in `model.beam_search`; exclude: exclusions, as there; prefix: a forced beginning,
        as there, a forced word's value being the members' combined one."""
        from .beam import ensemble_nbest
        return ensemble_nbest(self.members, self.weights, MODES[self.mode], visual_feats, region_feats, n_best=n_best,
                              length_penalty=length_penalty, no_repeat_ngram=no_repeat_ngram, min_len=min_len, beam_size=beam_size,
                              num_groups=num_groups, diversity_penalty=diversity_penalty, exclude=exclude, prefix=prefix)

    def greedy(self, visual_feats, region_feats):
        """(B, L) ids, <end>-padded: the search with one beam"""
        return self.beam_search(visual_feats, region_feats, beam_size=1, n_best=1)[0][:, 0]

    def sample(self, visual_feats, region_feats, n=1, temperature=1.0, seed=None, top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0,
               exclude=None, return_kept=False, **refused):
        """n captions per clip drawn from the ensemble's own distribution: (ids (B*n, L), logp (B*n, L), lens (B*n,)[, kept]) with
        the shapes and meanings of `CapGnnModel.sample`, clip b owning rows b*n .. b*n + n - 1.  At every word the members' rows are
        combined as the beam search combines them and the word is drawn with probability proportional to exp(c / temperature) over
        the words the controls keep (`beam.ensemble_sample`): the temperature tempers the ENSEMBLE's distribution; temperature 0 is
        `greedy` up to lens.  Every member runs in eval mode, whatever its `.training` says, and encodes each clip once; the members
        may be any of the three model classes, so `Ensemble([CapBaseline1(...)]).sample(...)` is the sampler those classes lack.
        seed None draws the first member's next seed; a given seed reproduces the draw.  top_k, top_p, min_len, no_repeat_ngram,
        exclude (per_clip indexed by clip), return_kept: as in `CapGnnModel.sample`.  prefix= and share_encoder= are refused with a
        ValueError that names the combination, before any encoder runs."""
        unknown = sorted(set(refused) - {'prefix', 'share_encoder'})
        if unknown:
            raise TypeError('Ensemble.sample got unexpected keyword arguments %s' % unknown)
        from .beam import ensemble_sample
        return ensemble_sample(self.members, self.weights, MODES[self.mode], visual_feats, region_feats, n=n, temperature=temperature,
                               seed=seed, top_k=top_k, top_p=top_p, min_len=min_len, no_repeat_ngram=no_repeat_ngram, exclude=exclude,
                               return_kept=return_kept, **refused)

    @torch.no_grad()
    def teacher_logits(self, frames, regions, captions, max_words=None, seq_per_clip=1):
        """The members' logits on `captions`, teacher-forced at every position and without dropout whatever a member's `.training`
        says (the flag is not touched): a list of M time-major (L, B*n, V) float32 tensors, row (t, b) what member m predicts for
        word t of caption b after its words 0..t-1.  L = captions.shape[1], cut to max_words when that is set.  seq_per_clip = n:
        frames / regions hold B clips, captions their B*n rows; a CapGnnModel member runs its encoder once per clip, the baseline
        models get the clip rows repeated.  Nothing is read back; the launches may be captured."""
        n = int(seq_per_clip)
        if n < 1 or captions.shape[0] != n * frames.shape[0]:
            raise ValueError('%d caption rows for %d clips with seq_per_clip = %r' % (captions.shape[0], frames.shape[0], seq_per_clip))
        if max_words is not None:
            captions = captions[:, :max_words]
        captions = captions.contiguous()
        L = captions.shape[1]
        out = []
        for m in self.members:
            m.flatten_parameters_()
            sv = {}
            if n == 1 or m.seq_per_clip_ok:
                m._engine_forward(frames, regions, captions, L, [True] * L, False, 0, sv, outputs=False, seq_per_clip=n)
            else:
                m._engine_forward(expand_rows(frames, n), expand_rows(regions, n), captions, L, [True] * L, False, 0, sv, outputs=False)
            out.append(sv['dec']['LOGITS'])
        return out

    def score(self, visual_feats, region_feats, ids, **options):
        """The log-probability of GIVEN captions under the ensemble, combined per word as its beam search combines them:
        `rescore.score_captions(self, ...)` -> (scores, lens[, tok_lp][, tok_rank]).  One teacher-forced pass per member and one
        `seq_logprob` launch."""
        from .rescore import score_captions
        return score_captions(self, visual_feats, region_feats, ids, **options)

    def __call__(self, visual_feats, region_feats, captions=None):
        """inference as `model(frames, regions, None)` returns it: (ids (B, L) of the best beam at the first member's beam size,
        <end>-padded, 0, 0, 0)"""
        if captions is not None:
            raise ValueError('an ensemble decodes only: call it with captions=None and train its members one by one')
        return self.beam_search(visual_feats, region_feats, n_best=1)[0][:, 0], 0, 0, 0


def _device(model):
    return next(model.parameters()).device

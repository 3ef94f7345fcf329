"""Ensemble decoding: several trained models -- seeds of one configuration, CapGnnModel beside a baseline, the checkpoints a GAN run
and an SCST run leave behind -- decode one caption per clip in ONE beam search.  Every member runs its own encoder and decode
step; `dlsg_beam_select_ens` combines their logit rows on the device at every word (`beam.ensemble_nbest`), so the search has the
launches of the members' searches plus nothing that touches the host.  An ensemble decodes; it does not train."""
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

    def beam_search(self, visual_feats, region_feats, beam_size=None, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0):
        """`model.beam_search` of the ensemble: (ids (B, n, L), scores (B, n), lens (B, n)), device tensors, nothing read back.
        beam_size None: the first member's; no member's decoder.beam_size is changed."""
        from .beam import ensemble_nbest
        return ensemble_nbest(self.members, self.weights, MODES[self.mode], visual_feats, region_feats, n_best=n_best,
                              length_penalty=length_penalty, no_repeat_ngram=no_repeat_ngram, min_len=min_len, beam_size=beam_size)

    def greedy(self, visual_feats, region_feats):
        """(B, L) ids, <end>-padded: the search with one beam"""
        return self.beam_search(visual_feats, region_feats, beam_size=1, n_best=1)[0][:, 0]

    def __call__(self, visual_feats, region_feats, captions=None):
        """inference as `model(frames, regions, None)` returns it: (ids (B, L) of the best beam at the first member's beam size,
        <end>-padded, 0, 0, 0)"""
        if captions is not None:
            raise ValueError('an ensemble decodes only: call it with captions=None and train its members one by one')
        return self.beam_search(visual_feats, region_feats, n_best=1)[0][:, 0], 0, 0, 0


def _device(model):
    return next(model.parameters()).device

"""Consensus (minimum Bayes risk) reranking of candidate captions on the device: the reference-free use of an n-best list.  Each
candidate of a clip is scored by its expected CIDEr-D against the clip's OTHER candidates (`scoring.DeviceCiderD.consensus_device`,
one `dlsg_cider_consensus` launch on the training corpus's idf) and the list is reordered by that -- "CIDEr consensus reranking"
in the captioning literature, MBR decoding in translation toolkits.  Nothing here synchronises with the host: the reordering is
device gathers, so both functions can be captured (`graphs.ConsensusBeamGraph`)."""
import math

import torch

WEIGHTS = ('uniform', 'posterior')


def consensus_rerank(reward, ids, scores=None, lens=None, weights='uniform', temperature=1.0, n_best=None):
    """Rerank candidate lists by consensus.  reward: a `scoring.DeviceCiderD`; ids int64 (B, n, L) -- `beam_search` output as it
    stands, or `sample` output viewed as (B, n, L); scores float32 (B, n) and lens int64 (B, n) of the candidates, either may be
    None.  weights='uniform': every candidate counts the same (for samples this is the Monte Carlo estimate of the expected
    utility); score VALUES are ignored, but a candidate whose score is -inf or NaN (a beam slot the search left empty) is invalid:
    it neither votes nor can win.  weights='posterior': candidate j votes with exp((scores[j] - max) / temperature); needs scores.
    Returns (ids, expected, lens, order), each reordered by the consensus ranking and cut to the n_best (default: all) first:
    expected float64 (B, n_best) descending, order int64 the candidates' indices in the input list, lens None when none came in.
    Ties keep the input order, so a consensus that says nothing returns the search's own ranking."""
    if weights not in WEIGHTS:
        raise ValueError('consensus weights %r: one of %s' % (weights, ', '.join(WEIGHTS)))
    if weights == 'posterior' and scores is None:
        raise ValueError("consensus weights 'posterior' need the candidates' scores")
    if not temperature > 0.0:
        raise ValueError('consensus temperature %r must be positive' % (temperature,))
    if ids.dim() != 3:
        raise ValueError('consensus_rerank takes ids of shape (B, n, L), not %s' % (tuple(ids.shape),))
    n = ids.shape[1]
    keep = n if n_best is None else n_best
    if not 1 <= keep <= n:
        raise ValueError('n_best %d outside 1 .. %d candidates' % (keep, n))
    # uniform weights that still honour validity: an infinite temperature weighs every valid candidate 1
    order, expected = reward.consensus_device(ids, scores, temperature if weights == 'posterior' else math.inf)
    order = order[:, :keep]
    out = torch.gather(ids, 1, order.unsqueeze(2).expand(-1, -1, ids.shape[2]))
    return out, torch.gather(expected, 1, order), None if lens is None else torch.gather(lens, 1, order), order


@torch.no_grad()
def consensus_search(model_or_ensemble, frames, regions, reward, n_best=1, weights='uniform', temperature=1.0, stochastic=None,
                     **beam_options):
    """`beam_search` of a model (CapGnnModel, the baselines) or an `ensemble.Ensemble` with every beam kept, then
    `consensus_rerank`: (ids (B, n_best, L), expected, lens, order).  beam_options: beam_size, length_penalty, no_repeat_ngram,
    min_len, num_groups, diversity_penalty, exclude, prefix -- diverse groups give the consensus something to choose from, a prefix
    (`beam.pack_prefix`) makes the candidates n endings of one beginning.  The search's launches plus one.
    stochastic=dict(n=..., temperature=..., seed=..., min_len=..., no_repeat_ngram=...): the candidates are the n distinct
    captions of `model.sample_without_replacement` instead (a model, not an ensemble), their log-probabilities the scores: a
    without-replacement sample of the model as the candidate list of the Monte Carlo estimate, with no row spent on a duplicate.
    beam_options must then be empty, and a prefix is refused in either place."""
    if stochastic is not None:
        if stochastic.get('prefix') is not None or beam_options.get('prefix') is not None:
            raise ValueError('prefix and consensus_search(stochastic=...): a forced beginning is not covered in sampling without '
                             'replacement')
        if beam_options:
            raise ValueError('consensus_search(stochastic=...) takes no beam options (%s): the candidates come from '
                             'sample_without_replacement' % ', '.join(sorted(beam_options)))
        if 'return_threshold' in stochastic:
            raise ValueError('consensus_search(stochastic=...) reranks the captions themselves: return_threshold has no use here')
        if not hasattr(model_or_ensemble, 'sample_without_replacement'):
            raise ValueError('consensus_search(stochastic=...) takes one model: an ensemble does not sample without replacement')
        ids, scores, lens = model_or_ensemble.sample_without_replacement(frames, regions, **stochastic)
    else:
        ids, scores, lens = model_or_ensemble.beam_search(frames, regions, **beam_options)
    return consensus_rerank(reward, ids, scores, lens, weights, temperature, n_best)

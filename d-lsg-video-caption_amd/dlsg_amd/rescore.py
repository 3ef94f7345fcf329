"""Scoring GIVEN captions on the device.  Every search here reports `scores`, but only for captions it generated itself and only
under the model that generated them; `score_captions` answers "what is the log-probability of THIS caption for this clip under
THAT model" -- a model or an `ensemble.Ensemble` -- by one teacher-forced pass per member (`Ensemble.teacher_logits`: no dropout,
the encoder once per clip for its n candidates) and one `dlsg_seq_logprob` launch, which combines the members' rows as the
ensemble beam step does and reads only the rows of a caption's own words.  A model that rescores its own search's output
reproduces that search's `scores` and `lens`.  On top of it: `rescore` reorders candidate lists (search with one model, rank with
an ensemble), `rescore_search` does both in one call.  Nothing here synchronises with the host, so all of it can be captured
(`graphs.ScoreGraph`, `graphs.RescoreBeamGraph`)."""
import torch

from .ensemble import MODES, Ensemble


def as_ensemble(scorer):
    """a model as the ensemble of itself; an `Ensemble` as it is"""
    return scorer if isinstance(scorer, Ensemble) else Ensemble([scorer])


@torch.no_grad()
def score_captions(scorer, frames, regions, ids, lens=None, length_penalty=0.0, return_tokens=False, return_ranks=False):
    """The log-probability of the captions `ids` for the clips (frames, regions) under `scorer`, a model (CapGnnModel, the
    baselines) or an `Ensemble`.  ids int64 (B, L) or (B, n, L): one caption, or n candidates, per clip, <end>-padded as every
    search returns them (L at most the scorer's max_words); lens, optional, int64 shaped like ids without the last axis: the
    number of words to count instead of "up to and including the first <end>".  Returns (scores, lens[, tok_lp][, tok_rank]):
    scores float32 = log-prob / len^length_penalty and lens int64, shaped like ids without the last axis; with return_tokens the
    words' log-probabilities float32 (..., L), 0 behind the caption; with return_ranks each word's rank in its row, int32
    (..., L), 0 = the word a greedy decode would choose there, -1 behind the caption.  The members run teacher-forced and
    without dropout whatever `.training` says; one `seq_logprob` launch; nothing is read back."""
    ens = as_ensemble(scorer)
    if ids.dim() not in (2, 3) or ids.dtype != torch.int64:
        raise ValueError('score_captions takes int64 ids of shape (B, L) or (B, n, L), not %s %s' % (ids.dtype, tuple(ids.shape)))
    B, L = ids.shape[0], ids.shape[-1]
    n = ids.shape[1] if ids.dim() == 3 else 1
    dec = ens.decoder
    if not 1 <= L <= dec.max_words:
        raise ValueError('captions of %d words: the scorer has max_words %d' % (L, dec.max_words))
    from .beam import _check_max_words
    _check_max_words(L, 'caption scoring')
    if not length_penalty >= 0.0:                                      # (NaN fails the comparison)
        raise ValueError('length_penalty (%r) must not be negative or NaN' % (length_penalty,))
    shape = tuple(ids.shape[:-1])
    if lens is not None:
        if tuple(lens.shape) != shape or lens.dtype != torch.int64 or lens.device != ids.device:
            raise ValueError('lens must be int64 of shape %s on %s, not %s %s on %s' % (shape, ids.device, lens.dtype, tuple(lens.shape), lens.device))
        lens = lens.reshape(B * n).contiguous()
    rows = ids.reshape(B * n, L).contiguous()
    logits = ens.teacher_logits(frames, regions, rows, seq_per_clip=n)
    scores, lens_out, _, tok_lp, tok_rank = ens.ops.seq_logprob(logits, ens.weights, MODES[ens.mode], rows, lens, float(length_penalty),
                                                                 return_tokens, return_ranks, end=dec.vocab('<end>'))
    out = (scores.view(shape), lens_out.view(shape))
    if return_tokens:
        out += (tok_lp.view(shape + (L,)),)
    if return_ranks:
        out += (tok_rank.view(shape + (L,)),)
    return out


@torch.no_grad()
def rescore(scorer, frames, regions, ids, scores=None, lens=None, mix=1.0, length_penalty=0.0, n_best=None):
    """Reorder candidate lists by a scorer: ids int64 (B, n, L), `beam_search` output as it stands (or `sample` output viewed so),
    scores (B, n) float32 and lens (B, n) int64 of the candidates, either may be None.  Every candidate gets new =
    `score_captions(scorer, ..., lens, length_penalty)`, the list is sorted by mix * new + (1 - mix) * scores, descending, ties in
    input order, and cut to the n_best (default: all) first.  A candidate whose incoming score is -inf or NaN (a beam slot the
    search left empty) stays -inf and goes last.  mix = 1: the scorer alone decides (scores only mark the invalid candidates).
    Returns (ids, scores, lens, order): the mixed scores float32 (B, n_best), the lens that were counted, order int64 the
    candidates' indices in the input list.  Device gathers only."""
    if ids.dim() != 3:
        raise ValueError('rescore takes ids of shape (B, n, L), not %s' % (tuple(ids.shape),))
    if scores is None and mix != 1.0:
        raise ValueError('rescore with mix %r needs the candidates\' scores' % (mix,))
    if not 0.0 <= mix <= 1.0:
        raise ValueError('mix (%r) must lie in [0, 1]' % (mix,))
    B, n, L = ids.shape
    keep = n if n_best is None else n_best
    if not 1 <= keep <= n:
        raise ValueError('n_best %d outside 1 .. %d candidates' % (keep, n))
    if scores is not None and (tuple(scores.shape) != (B, n) or scores.dtype != torch.float32):
        raise ValueError('rescore scores must be float32 of shape %s, not %s %s' % ((B, n), scores.dtype, tuple(scores.shape)))
    new, counted = score_captions(scorer, frames, regions, ids, lens, length_penalty)
    mixed = new
    if scores is not None:
        if mix != 1.0:
            mixed = mix * new + (1.0 - mix) * scores
        mixed = torch.where(scores > float('-inf'), mixed, torch.full_like(mixed, float('-inf')))      # (NaN fails the comparison)
    top, order = mixed.sort(dim=1, descending=True, stable=True)
    top, order = top[:, :keep].contiguous(), order[:, :keep].contiguous()
    return torch.gather(ids, 1, order.unsqueeze(2).expand(-1, -1, L)), top, torch.gather(counted, 1, order), order


@torch.no_grad()
def rescore_search(model_or_ensemble, scorer, frames, regions, n_best=1, mix=1.0, **beam_options):
    """`beam_search` of a model or an `Ensemble` with every beam kept, then `rescore` by `scorer` with the search's
    length_penalty: (ids (B, n_best, L), scores, lens, order).  One model searches, the scorer's members each pay one
    teacher-forced pass over the kept beams (DESIGN.md section 27 has what that costs).  beam_options: beam_size, length_penalty, no_repeat_ngram, min_len, num_groups,
    diversity_penalty.  The search's launches, the scorer's forward passes and one launch."""
    ids, scores, lens = model_or_ensemble.beam_search(frames, regions, **beam_options)
    return rescore(scorer, frames, regions, ids, scores, lens, mix, beam_options.get('length_penalty', 0.0), n_best)

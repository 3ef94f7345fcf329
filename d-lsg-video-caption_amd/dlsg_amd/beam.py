"""Beam-search inference (Decoder.forward beam branch models/layer.py:449-460, Decoder.beam_step :489-567,
BeamSearch.search models/allennlp_beamsearch.py:51-294 with per_node_beam_size == beam_size, layer.py:346).

The decode step runs on the HIP kernels with all B*k beams as one batch (the reference loops over the k beams,
layer.py:521-551; rows are independent so the values are the same).  The step-invariant tensors are never re-gathered by
back-pointer: K', V' stay one block per clip that its k beams read (dlsg_dec_mid_args.kv_div), the global-feature gates
are expanded once; only the four LSTM states are reordered (one gather launch, ping-pong slots).  Candidate selection -- log-softmax, top-k over the
vocabulary per beam, top-k over the k*k continuations, back-pointers -- is one HIP launch per step (`beam_select`);
the host does not synchronise inside the loop except for the early-exit test every 4th step.

`beam_nbest` is the search beyond the reference: all k hypotheses with their scores, length normalisation, repeated-n-gram
blocking and a minimum length, with no host synchronisation at all (`beam_select_hist` carries every beam's tokens along, so
there is no back-trace; `beam_finalize` ranks the beams).  `ensemble_nbest` is that search run by several models at once: each
member steps its own state, `beam_select_ens` combines their logits and chooses the beams (`ensemble.Ensemble`).
`constrained_nbest` is `beam_nbest` whose captions must contain given words: `beam_select_cons` shares the beams out over the
banks "constraints met" (dynamic beam allocation) and recomputes what a beam has met from its token history; with phrases
(`pack_phrases`) the same loop runs on `beam_select_phrases`, whose banks are (constraints met, progress into a phrase).  Words
and phrases share their host side: one packer (`_pack`; `pack_constraints` and `pack_phrases` are its two ways of reading a
constraint's alternatives), one check of a packed tensor (`_check_packed`) and one search body, which differs by the tensor's
rank in the step it launches and in how `_constraints_met` counts.
`beam_nbest(exclude=...)` and `ensemble_nbest(exclude=...)` are those searches under exclusions -- words, phrases and endings a caption
must not contain (`pack_exclusions`): `beam_select_excl` adds the last word of every excluded entry that a beam's history leads up to
to the beam's ban list; `exclusions_hit` counts what a caption contains of them.  `stochastic_nbest(exclude=...)` draws its captions
under the same tables (`beam_select_gumbel_excl`), the model renormalised over the words that are left, as its other bans do.
`ensemble_sample` draws from an ensemble instead of searching with it: the members step as in `ensemble_nbest`, on rows that never
change parents, and one `sample_ens` launch per word combines their rows and draws from the combined distribution.
`prefix=` makes the history searches continue a given beginning (`pack_prefix`): behind the select launch of each of the first P
steps `beam_force_prefix` rewrites the clips whose prefix reaches that step -- the forced word in every slot, its value on beam 0,
-inf on the others -- and since bans and constraint state are recomputed from the history row, the prefix is seen by all of them.
"""
import collections

import torch

from . import engine as E
from .graphs import expand_rows


@torch.no_grad()
def beam_infer(model, visual_feats, region_feats):
    """Beam search as the reference runs it (early exit tested every 4th step on the host)."""
    return beam_finish(model, *beam_device(model, visual_feats, region_feats, early_exit=True))


@torch.no_grad()
def beam_device(model, visual_feats, region_feats, early_exit=True):
    """Everything of the search that runs on the device.  early_exit=False: no host synchronisation at all (all L steps
    are launched; beam_finish cuts the result to the step the reference would have stopped at) -- this form is what
    BeamGraph captures into a hipGraph.  Returns the tensors beam_finish needs."""
    mems, sv, seed, extras = _encode(model, visual_feats, region_feats)
    return beam_search_from(model, mems, sv, seed, early_exit, extras)


def _encode(model, visual_feats, region_feats):
    """the encoder of the model's class: the attended memories, the saved tensors, the seed and the proposals forward() returns"""
    model.flatten_parameters_()
    seed = model.next_seed()
    sv = {}
    props, mems = model._encoder_pass(visual_feats, region_feats, False, seed, sv)
    return mems, sv, seed, props


def _beam_setup(model, mems, sv, seed, k):
    """What the two searches share: the step-invariant decoder work on the B clips, the state of their R = B*k beams, and
    `advance(t, words, rows)` -- step t of all beams on `words`, for t > 0 after the reorder of the state by the back-pointer rows
    `rows` of step t-1 -- which returns the step's logits (R, V).  -> (advance, B, R, L)"""
    ops, dec = model.ops, model.decoder
    frames = mems[0]                                   # (reference tensor for device / dtype of the scratch arrays)
    s = E.dec_prepare(ops, dec, mems, sv, False, seed)
    B, V, L = frames.shape[0], dec.vocab_size, dec.max_words
    if k > V:
        raise ValueError('Target vocab size (%d) too small relative to per_node_beam_size (%d)' % (V, k))
    # ---- K', V' stay one block per CLIP: the k beams of a clip are consecutive rows and read their clip's block (kv_div) -- no
    # expanded (B*k)-row copies (82 MB at 128 x 5 rows).  Measured: the word step is not faster for it (20.0 ms per batch either
    # way: the fused step kernel is bound by its per-row chain, the expanded copies were Infinity-Cache resident); it saves the
    # memory and the one-time copies.  Only the small global-feature gate term is expanded to B*k rows
    s['kv_div'] = k
    s['gq'] = expand_rows(s['gq'], k)
    R = B * k
    E.dec_alloc(dec, s, frames, R, L)
    # recurrent state: two physical slots per step.  Step t reads slot 2t and writes slot 2t+1; the reorder by
    # back-pointer gathers slot 2t+1 into slot 2t+2, so nothing is gathered in place and nothing is copied back.
    state_keys = ['LHP', 'QH', 'QC', 'LC']
    big = {key: torch.zeros(2 * L + 2, R, s[key].shape[2], dtype=torch.float32, device=frames.device) for key in state_keys}
    Emb = dec.word_embed.weight

    def advance(t, words, rows):
        if t:
            # state of step t: slot 2t <- slot 2t-1, rows reordered by the parents chosen at step t-1
            ops.gather_rows_multi([big[key][2 * t - 1] for key in state_keys], rows, [big[key][2 * t] for key in state_keys])
        for key in state_keys:
            s[key] = big[key][t:]                                  # index t -> slot 2t, index t+1 -> slot 2t+1
        ops.embed_fwd(Emb, words, s['WE'][t])                      # beam_step applies no word dropout (layer.py:537)
        E.dec_step(ops, dec, s, t, frames, False, seed, R)
        E.dec_logits(ops, dec, s, t, t + 1)
        return s['LOGITS'][t]
    return advance, B, R, L


@torch.no_grad()
def beam_search_from(model, mems, sv, seed, early_exit=True, extras=None):
    """The search itself from given attended memories (`mems`: the proposals of the encoder streams, or whatever a caller of
    `Decoder.forward` hands in -- models/layer.py:449-455 builds its start state from `cnn_feats` / `cnn_feats_2` / `global_feat`
    the same way); `sv['dec_gsrc']` are the tensors whose row means form the global feature, `sv['step_feats']` replaces them
    (layer.py:404-405)."""
    ops, dec = model.ops, model.decoder
    k = dec.beam_size
    advance, B, R, L = _beam_setup(model, mems, sv, seed, k)
    end = dec.vocab('<end>')
    dev = mems[0].device
    preds = torch.empty(L, R, dtype=torch.int64, device=dev)       # chosen classes per step, (B,k) flattened
    backs = torch.zeros(L, R, dtype=torch.int64, device=dev)
    rows = torch.empty(R, dtype=torch.int64, device=dev)
    lps = torch.zeros(2, R, dtype=torch.float32, device=dev)       # running log-probs, ping-pong
    ended = torch.zeros(L, dtype=torch.int32, device=dev)          # number of <end> among the classes chosen at step t
    start = torch.full((R,), dec.vocab('<start>'), dtype=torch.int64, device=dev)
    # the reference tests `all beams ended` on the host before every step (allennlp_beamsearch.py:168); here the count of
    # <end> tokens is kept on the device and read every CHECK steps, and the result is cut to the step the reference
    # would have stopped at (steps after that only append <end> at log-prob 0 and change nothing before them)
    CHECK = 4
    logits = advance(0, start, rows)
    ops.beam_select(logits, start, lps[0], preds[0], lps[1], backs[0], rows, k, end, first=True, ended_count=ended[0:1])
    done = 1
    for t in range(1, L):
        if early_exit and t % CHECK == 0:
            cnt = ended[:t].tolist()
            if any(c == R for c in cnt):
                break
        logits = advance(t, preds[t - 1], rows)
        cur, nxt = lps[t % 2], lps[(t + 1) % 2]
        ops.beam_select(logits, preds[t - 1], cur, preds[t], nxt, backs[t], rows, k, end, ended_count=ended[t:t + 1])
        done = t + 1
    return preds, backs, lps, ended, done, B, k, R, L, extras


def beam_finish(model, preds, backs, lps, ended, done, B, k, R, L, extras):
    """Host side of the search: where the reference would have stopped (allennlp_beamsearch.py:168), the back-trace
    (:272-292) and the choice of the best beam (layer.py:456-460)."""
    cnt = ended[:done].tolist()                                   # host synchronisation
    chk = getattr(model.ops, 'check_persistent', None)
    if chk is not None:
        chk()                                                     # the encoder's persistent BiLSTM: time-out word is final here
    n_steps = done
    hit = [i for i, c in enumerate(cnt[:L - 1]) if c == R]
    if hit:
        n_steps = min(done, hit[0] + 1)
    if k == 1 and cnt[0] == R:
        n_steps = 1
    # ---- back-trace over the steps the reference would have run (allennlp_beamsearch.py:272-292)
    P = preds[:n_steps].view(n_steps, B, k)
    Bk = backs[:n_steps].view(n_steps, B, k)
    # once every beam has ended, further steps keep the log-probs and their order, so the last buffer is the reference's
    last_lp = lps[done % 2].view(B, k)
    if n_steps == 1:
        all_preds = P[0].unsqueeze(2)
    else:
        rec = [P[n_steps - 1].unsqueeze(2)]
        cur = Bk[n_steps - 1]
        for t in range(n_steps - 2, 0, -1):
            rec.append(P[t].gather(1, cur).unsqueeze(2))
            cur = Bk[t].gather(1, cur)
        rec.append(P[0].gather(1, cur).unsqueeze(2))
        all_preds = torch.cat(list(reversed(rec)), 2)
    best = last_lp.topk(1)[1].squeeze(1)                          # layer.py:456-460
    # (one gather: indexing clip by clip reads best[i] back to the host B times -- 128 synchronisations per batch)
    out = all_preds.gather(1, best.view(B, 1, 1).expand(B, 1, all_preds.shape[2])).squeeze(1)
    return model._public(out, extras, [])


MAX_BEAM, MAX_WORDS = 8, 64          # limits of dlsg_beam_select_hist / dlsg_beam_finalize


def _check_max_words(L, what):
    """ValueError for a history longer than the step kernels keep"""
    if L > MAX_WORDS:
        raise ValueError('max_words %d: %s keeps at most %d tokens per beam' % (L, what, MAX_WORDS))


def _check_bans(L, no_repeat_ngram, min_len):
    """ValueError for an n-gram ban or a minimum length no history step can apply"""
    if no_repeat_ngram < 0 or min_len < 0:
        raise ValueError('no_repeat_ngram (%d) and min_len (%d) must not be negative' % (no_repeat_ngram, min_len))
    if min_len >= L:
        raise ValueError('min_len %d leaves no room for <end> in max_words %d' % (min_len, L))


def check_nbest_options(k, L, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0, num_groups=1, diversity_penalty=0.0):
    """ValueError for what `beam_nbest` cannot run; returns n"""
    n = k if n_best is None else n_best
    if not 1 <= k <= MAX_BEAM:
        raise ValueError('beam size %d: the n-best search takes 1 to %d beams' % (k, MAX_BEAM))
    _check_max_words(L, 'the n-best search')
    if not 1 <= n <= k:
        raise ValueError('n_best %d outside 1 .. beam size %d' % (n, k))
    _check_bans(L, no_repeat_ngram, min_len)
    if not 1 <= num_groups <= k or k % num_groups:
        raise ValueError('num_groups %r: diverse beam search splits the %d beams into 1 .. %d groups of equal size' % (num_groups, k, k))
    if not diversity_penalty >= 0.0:                                   # (NaN fails the comparison)
        raise ValueError('diversity_penalty (%r) must not be negative or NaN' % (diversity_penalty,))
    if diversity_penalty > 0.0 and num_groups == 1:
        raise ValueError('diversity_penalty %r does nothing with one group: set num_groups' % (diversity_penalty,))
    return n


def _hist_search(models, k, visual_feats, region_feats, select, prefix=None, weights=None, mode=0):
    """The search every history step kernel runs in: each model encodes its clips and steps its own state on the shared words and
    back-pointer rows; at every word `select(t, logits, step)` makes the one launch that chooses the beams -- `logits` the models'
    (R, V) rows, `step` the arguments every history step takes after the logits (words, the log-prob and pred ping-pong, back, rows,
    k, <end>, the history ping-pong, t).  All L steps are launched, nothing is read back.  -> the last step's (hist (R, L), lps (R,))
    prefix (B, P) int64 (`check_prefix`): behind the select launch of each of the first P steps one `beam_force_prefix` launch
    rewrites the clips whose prefix reaches that step, with the models as members of `weights` (None: one model) in `mode`."""
    steps = []
    for model in models:
        mems, sv, seed, _ = _encode(model, visual_feats, region_feats)
        advance, B, R, L = _beam_setup(model, mems, sv, seed, k)
        steps.append(advance)
    dec, dev = models[0].decoder, mems[0].device
    end = dec.vocab('<end>')
    preds = torch.empty(2, R, dtype=torch.int64, device=dev)       # ping-pong: the history keeps the tokens
    hist = torch.empty(2, R, L, dtype=torch.int64, device=dev)     # filled by step 0
    back = torch.empty(R, dtype=torch.int64, device=dev)
    rows = torch.empty(R, dtype=torch.int64, device=dev)
    lps = torch.zeros(2, R, dtype=torch.float32, device=dev)
    words = torch.full((R,), dec.vocab('<start>'), dtype=torch.int64, device=dev)
    for t in range(L):
        logits = [advance(t, words, rows) for advance in steps]
        step = (words, lps[t % 2], preds[t % 2], lps[(t + 1) % 2], back, rows, k, end, hist[t % 2], hist[(t + 1) % 2], t)
        select(t, logits, step)
        if prefix is not None and t < prefix.shape[1]:                 # (the table's width: nothing is read back)
            models[0].ops.beam_force_prefix(logits, [1.0] if weights is None else weights, mode, *step, prefix)
        words = preds[t % 2]
    return hist[L % 2], lps[L % 2]


def _finalize(model, hist, lps, k, n, length_penalty):
    """`beam_finalize` on a search's last history: the n best of every clip's k beams -> (ids (B, n, L), scores (B, n), lens (B, n))"""
    dev, B, L = hist.device, hist.shape[0] // k, hist.shape[1]
    ids = torch.empty(B, n, L, dtype=torch.int64, device=dev)
    scores = torch.empty(B, n, dtype=torch.float32, device=dev)
    lens = torch.empty(B, n, dtype=torch.int64, device=dev)
    model.ops.beam_finalize(hist, lps, k, model.decoder.vocab('<end>'), float(length_penalty), ids, scores, lens)
    return ids, scores, lens


def _nbest_search(models, weights, mode, visual_feats, region_feats, n_best, length_penalty, no_repeat_ngram, min_len, beam_size,
                  num_groups, diversity_penalty, exclude=None, prefix=None):
    """The search of `beam_nbest` (weights None: one model) and `ensemble_nbest`: `_hist_search` on the step kernel the options
    ask for, `beam_finalize` ranks the beams."""
    dec, ops = models[0].decoder, models[0].ops
    k = dec.beam_size if beam_size is None else beam_size
    n = check_nbest_options(k, dec.max_words, n_best, length_penalty, no_repeat_ngram, min_len, num_groups, diversity_penalty)
    prefix = search_prefix(ops, prefix, visual_feats.shape[0], visual_feats.device, dec, num_groups)
    if exclude is not None:
        shared, per_clip = check_exclusions(exclude, visual_feats.shape[0], visual_feats.device, num_groups)

    def select(t, logits, step):
        if exclude is not None:                                        # (never with groups: check_exclusions)
            ops.beam_select_excl(logits, [1.0] if weights is None else weights, mode, *step, shared, per_clip, no_repeat_ngram, min_len)
        elif num_groups > 1:                                           # (a single model: one member of weight 1)
            ops.beam_select_groups(logits, [1.0] if weights is None else weights, mode, *step, no_repeat_ngram, min_len, num_groups,
                                   float(diversity_penalty))
        elif weights is None:
            ops.beam_select_hist(logits[0], *step, no_repeat_ngram, min_len)   # (reads a logit row twice, the ensemble step three times)
        else:
            ops.beam_select_ens(logits, weights, mode, *step, no_repeat_ngram, min_len)
    return _finalize(models[0], *_hist_search(models, k, visual_feats, region_feats, select, prefix, weights, mode), k, n, length_penalty)


@torch.no_grad()
def beam_nbest(model, visual_feats, region_feats, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0, beam_size=None,
               num_groups=1, diversity_penalty=0.0, exclude=None, prefix=None):
    """The n best of the k beams of every clip: (ids (B, n, L) int64, padded with <end>; scores (B, n) float32 =
    log-prob / len^length_penalty, descending; lens (B, n) int64 = tokens up to and including the first <end>, else L), device
    tensors.  no_repeat_ngram = g: no caption repeats a g-gram; min_len: no <end> before that many words.  A banned word takes
    log-prob -inf, the others are not renormalised.  All L steps are launched and nothing is read back: once every beam of a clip
    has ended a step only appends <end> at log-prob 0, so with the options off the rows are the reference's beams, end-padded.
    beam_size: the number of beams, default the decoder's.  Because nothing is read back, the persistent BiLSTM's time-out word
    is not looked at here: call `model.ops.check_persistent()` where the ids are copied to the host (`scoring.gather_results`
    does).
    num_groups = G > 1: diverse beam search (Vijayakumar et al. 2016) -- the beams are G groups of beam_size / G, chosen one
    group after another at every word; a word that earlier groups chose at that step costs a later group `diversity_penalty` per
    choice (inf: it is excluded).  The penalty steers the choice only: scores stay log-prob / len^length_penalty, and the n best
    are ranked over all groups together.  One `beam_select_groups` launch per step; num_groups = 1 launches what it always did.
    exclude: the `Exclusions` of `pack_exclusions` -- words and phrases no caption may contain, for all clips or per clip: a beam may
    not choose the last word of an entry behind the entry's other words (`<unk>` is a one-word entry, a bad ending the pair
    (word, <end>)).  One `beam_select_excl` launch per step, the model as one member of weight 1; not together with num_groups > 1.
    exclude=None launches what it always did.
    prefix: how every caption begins -- the (B, P) int64 tensor of `pack_prefix` on the clips' device (clip b's prefix: the leading run
    of ids in [0, V) of row b, any other id, normally -1, ends it; lengths may differ and may be 0), or the per-clip list `pack_prefix`
    takes, which is packed here.  At the steps t < p_b the caption's word is prefix[b, t] whatever the bans say; from p_b on the
    search goes on as it would behind these words had it chosen them: the n-gram ban and the exclusions see the prefix (an entry can
    be completed across the boundary and is banned there), min_len counts it.  The caller's own words are not checked against
    `exclude`: `exclusions_hit` can be non-zero because of the prefix alone.  The scores include the forced words' log-probs and lens
    count them, so `score(ids)` returns the search's scores and lens.  One `beam_force_prefix` launch behind the select launch of
    each of the first P steps; not together with num_groups > 1.  prefix None, or P == 0, launches what it always did."""
    return _nbest_search([model], None, 0, visual_feats, region_feats, n_best, length_penalty, no_repeat_ngram, min_len, beam_size,
                         num_groups, diversity_penalty, exclude, prefix)


@torch.no_grad()
def ensemble_nbest(models, weights, mode, visual_feats, region_feats, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0,
                   beam_size=None, num_groups=1, diversity_penalty=0.0, exclude=None, prefix=None):
    """`beam_nbest` with several models that decode one caption: every member runs its own encoder and its own decode step on the
    shared words and back-pointer rows (its own state slots; any of the model classes, any hidden sizes), and one
    `beam_select_ens` launch per step combines the members' logit rows -- mode 0: log of the weighted mean probability, mode 1:
    weighted mean log-probability -- and chooses the beams.  One set of preds / hist / back / rows / lps; no host synchronisation.
    The members share vocabulary, max_words and device (`ensemble.Ensemble` checks that); beam_size defaults to the first member's.
    num_groups, diversity_penalty: diverse beam search as in `beam_nbest`, on the combined values (`beam_select_groups`).
    exclude: exclusions as in `beam_nbest` (`beam_select_excl` in place of `beam_select_ens`).
    prefix: a forced beginning as in `beam_nbest`; a forced word's value is the members' combined one."""
    return _nbest_search(models, weights, mode, visual_feats, region_feats, n_best, length_penalty, no_repeat_ngram, min_len, beam_size,
                         num_groups, diversity_penalty, exclude, prefix)


class EnsembleSampleNotCovered(ValueError):
    """`Ensemble.sample` where it cannot run: with a keyword the sampled ensemble loop does not cover (prefix, share_encoder), or on
    members whose ops object has no `sample_ens`.  A ValueError that names the combination."""


def check_ensemble_sample(ops, dec, B, device, n, temperature, top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, exclude=None,
                          prefix=None, share_encoder=None):
    """ValueError for what `ensemble_sample` cannot run, before any encoder does; returns the two exclusion tables (None, None without)"""
    if prefix is not None:
        raise EnsembleSampleNotCovered('prefix and Ensemble.sample: a forced beginning is not covered (the force launch writes one '
                                       'member\'s embedding, and a forced word under c / temperature is a design of its own)')
    if share_encoder is not None:
        raise EnsembleSampleNotCovered('share_encoder and Ensemble.sample: the ensemble\'s loop always runs every member\'s encoder '
                                       'once per clip; there is nothing to switch')
    if int(n) != n or n < 1:
        raise ValueError('n (%r): Ensemble.sample draws 1 or more captions per clip' % (n,))
    if not temperature >= 0.0:                                         # (NaN fails the comparison)
        raise ValueError('temperature (%r) must not be negative or NaN (0: greedy)' % (temperature,))
    _check_max_words(dec.max_words, 'the ensemble\'s sampled step')
    E.check_sample_options(dec.max_words, top_k, top_p, min_len, no_repeat_ngram, dec.vocab_size)
    tables = E.sample_exclusions(exclude, B, device, dec.max_words, dec.vocab_size)
    if not hasattr(ops, 'sample_ens'):
        raise EnsembleSampleNotCovered('Ensemble.sample: %s has no sample_ens, the word step that draws from the members\' combined '
                                       'distribution' % type(ops).__name__)
    return tables if tables is not None else (None, None)


@torch.no_grad()
def ensemble_sample(models, weights, mode, visual_feats, region_feats, n=1, temperature=1.0, seed=None, top_k=0, top_p=1.0, min_len=0,
                    no_repeat_ngram=0, exclude=None, return_kept=False, prefix=None, share_encoder=None):
    """n captions per clip drawn from the ENSEMBLE's distribution: at every word the members' logit rows are combined into c
    (`beam_select_ens`'s rule: mode 0 the log of the weighted mean probability, mode 1 the weighted mean log-probability) and the
    word is drawn with probability proportional to exp(c / temperature) over the words the controls keep -- the temperature tempers
    the combined distribution, not each member's; temperature 0 is greedy on c.  -> (ids (B*n, L) int64, logp (B*n, L) float32,
    lens (B*n,) int64[, kept (B*n, L) int32]) as `CapGnnModel.sample` returns them, clip b owning rows b*n .. b*n + n - 1; logp is
    the drawn word's log-probability under the renormalised distribution it was drawn from, kept the number of words it was drawn
    from (always written here, so return_kept needs no control on).
    The loop is the ensemble search's on rows that never change parents: every member encodes its B clips once and steps its own
    state on R = B*n rows in eval mode (`_beam_setup` with k = n, the state gather on identity rows), and ONE `sample_ens` launch
    per word combines the members' rows and draws -- row t of a time-major (L, R) id buffer, which is also the rows' history.  The
    noise of row r at word t is keyed ((t + 1) R + r) V + j under (seed, SITE_SAMPLE): the noise `CapGnnModel.sample` gives that row
    (an ensemble of one model ranks x - lse + noise where the model's own sampler ranks x + noise: the same draw up to the rounding
    of the subtraction).  seed None draws the first
    member's next seed; it may be a device word (a captured graph).  Nothing is read back.
    top_k, top_p, min_len, no_repeat_ngram, exclude: the controls of `CapGnnModel.sample`, on the combined values; per-clip exclusions
    are indexed by clip.  prefix and share_encoder are refused (`EnsembleSampleNotCovered`)."""
    dec, ops = models[0].decoder, models[0].ops
    shared, per_clip = check_ensemble_sample(ops, dec, visual_feats.shape[0], visual_feats.device, n, temperature, top_k, top_p, min_len,
                                             no_repeat_ngram, exclude, prefix, share_encoder)
    n = int(n)
    if seed is None:
        seed = models[0].next_seed()                                   # (before the encoders draw their own)
    steps = []
    for model in models:
        mems, sv, own, _ = _encode(model, visual_feats, region_feats)
        advance, B, R, L = _beam_setup(model, mems, sv, own, n)
        steps.append(advance)
    dev, end = mems[0].device, dec.vocab('<end>')
    ids = torch.empty(L, R, dtype=torch.int64, device=dev)             # time-major: row t is step t's words, rows < t its history
    logp = torch.empty(L, R, dtype=torch.float32, device=dev)
    kept = torch.empty(L, R, dtype=torch.int32, device=dev)
    lens = torch.full((R,), L, dtype=torch.int64, device=dev)
    comb = torch.empty(R, dec.vocab_size, dtype=torch.float32, device=dev)
    rows = torch.arange(R, dtype=torch.int64, device=dev)             # a row is its own parent at every step
    words = torch.full((R,), dec.vocab('<start>'), dtype=torch.int64, device=dev)
    for t in range(L):
        logits = [advance(t, words, rows) for advance in steps]
        ops.sample_ens(logits, weights, mode, comb, ids[t], logp[t], lens, t, end, temperature=float(temperature), seed=seed,
                       site_sample=E.SITE_SAMPLE, row0=(t + 1) * R, top_k=top_k, top_p=top_p, min_len=min_len,
                       no_repeat_ngram=no_repeat_ngram, hist=ids, kept=kept[t], excl_shared=shared, excl_clip=per_clip, rows_per_clip=n)
        words = ids[t]
    out = ids.t().contiguous(), logp.t().contiguous(), lens
    return out + (kept.t().contiguous(),) if return_kept else out


def check_stochastic_options(n, L, V, temperature, min_len=0, no_repeat_ngram=0, return_threshold=False):
    """ValueError for what `stochastic_nbest` cannot run; returns the number of beams: n, one more with the threshold"""
    top = MAX_BEAM - 1 if return_threshold else MAX_BEAM
    if not 1 <= n <= top:
        raise ValueError('n %r: sampling without replacement draws 1 to %d captions per clip%s'
                         % (n, top, ' with return_threshold (it runs one more beam)' if return_threshold else ''))
    k = n + 1 if return_threshold else n
    if not temperature > 0.0:                                          # (NaN fails the comparison)
        raise ValueError('temperature (%r) must be positive' % (temperature,))
    _check_max_words(L, 'the search')
    _check_bans(L, no_repeat_ngram, min_len)
    if V < k:
        raise ValueError('vocabulary size (%d) too small for %d beams' % (V, k))
    return k


@torch.no_grad()
def stochastic_nbest(model, visual_feats, region_feats, n=5, temperature=1.0, seed=None, min_len=0, no_repeat_ngram=0,
                     return_threshold=False, exclude=None, prefix=None):
    """Stochastic beam search (Kool, van Hoof & Welling 2019): n DISTINCT captions per clip that are an exact ordered sample without
    replacement from softmax(logits / temperature), renormalised over the words min_len and no_repeat_ngram leave -- row 0 is
    distributed as one ordinary sample, rows 0 .. m-1 as a without-replacement sample of size m.  Returns (ids (B, n, L) int64
    padded with <end>, logp (B, n) float32 the captions' log-probabilities under that model, lens (B, n) int64 counting the first
    <end>, else L).  return_threshold=True runs n + 1 beams and adds (gumbel (B, n) float64, the rows' perturbed log-probabilities,
    descending; kappa (B,) float64, that of beam n + 1): `importance_weights(logp, kappa)` then weighs the n rows into an unbiased
    estimator of any expectation under the model.
    The search is `beam_nbest`'s -- eval-mode decode, state ping-pong, one select launch per word, all L steps launched, nothing read
    back -- on `beam_select_gumbel`, whose noise is `sample`'s: with n = 1 the words are those of `model.eval().sample(n=1,
    temperature, seed)`.  seed None draws the model's next seed; it may be a device word (a captured graph).
    exclude: the `Exclusions` of `pack_exclusions` -- the step is `beam_select_gumbel_excl`, whose banned words are those of the
    two other bans and the last words of the entries a beam's history leads up to; the model is renormalised over the words that
    are left, as with the other two (the beam search under exclusions does not renormalise).  None, or two empty tables, launches
    what the call launched without the keyword.
    prefix: not covered -- anything but None is a ValueError (the perturbed value of a forced node is a design of its own)."""
    if prefix is not None:
        raise PrefixNotCovered('prefix and sample_without_replacement: a forced beginning is not covered in stochastic beam search')
    dec = model.decoder
    L = dec.max_words
    k = check_stochastic_options(n, L, dec.vocab_size, temperature, min_len, no_repeat_ngram, return_threshold)
    shared, per_clip = (None, None) if exclude is None else check_exclusions(exclude, visual_feats.shape[0], visual_feats.device)
    if shared is not None or per_clip is not None:
        require_excl_step(model.ops, 'beam_select_gumbel_excl')
    if seed is None:
        seed = model.next_seed()                                       # (before the encoder draws its own)
    G = []                                                             # the beams' perturbed values (2, R), ping-pong

    def select(t, logits, step):
        if t == 0:                                                     # (beside the search's buffers, behind the encoder)
            G.append(torch.zeros(2, step[0].shape[0], dtype=torch.float64, device=step[0].device))
        options = dict(temperature=float(temperature), seed=seed, site_sample=E.SITE_SAMPLE, no_repeat_ngram=no_repeat_ngram, min_len=min_len)
        if shared is None and per_clip is None:
            model.ops.beam_select_gumbel(logits[0], *step, G[0][t % 2], G[0][(t + 1) % 2], **options)
        else:
            model.ops.beam_select_gumbel_excl(logits[0], *step, G[0][t % 2], G[0][(t + 1) % 2], shared, per_clip, **options)
    hist, lps = _hist_search([model], k, visual_feats, region_feats, select)
    ids = hist.view(-1, k, L)
    B = ids.shape[0]
    # words before the first <end>, plus that <end>: L for a row without one
    lens = ((ids == dec.vocab('<end>')).cumsum(2) == 0).sum(2).add_(1).clamp_(max=L)
    out = ids[:, :n].contiguous(), lps.view(B, k)[:, :n].contiguous(), lens[:, :n].contiguous()
    if return_threshold:
        Gk = G[0][L % 2].view(B, k)
        out += (Gk[:, :n].contiguous(), Gk[:, n].contiguous())
    return out


def importance_weights(logp, kappa):
    """The weights that turn the n rows of `stochastic_nbest(..., return_threshold=True)` into an unbiased estimator: with phi =
    logp (B, n) and kappa (B,) the perturbed value of beam n + 1, w = exp(phi) / q, q = 1 - exp(-exp(phi - kappa)) the probability
    that the caption's perturbed value exceeds kappa; sum_i w_i f(y_i) estimates E_p[f].  float64 (B, n)."""
    phi = logp.double()
    return phi.exp() / -torch.expm1(-(phi - kappa.double().unsqueeze(1)).exp())


MAX_CONSTRAINTS, MAX_ALTERNATIVES, MAX_PHRASE = 8, 8, 4          # DLSG_CONS_MAX, DLSG_CONS_ALT, DLSG_PHRASE_MAX


def _pack(per_clip, vocab, device, skip_unknown, phrases):
    """The packer of both constraint tensors: (B, C, W, P) int64 padded with -1 from per-clip lists of constraints, each one
    alternative or a collection of them.  phrases says how a constraint's alternatives are read: as phrases (a string is split on
    whitespace, a tuple is one phrase of words or ids) or as single words (a tuple is a collection of alternatives; P is 1 and the
    axis is dropped).  An alternative with a word outside the vocabulary is refused or, with skip_unknown, dropped whole."""
    special = {vocab(w) for w in ('<end>', '<start>', '<pad>') if w in vocab.word2idx}
    collections = (list, set, frozenset) if phrases else (list, tuple, set, frozenset)
    packed = []
    for b, clip in enumerate(per_clip):
        if len(clip) > MAX_CONSTRAINTS:
            raise ValueError('clip %d: %d constraints, at most %d per clip' % (b, len(clip), MAX_CONSTRAINTS))
        sets = []
        for con in clip:
            alts = []
            for a in (list(con) if isinstance(con, collections) else [con]):
                words = [a] if not phrases else a.split() if isinstance(a, str) else list(a) if isinstance(a, tuple) else [a]
                if not words:
                    raise ValueError('clip %d: an empty phrase %r' % (b, a))
                if len(words) > MAX_PHRASE:
                    raise ValueError('clip %d: %r has %d words, at most %d per phrase' % (b, a, len(words), MAX_PHRASE))
                ids = []
                for wd in words:
                    if isinstance(wd, str):
                        i = vocab.word2idx.get(wd, -1)
                    else:
                        i = int(wd) if 0 <= int(wd) < len(vocab) else -1
                    if i < 0:
                        if skip_unknown:
                            break
                        raise ValueError('clip %d: %r is not in the vocabulary' % (b, wd))
                    if i in special:
                        raise ValueError('clip %d: %r cannot be required (<end>, <start> and <pad> are not words of a caption)' % (b, wd))
                    ids.append(i)
                if len(ids) == len(words) and ids not in alts:
                    alts.append(ids)
            if len(alts) > MAX_ALTERNATIVES:
                raise ValueError('clip %d: %d alternatives in one constraint, at most %d' % (b, len(alts), MAX_ALTERNATIVES))
            sets.append(alts)
        packed.append(sets)
    C = max([len(s) for s in packed] + [0])
    W = max([len(alts) for s in packed for alts in s] + [1])
    P = max([len(ids) for s in packed for alts in s for ids in alts] + [1])
    out = torch.full((len(packed), C, W, P), -1, dtype=torch.int64)
    for b, sets in enumerate(packed):
        for c, alts in enumerate(sets):
            for w, ids in enumerate(alts):
                out[b, c, w, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    out = out if phrases else out.squeeze(3)
    return out if device is None else out.to(device)


def pack_constraints(per_clip, vocab, device=None, skip_unknown=False):
    """The constraint tensor of `constrained_nbest`: (B, C, W) int64 padded with -1.  per_clip: for every clip a list of
    constraints, each a word, a word id or a list of alternatives (words or ids) of which the caption must contain one.
    ValueError for more than 8 constraints per clip or 8 alternatives per constraint, for <end>, <start> or <pad> in a set, and
    for a word outside the vocabulary -- unless skip_unknown: then the alternative is dropped, and a constraint left with none is
    absent."""
    return _pack(per_clip, vocab, device, skip_unknown, phrases=False)


def _check_packed(k, L, B, cons, device, phrases, n_best, length_penalty, no_repeat_ngram, min_len):
    """ValueError for what `constrained_nbest` cannot run on a packed tensor, (B, C, W) words or (B, C, W, P) phrases: what
    `check_nbest_options` refuses, a tensor of the wrong shape, dtype or device, or with more constraints than words; returns n"""
    n = check_nbest_options(k, L, n_best, length_penalty, no_repeat_ngram, min_len)
    axes, packer = ('(B, C, W, P)', 'pack_phrases') if phrases else ('(B, C, W)', 'pack_constraints')
    if not torch.is_tensor(cons) or cons.dtype != torch.int64:
        raise ValueError('constraints: an int64 tensor %s (%s makes one), not %s'
                         % (axes, packer, cons.dtype if torch.is_tensor(cons) else type(cons).__name__))
    if cons.dim() != (4 if phrases else 3) or cons.shape[0] != B:
        raise ValueError('constraints of shape %s: %s with B = %d clips' % (tuple(cons.shape), axes, B))
    limits = (MAX_ALTERNATIVES, MAX_PHRASE) if phrases else (MAX_ALTERNATIVES,)
    if cons.shape[1] > MAX_CONSTRAINTS or (cons.shape[1] > 0 and not all(1 <= s <= m for s, m in zip(cons.shape[2:], limits))):
        raise ValueError('constraints of shape %s: at most %d constraints per clip of 1 to %d alternative%s'
                         % (tuple(cons.shape), MAX_CONSTRAINTS, MAX_ALTERNATIVES, ' phrases of 1 to %d words' % MAX_PHRASE if phrases else 's'))
    if cons.device != device:
        raise ValueError('constraints on %s, the clips on %s' % (cons.device, device))
    if cons.shape[1] + 1 > L:
        raise ValueError('%d constraints and <end> do not fit into max_words %d' % (cons.shape[1], L))
    return n


def check_constrained_options(k, L, B, cons, device, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0):
    """ValueError for what `constrained_nbest` cannot run (what `check_nbest_options` refuses, and a constraint tensor of the wrong
    shape, dtype or device, or with more constraints than words: a caption of max_words tokens holds max_words - 1 words and
    <end>; the tensor's C counts, since nothing is read back); returns n"""
    return _check_packed(k, L, B, cons, device, False, n_best, length_penalty, no_repeat_ngram, min_len)


def _is_phrase_string(x):
    """a string that is more than one word"""
    return isinstance(x, str) and x.split() != [x]


def has_phrases(per_clip):
    """whether per-clip constraint lists hold a string with whitespace in it: then they are phrases (`pack_phrases`), else the
    words and sets of words of `pack_constraints`"""
    for clip in per_clip:
        for con in clip:
            if any(_is_phrase_string(a) for a in (con if isinstance(con, (list, tuple, set, frozenset)) else [con])):
                return True
    return False


def pack_phrases(per_clip, vocab, device=None, skip_unknown=False):
    """The phrase tensor of `constrained_nbest`: (B, C, W, P) int64 padded with -1.  per_clip: for every clip a list of
    constraints, each a phrase or a list (or set) of alternative phrases of which the caption must contain one as contiguous
    words; a phrase is a string, split on whitespace, a tuple of words or word ids, or a single word or id.  ValueError for more
    than 8 constraints per clip, 8 alternatives per constraint or 4 words per phrase, for an empty phrase, for <end>, <start> or
    <pad> inside a phrase, and for a word outside the vocabulary -- unless skip_unknown: then the whole alternative is dropped, and
    a constraint left with none is absent.  Alternatives that are equal are folded."""
    return _pack(per_clip, vocab, device, skip_unknown, phrases=True)


def check_phrase_options(k, L, B, phr, device, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0):
    """ValueError for what `constrained_nbest` cannot run on a phrase tensor: what `check_nbest_options` refuses, a tensor of the
    wrong shape, dtype or device, or with more constraints than words (C + 1 > max_words: the tensor's C counts, since nothing is
    read back); returns n"""
    return _check_packed(k, L, B, phr, device, True, n_best, length_penalty, no_repeat_ngram, min_len)


def check_phrases_fit(phr, L):
    """ValueError if a clip of a host tensor of `pack_phrases` needs more than max_words for the search's guarantee: C_b constraints
    of at most n_max_b words, and <end>"""
    if phr.numel():
        lens = (phr >= 0).sum(3)                                       # (pack_phrases pads behind the words only)
        need = (lens > 0).any(2).sum(1) * lens.amax((1, 2)) + 1
        if int(need.max()) > L:
            b = int(need.argmax())
            raise ValueError('clip %d: %d phrase constraints of up to %d words and <end> do not fit into max_words %d'
                             % (b, int((lens[b] > 0).any(1).sum()), int(lens[b].max()), L))


def phrases_met(ids, phrases, vocab_size=None):
    """How many of its clip's phrase constraints every caption contains: ids (B, n, L) or (B, L) int64, phrases (B, C, W, P) int64 as
    `pack_phrases` makes them (a phrase: the leading run of ids in [0, vocab_size), any id >= 0 without vocab_size) -> (B, n) or
    (B,) int64, the number of constraints with an alternative that stands in the caption as contiguous tokens.  Device tensors in,
    a device tensor out, nothing is read back; any captions, not only a search's."""
    if ids.dim() not in (2, 3) or phrases.dim() != 4 or ids.shape[0] != phrases.shape[0]:
        raise ValueError('phrases_met: ids (B, n, L) or (B, L) and phrases (B, C, W, P), not %s and %s' % (tuple(ids.shape), tuple(phrases.shape)))
    rows = ids if ids.dim() == 3 else ids.unsqueeze(1)
    B, n, L = rows.shape
    _, C, W, P = phrases.shape
    valid = phrases >= 0 if vocab_size is None else (phrases >= 0) & (phrases < vocab_size)
    run = valid.long().cumprod(3).bool()                               # (B, C, W, P): word j belongs to the phrase
    # the P tokens from every position on, -2 behind the caption's end
    win = torch.cat([rows, rows.new_full((B, n, max(P - 1, 0)), -2)], 2).unfold(2, P, 1) if P else rows.new_zeros(B, n, L, 0)
    same = (win.view(B, n, L, 1, 1, P) == phrases.view(B, 1, 1, C, W, P)) | ~run.view(B, 1, 1, C, W, P)
    occurs = same.all(5) & run[..., :1].reshape(B, 1, 1, C, W)         # an absent alternative occurs nowhere
    met = occurs.any(2).any(3).sum(2)                                  # (B, n)
    return met if ids.dim() == 3 else met[:, 0]


def _constraints_met(ids, cons, vocab_size):
    """How many of its clip's constraints every row of ids (B, k, L) meets -> (B, k) int64: `phrases_met` for a (B, C, W, P) tensor;
    for (B, C, W) words the same integers from a broadcast compare of the ids with the valid entries (padding never matches),
    which is fewer launches inside a captured search"""
    if cons.dim() == 4:
        return phrases_met(ids, cons, vocab_size)
    B, k, L = ids.shape
    valid = (cons >= 0) & (cons < vocab_size)
    hit = (ids.view(B, k, L, 1, 1) == cons.view(B, 1, 1, *cons.shape[1:])) & valid.view(B, 1, 1, *cons.shape[1:])
    return hit.any(4).any(2).sum(2)


# ---------------------------------------------------------------------------------------------- exclusions
MAX_EXCL_SHARED, MAX_EXCL_CLIP = 64, 32                          # DLSG_EXCL_SHARED, DLSG_EXCL_CLIP
# the words a caption should not stop behind (self-critical.pytorch, utils/misc.py: bad_endings)
BAD_ENDINGS = ('a', 'an', 'the', 'in', 'for', 'at', 'of', 'with', 'before', 'after', 'on', 'upon', 'near', 'to', 'is', 'are', 'am')

Exclusions = collections.namedtuple('Exclusions', ['shared', 'per_clip'])
Exclusions.__doc__ = """What `beam_search(exclude=...)` must not emit, as `beam_select_excl` reads it: shared (NS <= 64, P) int64 or None,
the entries that hold for every clip, and per_clip (B, NC <= 32, P) int64 or None, each clip's own; an entry is a row of up to P <= 4
word ids padded with -1, whose last word is banned behind its other words.  `pack_exclusions` makes one."""


def _excluded_entry(phrase, vocab, where, skip_unknown):
    """one excluded phrase -- a string, split on whitespace, a tuple of words or ids, or one word or id -- as a list of ids; None
    for a phrase with a word outside the vocabulary under skip_unknown; ValueError for what cannot be excluded"""
    words = phrase.split() if isinstance(phrase, str) else list(phrase) if isinstance(phrase, (tuple, list)) else [phrase]
    if not words:
        raise ValueError('%san empty phrase %r' % (where, phrase))
    if len(words) > MAX_PHRASE:
        raise ValueError('%s%r has %d words, at most %d per phrase' % (where, phrase, len(words), MAX_PHRASE))
    never = {vocab.word2idx[w] for w in ('<start>', '<pad>') if w in vocab.word2idx}
    end = vocab.word2idx.get('<end>', -1)
    ids = []
    for j, wd in enumerate(words):
        if isinstance(wd, str):
            i = vocab.word2idx.get(wd, -1)                              # (<unk> written out is a word of the vocabulary)
        else:
            i = int(wd) if 0 <= int(wd) < len(vocab) else -1
        if i < 0:
            if skip_unknown:
                return None
            raise ValueError('%s%r is not in the vocabulary' % (where, wd))
        if i in never:
            raise ValueError('%s%r cannot be excluded (<start> and <pad> are never chosen)' % (where, wd))
        if i == end and (j + 1 < len(words) or len(words) < 2):
            raise ValueError('%s%r: <end> can only be the last of at least two words (a bad ending)' % (where, phrase))
        ids.append(i)
    return ids


def pack_exclusions(vocab, words=(), phrases=(), bad_endings=False, suppress_unk=False, per_clip=None, device=None, skip_unknown=False):
    """The `Exclusions` of `beam_search(exclude=...)`: two int64 tensors padded with -1, shared (NS, P) -- None without a shared
    entry -- and per_clip (B, NC, P) -- None without the argument.  words: words or ids no caption may contain; phrases: phrases no
    caption may contain as contiguous words, each a string, split on whitespace, a tuple of words or ids, or one word or id;
    bad_endings=True: no caption stops behind a word of `BAD_ENDINGS` (those the vocabulary has), a sequence of words in its place:
    behind one of those; suppress_unk: `<unk>` is never emitted; per_clip: for every clip a list of further phrases.  Equal entries
    are folded.  ValueError for more than 64 shared or 32 per-clip entries, more than 4 words in a phrase, an empty phrase, <start>
    or <pad> in a phrase, <end> anywhere but as the last of at least two words, and for a word outside the vocabulary (`<unk>`
    written out is allowed) -- unless skip_unknown: then that entry is dropped."""
    def entries(items, where):
        out = []
        for it in items:
            ids = _excluded_entry(it, vocab, where, skip_unknown)
            if ids is not None and ids not in out:
                out.append(ids)
        return out
    shared = [(w,) if isinstance(w, str) else w for w in words] + list(phrases)
    if suppress_unk:
        shared.append(('<unk>',))
    if bad_endings is True:
        shared += [(w, '<end>') for w in BAD_ENDINGS if w in vocab.word2idx]
    elif bad_endings:
        shared += [(w, '<end>') for w in bad_endings]
    shared = entries(shared, '')
    if len(shared) > MAX_EXCL_SHARED:
        raise ValueError('%d shared exclusions, at most %d' % (len(shared), MAX_EXCL_SHARED))
    clips = None if per_clip is None else [entries(clip, 'clip %d: ' % b) for b, clip in enumerate(per_clip)]
    for b, clip in enumerate(clips or []):
        if len(clip) > MAX_EXCL_CLIP:
            raise ValueError('clip %d: %d exclusions, at most %d per clip' % (b, len(clip), MAX_EXCL_CLIP))
    P = max([len(e) for e in shared] + [len(e) for clip in clips or [] for e in clip] + [1])

    def table(rows, n):
        out = torch.full((n, P), -1, dtype=torch.int64)
        for a, ids in enumerate(rows):
            out[a, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
        return out
    sh = table(shared, len(shared)) if shared else None
    pc = None
    if clips is not None:
        NC = max([len(clip) for clip in clips] + [0])
        pc = torch.stack([table(clip, NC) for clip in clips]) if clips else torch.full((0, NC, P), -1, dtype=torch.int64)
    if device is not None:
        sh, pc = (None if x is None else x.to(device) for x in (sh, pc))
    return Exclusions(sh, pc)


class ExcludeNotCovered(TypeError, ValueError):
    """`exclude` where it cannot be honoured: given to a search that does not cover exclusions, or to a model whose ops object has
    no step under exclusions.  A ValueError that names the combination -- and a TypeError, which is what these calls raised while they
    took no such keyword, so that code written against them keeps catching it."""


def require_excl_step(ops, step):
    """ExcludeNotCovered unless `ops` implements `step`, the launch a decode under exclusions makes at every word (HipOps does; an
    ops object written before the step existed does not): raised before the encoder runs, not as an AttributeError at the first word"""
    if not hasattr(ops, step):
        raise ExcludeNotCovered('exclude: %s has no %s, the word step under exclusions' % (type(ops).__name__, step))


def check_exclusions(exclude, B, device, num_groups=1):
    """ValueError for an `exclude` the n-best search cannot run on B clips on `device`: not an `Exclusions`, a table of the wrong
    dtype, rank, device or size, a per-clip table whose first dimension is not the batch, two tables of different P, or together
    with beam groups; returns the two tables, contiguous (None for an absent or empty one)"""
    if num_groups > 1:
        raise ValueError('exclude and num_groups = %d: exclusions are not covered in diverse beam search' % num_groups)
    if not isinstance(exclude, tuple) or len(exclude) != 2:
        raise ValueError('exclude: an Exclusions(shared, per_clip) (pack_exclusions makes one), not %s' % type(exclude).__name__)
    out, P = [], None
    for tab, d, lim, what in ((exclude[0], 2, MAX_EXCL_SHARED, 'shared'), (exclude[1], 3, MAX_EXCL_CLIP, 'per-clip')):
        if tab is None:
            out.append(None)
            continue
        axes = '(NS, P)' if d == 2 else '(B, NC, P)'
        if not torch.is_tensor(tab) or tab.dtype != torch.int64 or tab.dim() != d:
            raise ValueError('exclude: the %s table is an int64 tensor %s, not %s'
                             % (what, axes, '%s %s' % (tab.dtype, tuple(tab.shape)) if torch.is_tensor(tab) else type(tab).__name__))
        if d == 3 and tab.shape[0] != B:
            raise ValueError('exclude: the per-clip table of shape %s holds %d clips, the batch %d' % (tuple(tab.shape), tab.shape[0], B))
        if tab.shape[-2] > lim or (tab.shape[-2] > 0 and not 1 <= tab.shape[-1] <= MAX_PHRASE):
            raise ValueError('exclude: the %s table of shape %s: at most %d entries of 1 to %d words' % (what, tuple(tab.shape), lim, MAX_PHRASE))
        if tab.device != device:
            raise ValueError('exclude: the %s table on %s, the clips on %s' % (what, tab.device, device))
        if tab.shape[-2] == 0:
            out.append(None)
            continue
        if P not in (None, tab.shape[-1]):
            raise ValueError('exclude: the shared table has %d words per entry, the per-clip table %d' % (P, tab.shape[-1]))
        P = tab.shape[-1]
        out.append(tab.contiguous())
    return out


def exclusions_hit(ids, lens, exclusions, vocab_size=None):
    """How often captions contain what is excluded: ids (B, n, L) or (B, L) int64, lens (B, n) or (B,) int64 as a search returns
    them, exclusions an `Exclusions` (an entry: the leading run of ids in [0, vocab_size), of any id >= 0 without vocab_size) ->
    (B, n) or (B,) int64, the number of positions p < lens at which an entry ends, that is ids[p - n + 1 .. p] equals an entry of n
    words -- a bad ending ends at the caption's <end>, which lens counts.  0 everywhere is what `beam_search(exclude=...)` owes for
    every caption of finite score.  Torch operations on the tensors' device, nothing is read back; any captions, not only a search's."""
    rows, ln = (ids, lens) if ids.dim() == 3 else (ids.unsqueeze(1), lens.unsqueeze(1))
    B, n, L = rows.shape
    tabs = []
    if exclusions[0] is not None and exclusions[0].shape[0]:
        tabs.append(exclusions[0].to(rows.device).unsqueeze(0).expand(B, *exclusions[0].shape))
    if exclusions[1] is not None and exclusions[1].shape[1]:
        if exclusions[1].shape[0] != B:
            raise ValueError('exclusions_hit: the per-clip table holds %d clips, ids %d' % (exclusions[1].shape[0], B))
        tabs.append(exclusions[1].to(rows.device))
    hits = torch.zeros(B, n, L, dtype=torch.bool, device=rows.device)
    for tab in tabs:                                                   # (B, N, P)
        P = tab.shape[2]
        valid = tab >= 0 if vocab_size is None else (tab >= 0) & (tab < vocab_size)
        run = valid.long().cumprod(2)
        m = run.sum(2)                                                 # (B, N): the entries' lengths
        # the entry right-aligned in its P slots: slot s holds word s - (P - m)
        src = torch.arange(P, device=rows.device).view(1, 1, P) - (P - m).unsqueeze(2)
        right = tab.gather(2, src.clamp(min=0))
        used = src >= 0
        # the P tokens that end at every position, -2 before the caption's start
        win = torch.cat([rows.new_full((B, n, P - 1), -2), rows], 2).unfold(2, P, 1)       # (B, n, L, P)
        same = (win.unsqueeze(3) == right.view(B, 1, 1, -1, P)) | ~used.view(B, 1, 1, -1, P)
        hits |= (same.all(4) & (m > 0).view(B, 1, 1, -1)).any(3)
    below = torch.arange(L, device=rows.device).view(1, 1, L) < ln.unsqueeze(2)
    out = (hits & below).sum(2)
    return out if ids.dim() == 3 else out[:, 0]


# ---------------------------------------------------------------------------------------------- forced prefixes
def pack_prefix(per_clip, vocab, device=None, max_words=None, allow_unk=False):
    """The prefix tensor of `beam_search(prefix=...)` and `sample(prefix=...)`: (B, P) int64 padded with -1, P the longest prefix
    (0 when no clip has one).  per_clip: for every clip how its captions begin -- a string, split on whitespace, a tuple or list
    of words or ids, or None / '' for no prefix.  ValueError for <end>, <start> or <pad> in a prefix, for a word outside the
    vocabulary -- unless allow_unk: then it becomes `<unk>` (`<unk>` written out is always allowed) --, and, with max_words, for a
    prefix longer than max_words - 1 (a caption of max_words tokens holds max_words - 1 words and <end>)."""
    special = {vocab(w) for w in ('<end>', '<start>', '<pad>') if w in vocab.word2idx}
    rows = []
    for b, item in enumerate(per_clip):
        words = [] if item is None else item.split() if isinstance(item, str) else list(item) if isinstance(item, (tuple, list)) else None
        if words is None:
            raise ValueError('clip %d: a prefix is a string, a tuple or list of words or ids, or None, not %s' % (b, type(item).__name__))
        ids = []
        for wd in words:
            if isinstance(wd, str):
                i = vocab.word2idx.get(wd, -1)
            else:
                i = int(wd) if 0 <= int(wd) < len(vocab) else -1
            if i < 0 and allow_unk and '<unk>' in vocab.word2idx:
                i = vocab.word2idx['<unk>']
            if i < 0:
                raise ValueError('clip %d: %r is not in the vocabulary' % (b, wd))
            if i in special:
                raise ValueError('clip %d: %r cannot stand in a prefix (<end>, <start> and <pad> are not words of a caption)' % (b, wd))
            ids.append(i)
        if max_words is not None and len(ids) > max_words - 1:
            raise ValueError('clip %d: a prefix of %d words and <end> do not fit into max_words %d' % (b, len(ids), max_words))
        rows.append(ids)
    out = torch.full((len(rows), max([len(ids) for ids in rows] + [0])), -1, dtype=torch.int64)
    for b, ids in enumerate(rows):
        out[b, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    return out if device is None else out.to(device)


def check_prefix(prefix, B, device, L, vocab=None):
    """ValueError for a `prefix` a decode of B clips on `device` with max_words L cannot run on: not an int64 tensor (B, P) on that
    device, or P > L - 1; returns the tensor, contiguous, or None for P == 0.  With `vocab` a list in place of a tensor is packed
    first (`pack_prefix` with max_words L)."""
    if vocab is not None and isinstance(prefix, (list, tuple)):
        prefix = pack_prefix(prefix, vocab, device, max_words=L)
    if not torch.is_tensor(prefix) or prefix.dtype != torch.int64 or prefix.dim() != 2:
        raise ValueError('prefix: an int64 tensor (B, P) (pack_prefix makes one), not %s'
                         % ('%s %s' % (prefix.dtype, tuple(prefix.shape)) if torch.is_tensor(prefix) else type(prefix).__name__))
    if prefix.shape[0] != B:
        raise ValueError('prefix of shape %s holds %d clips, the batch %d' % (tuple(prefix.shape), prefix.shape[0], B))
    if prefix.device != device:
        raise ValueError('prefix on %s, the clips on %s' % (prefix.device, device))
    if prefix.shape[1] > L - 1:
        raise ValueError('prefix of %d words and <end> do not fit into max_words %d' % (prefix.shape[1], L))
    return prefix.contiguous() if prefix.shape[1] else None


class PrefixNotCovered(ValueError):
    """`prefix` where it cannot be honoured: given to a decode that does not cover a forced beginning, or to a model whose ops
    object has no force launch.  A ValueError that names the combination."""


def require_prefix_step(ops, step):
    """PrefixNotCovered unless `ops` implements `step`, the launch a decode under a forced prefix makes behind its word step (HipOps
    does; an ops object written before the launch existed does not): raised before the encoder runs"""
    if not hasattr(ops, step):
        raise PrefixNotCovered('prefix: %s has no %s, the launch behind the word step under a forced prefix' % (type(ops).__name__, step))


def search_prefix(ops, prefix, B, device, dec, num_groups=1):
    """what a history search does with its `prefix` keyword before the encoder runs: None stays None; otherwise beam groups are
    refused, the tensor (or list) is checked (`check_prefix`) and the ops object must have the force launch -> the tensor, or None
    for P == 0"""
    if prefix is None:
        return None
    if num_groups > 1:
        raise PrefixNotCovered('prefix and num_groups = %d: a forced beginning is not covered in diverse beam search (the later '
                               'groups\' beams would start at -inf)' % num_groups)
    prefix = check_prefix(prefix, B, device, dec.max_words, dec.vocab)
    if prefix is not None:
        require_prefix_step(ops, 'beam_force_prefix')
    return prefix


@torch.no_grad()
def constrained_nbest(model, visual_feats, region_feats, constraints, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0,
                      beam_size=None, return_met=False, exclude=None, prefix=None):
    """Lexically constrained beam search (dynamic beam allocation, Post & Vilar 2018): `beam_nbest` whose captions must contain a
    word of every constraint of their clip.  constraints: the (B, C, W) int64 tensor of `pack_constraints` on the clips' device
    (C sets of W alternative word ids per clip, -1 or an id outside the vocabulary for padding), or the per-clip lists, which are
    packed here.  Returns (ids, scores, lens) as `beam_nbest`, the rows of a clip ordered by the number of constraints they meet,
    most first, and by score within a number; return_met=True adds met (B, n) int64, that number.  A beam cannot end before it has
    met every constraint, and the beams are shared out over the banks "number of constraints met" at every word
    (`beam_select_cons`, include/dlsg.h), so row 0 meets every constraint whose set holds a word the model gives a finite logit.
    The loop is `beam_nbest`'s: the same buffers, all L steps launched, nothing read back -- the met masks are recomputed from the
    token history, so there is no further state.  Without constraints the result is `beam_nbest`'s, bit for bit.
    Phrases: a (B, C, W, P) int64 tensor of `pack_phrases`, or per-clip lists in which some string holds whitespace ("hot dog"),
    which are packed by it, require phrases as contiguous words: the same loop with one `beam_select_phrases` launch per word.  A
    3-D tensor and lists without such a string run what they always ran.  With phrases the banks are (constraints met, progress
    into a phrase); what a beam has met and how far into a phrase it is are recomputed from its history row, so there is still no state
    beside `_hist_search`'s and nothing is read back.  Lists are packed on the host, where the bound of the guarantee is checked:
    C_b constraints of up to n_max_b words meet within C_b * n_max_b words (no_repeat_ngram = 0, finite logits), which with <end>
    must fit into max_words.  With an n-gram ban the next word of a phrase can be banned although the phrase has not occurred: the
    search is then best effort, and a beam that cannot finish runs to max_words without <end>.  The rows of a clip are ordered by
    `phrases_met` of the final ids, most first, then by score.
    exclude: not covered -- anything but None is an `ExcludeNotCovered`, a ValueError (a required word could be an excluded one).
    prefix: a forced beginning as in `beam_nbest`.  A prefix word meets a constraint or advances a phrase like a word the search
    chose (what a beam has met is recomputed from its history row), and it overrides the <end> ban of unmet constraints as it does
    every other ban; return_met counts it."""
    if exclude is not None:
        raise ExcludeNotCovered('exclude and constraints: exclusions are not covered in constrained beam search')
    dec = model.decoder
    k, L = dec.beam_size if beam_size is None else beam_size, dec.max_words
    B, dev = visual_feats.shape[0], visual_feats.device
    phrases = constraints.dim() == 4 if torch.is_tensor(constraints) else has_phrases(constraints)
    if torch.is_tensor(constraints):
        cons = constraints
    elif phrases:
        cons = pack_phrases(constraints, dec.vocab)
        check_phrases_fit(cons, L)
        cons = cons.to(dev)
    else:
        cons = pack_constraints(constraints, dec.vocab, dev)
    n = _check_packed(k, L, B, cons, dev, phrases, n_best, length_penalty, no_repeat_ngram, min_len)
    cons = cons.contiguous()
    prefix = search_prefix(model.ops, prefix, B, dev, dec)

    def select(t, logits, step):                                   # (a 3-D tensor never runs the phrase step, which is slower)
        (model.ops.beam_select_phrases if phrases else model.ops.beam_select_cons)(logits[0], *step, cons, no_repeat_ngram, min_len)
    ids, scores, lens = _finalize(model, *_hist_search([model], k, visual_feats, region_feats, select, prefix), k, k, length_penalty)
    met = _constraints_met(ids, cons, dec.vocab_size)              # (B, k)
    order = met.sort(dim=1, descending=True, stable=True)[1][:, :n]
    out = (ids.gather(1, order.unsqueeze(2).expand(B, n, L)), scores.gather(1, order), lens.gather(1, order))
    return out + (met.gather(1, order),) if return_met else out


def constrained_beam_search(model, visual_feats, region_feats, constraints, **options):
    """`constrained_nbest`, the function form of `model.constrained_beam_search`"""
    return constrained_nbest(model, visual_feats, region_feats, constraints, **options)


def sample_without_replacement(model, visual_feats, region_feats, **options):
    """`stochastic_nbest`, the function form of `model.sample_without_replacement`"""
    return stochastic_nbest(model, visual_feats, region_feats, **options)


def beam_search(model, visual_feats, region_feats, beam_size=None, **options):
    """`beam_nbest` with `beam_size` beams (default: the decoder's own, which is not changed)"""
    return beam_nbest(model, visual_feats, region_feats, beam_size=beam_size, **options)


def sample(model_or_ensemble, visual_feats, region_feats, **options):
    """the function form of `model.sample` and `Ensemble.sample`: the object's own sampler with `options` -- a CapGnnModel's sampled
    decode, an ensemble's draw from its members' combined distribution (`ensemble_sample`)"""
    return model_or_ensemble.sample(visual_feats, region_feats, **options)

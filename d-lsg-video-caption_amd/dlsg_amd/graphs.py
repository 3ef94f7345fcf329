"""hipGraph capture and replay, in one place: entering and leaving the process's capture stream, the eager warm-up, capturing one
graph or a chain of segments, dropping a capture whose body raised, staging inputs into the static buffers a graph reads --
and the captured forms of inference built on it (GreedyGraph, SampleGraph, BeamGraph, NBestBeamGraph, StochasticBeamGraph,
ConstrainedBeamGraph, EnsembleBeamGraph, EnsembleSampleGraph, ConsensusBeamGraph, ScoreGraph, RescoreBeamGraph).  The Trainer (model.py), the GanTrainer (gan.py) and the SCSTTrainer (scst.py) capture through `capture` /
`capture_segments`."""
import torch


def stage(dst, src):
    """src into the static buffer `dst` a captured graph reads -- unless the caller filled that very buffer in place (a producer
    that writes a graph's inputs directly, `Trainer.static_inputs`): then there is nothing to copy"""
    if src.data_ptr() != dst.data_ptr():
        dst.copy_(src, non_blocking=True)


def capture_segments(dev, body, warmup):
    """Capture `body(cut)` on the device's capture stream as a chain of graphs that share one memory pool (a tensor allocated in
    one segment stays valid for the next): `cut(key, between=None)` ends the running segment under `key`, runs `between()` outside
    any capture and begins the next segment; the last one ends with the body, under the key None.  Returns ([(graph, key), ...] in
    replay order, the body's return value).
    `warmup()` runs first, eagerly, on the same stream: it warms the allocator and that stream's stream-K workspace
    (hip.HipOps._gemm_workspace), which must never be allocated inside a capture, and makes the one-time kernel attribute calls.
    If the body raises, the capture in progress is ended, the partial graphs are dropped and the exception propagates."""
    from .hip import HipOps
    side = HipOps.capture_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warmup()
        side.synchronize()
        pool, done, cur = torch.cuda.graph_pool_handle(), [], []

        def begin():
            cur.append(torch.cuda.CUDAGraph())
            # thread-local capture mode: calls made by other threads (e.g. the RCCL watchdog) cannot invalidate the capture
            cur[0].capture_begin(pool=pool, capture_error_mode='thread_local')

        def end(key=None):
            cur[0].capture_end()
            done.append((cur.pop(), key))

        def cut(key, between=None):
            end(key)
            if between is not None:
                between()
            begin()
        try:
            begin()
            out = body(cut)
            end()
        except BaseException:
            # leave no stream in capture mode behind: every capture of the process runs on this one, and a later synchronize
            # would raise on top of the real error
            if cur:
                try:
                    cur[0].capture_end()
                except Exception:
                    pass
            raise
    torch.cuda.current_stream().wait_stream(side)
    return done, out


def capture(dev, body, warmup=None):
    """Capture `body()` as one graph (see capture_segments; the warm-up defaults to the body itself).  Returns (graph, the body's
    return value): what the body returned are static buffers the replays write."""
    graphs, out = capture_segments(dev, lambda cut: body(), warmup or body)
    return graphs[0][0], out


def expand_rows(x, n):
    """x.repeat_interleave(n, 0) as one copy (row b*n + i = x[b]): no host synchronisation, so it may be captured"""
    if n == 1:
        return x
    return x.unsqueeze(1).expand(x.shape[0], n, *x.shape[1:]).reshape(x.shape[0] * n, *x.shape[1:])


def _members(model_or_ensemble):
    return list(getattr(model_or_ensemble, 'members', [model_or_ensemble]))


def _held_exclusions(options):
    """takes `exclude` out of a search's options -> (the other options, the graph's own copy of the two tables or None, the options
    the captured search runs with): the copies are static buffers like the inputs"""
    options = dict(options)
    exclude = options.pop('exclude', None)
    if exclude is None:
        return options, None, options
    exclude = type(exclude)(*[None if x is None else x.clone() for x in exclude])
    return options, exclude, dict(options, exclude=exclude)


def _held_prefix(model, options, device):
    """takes `prefix` out of the options a captured decode runs with -> (those options with the graph's own copy of the table in its
    place, the copy or None): a static buffer like the inputs; per-clip lists are packed here (`beam.pack_prefix`)"""
    prefix = options.get('prefix')
    if prefix is None:
        return options, None
    if not torch.is_tensor(prefix):
        from .beam import pack_prefix
        prefix = pack_prefix(prefix, model.decoder.vocab, device, max_words=model.decoder.max_words)
    prefix = prefix.clone()
    return dict(options, prefix=prefix), prefix


class _InferenceGraph(object):
    """A no-grad pass of `model` over (frames, regions), captured once for a batch shape and replayed: a subclass says what to
    run (`_run`, on the static inputs self.frames / self.regions; its return value becomes self.out).  A captured graph holds raw
    addresses into the parameter arena of every model it runs and their train / eval modes at construction -- `models` lists
    them where there are several (an ensemble's members; self.model is the first): `valid_for` tells whether the graph still
    fits, and a replay after a model re-packed its parameters (load_encoder, load_state_dict into a copy, .to()) raises instead
    of computing from the old arena.
    One more static input -- a seed word, a constraint tensor, caption ids: a subclass allocates its buffer before the capture,
    names the attribute that holds it in `extra` and defines `_fitted(value)`: the caller's value as what is copied into the buffer
    (a tensor like it, or host values), or ValueError; `graph(frames, regions, value)` then stages all three and replays."""

    extra = None

    def __init__(self, model, frames, regions, models=None):
        models = [model] if models is None else list(models)
        for m in models:
            m.flatten_parameters_()
        self.held = [(m, m._flat, m.training) for m in models]
        self.model, self.arena, self.training = self.held[0]
        self.frames, self.regions = frames.clone(), regions.clone()
        with torch.no_grad():
            self.graph, self.out = capture(frames.device, self._run)

    def valid_for(self, frames, regions):
        """this graph may be replayed on these inputs: same shapes, the arenas it was captured on, the same train / eval modes"""
        return self.frames.shape == frames.shape and self.regions.shape == regions.shape and \
            all(arena is m._flat and training == m.training for m, arena, training in self.held)

    def _stage(self, frames, regions):
        for i, (m, arena, _) in enumerate(self.held):
            if arena is not m._flat:
                raise RuntimeError('%s: %s re-packed its parameter arena after this graph was captured (flatten_parameters_ after '
                                   'load_encoder / load_state_dict / .to()); the graph holds addresses into the old arena -- build a '
                                   'new one' % (type(self).__name__, 'the model' if len(self.held) == 1 else 'member %d' % i))
        stage(self.frames, frames)
        stage(self.regions, regions)

    def _like_captured(self, x, what):
        """the tensor x if it has the shape, dtype and device of the `extra` buffer; ValueError otherwise"""
        buf = getattr(self, self.extra)
        if x.shape != buf.shape or x.dtype != buf.dtype or x.device != buf.device:
            raise ValueError('%s: %s of shape %s %s on %s, captured with %s int64 on %s -- build a new graph'
                             % (type(self).__name__, what, tuple(x.shape), x.dtype, x.device, tuple(buf.shape), buf.device))
        return x

    @torch.no_grad()
    def __call__(self, frames, regions, *value):
        if len(value) != (self.extra is not None):
            raise TypeError('%s takes (frames, regions%s)' % (type(self).__name__, ', ' + self.extra if self.extra else ''))
        if value:
            dst, src = getattr(self, self.extra), self._fitted(value[0])   # (refused before anything is staged)
        self._stage(frames, regions)
        if value:
            from .hip import copy_to_device
            stage(dst, src) if torch.is_tensor(src) else copy_to_device(dst, src)
        self.graph.replay()
        return self.out


class _SeededGraph(_InferenceGraph):
    """An inference graph that draws: the seed is read from a device word, so every replay draws afresh, and a replay with seed s
    gives the bits of the eager call with seed=s"""

    extra = 'seed'

    def __init__(self, model, frames, regions, models=None):
        self.seed = torch.zeros(1, dtype=torch.int64, device=frames.device)
        super().__init__(model, frames, regions, models)

    def _fitted(self, seed):
        return [int(seed)]


class GreedyGraph(_InferenceGraph):
    """hipGraph-captured greedy inference (BASELINE configs[4]: 'hipGraph-captured decode step'): encoder + the 26
    decode steps (argmax and embedding gather stay on device) are captured once for a batch shape and replayed; the
    ids are identical to the eager `model(frames, regions, None)` path with beam_size 1."""

    def _run(self):
        return self.model._greedy_ids(self.frames, self.regions, 0)[0]


class SampleGraph(_SeededGraph):
    """hipGraph-captured `CapGnnModel.sample`: the n-fold expansion of the batch, the encoder on B*n rows and the sampled decode
    steps, captured once for a batch shape (and for the model's train / eval mode at construction) and replayed.  The seed is
    read from a device word, so every replay draws fresh samples; a replay with seed s gives the bits of
    `model.sample(frames, regions, n, temperature, seed=s)`.  Outputs are static buffers, valid until the next replay.
    share_encoder=True captures `model.sample(..., share_encoder=True)` instead: the encoder on the B clips, their proposals
    fanned out in-graph (`rows_repeat`), the sampled decode steps on B*n rows; a replay with seed s gives that call's bits.
    top_k, top_p, min_len, no_repeat_ngram, return_kept: the sampling controls of `CapGnnModel.sample`, fixed at capture.
    exclude=Exclusions (`pack_exclusions`): kept as `graph.exclude`, the graph's own copy of the two tables, as NBestBeamGraph keeps
    it: `graph.exclude.shared.copy_(new)` changes what the next replay bans; the tables' shapes are fixed at capture.
    prefix=(B, P) int64 (`pack_prefix`, or the per-clip list it takes): kept as `graph.prefix`, the graph's own copy:
    `graph.prefix.copy_(new)` changes what the next replay's samples begin with; the shape is fixed at capture."""

    def __init__(self, model, frames, regions, n=1, temperature=1.0, share_encoder=False, top_k=0, top_p=1.0, min_len=0,
                 no_repeat_ngram=0, return_kept=False, exclude=None, prefix=None):
        self.n, self.temperature, self.share_encoder = n, temperature, bool(share_encoder)
        self.options, self.exclude, self._draw = _held_exclusions(dict(
            top_k=top_k, top_p=top_p, min_len=min_len, no_repeat_ngram=no_repeat_ngram, return_kept=return_kept, exclude=exclude))
        self._draw, self.prefix = _held_prefix(model, self._draw if prefix is None else dict(self._draw, prefix=prefix), frames.device)
        super().__init__(model, frames, regions)

    def _run(self):
        return self.model.sample(self.frames, self.regions, self.n, self.temperature, self.seed, self.share_encoder, **self._draw)


class BeamGraph(_InferenceGraph):
    """hipGraph-captured beam search (BASELINE configs[4]): encoder + all max_words beam steps (decode step, `beam_select`,
    state reorder) captured once for a batch shape; a replay has no host synchronisation, the early stop of the reference is
    applied afterwards (`beam.beam_finish`).  Ids are identical to `model(frames, regions, None)` with the same beam size."""

    def _run(self):
        from .beam import beam_device
        return beam_device(self.model, self.frames, self.regions, early_exit=False)

    @torch.no_grad()
    def __call__(self, frames, regions):
        from .beam import beam_finish
        return beam_finish(self.model, *super().__call__(frames, regions))


class NBestBeamGraph(_InferenceGraph):
    """hipGraph-captured `model.beam_search(frames, regions, **options)` for one batch shape: encoder, all max_words steps with
    the beams' token history, and the ranking.  A replay returns (ids, scores, lens) -- static buffers, valid until the next
    replay -- and synchronises nothing (call `model.ops.check_persistent()` where the ids are read back).
    exclude=Exclusions (`pack_exclusions`): the graph keeps its own copy of the two tables as `graph.exclude` and captures their
    addresses: `graph.exclude.per_clip.copy_(new)` (or `.shared`) changes what the next replay bans; another shape needs a new
    graph.
    prefix=(B, P) int64 (`pack_prefix`, or the per-clip list it takes): the graph keeps its own copy as `graph.prefix`, like
    `graph.exclude`: `graph.prefix.copy_(new)` changes what the next replay's captions begin with (a row of -1 frees its clip);
    another P needs a new graph."""

    def __init__(self, model, frames, regions, **options):
        self.options, self.exclude, self._search = _held_exclusions(options)
        self._search, self.prefix = _held_prefix(model, self._search, frames.device)
        super().__init__(model, frames, regions)

    def _run(self):
        return self.model.beam_search(self.frames, self.regions, **self._search)


class StochasticBeamGraph(_SeededGraph):
    """hipGraph-captured `model.sample_without_replacement(frames, regions, n, temperature, **options)` for one batch shape: encoder
    and all max_words steps of stochastic beam search.  The seed is read from a device word, like SampleGraph's, so every replay
    draws afresh; a replay with seed s gives the bits of the eager call with seed=s.  options: min_len, no_repeat_ngram,
    return_threshold, fixed at capture.  Outputs are static buffers, valid until the next replay; nothing synchronises.
    exclude=Exclusions: kept as `graph.exclude`, as NBestBeamGraph keeps it.  prefix: a forced beginning is not covered in sampling
    without replacement; anything but None is a ValueError."""

    def __init__(self, model, frames, regions, n=5, temperature=1.0, **options):
        if options.get('prefix') is not None:
            from .beam import PrefixNotCovered
            raise PrefixNotCovered('prefix and StochasticBeamGraph: a forced beginning is not covered in stochastic beam search')
        self.n, self.temperature = n, temperature
        self.options, self.exclude, self._search = _held_exclusions(options)
        super().__init__(model, frames, regions)

    def _run(self):
        return self.model.sample_without_replacement(self.frames, self.regions, self.n, self.temperature, self.seed, **self._search)


class ConstrainedBeamGraph(_InferenceGraph):
    """hipGraph-captured `model.constrained_beam_search(frames, regions, constraints, **options)` for one batch shape and one shape
    of the constraint tensor -- (B, C, W) words or (B, C, W, P) phrases --, which is a static buffer like the inputs:
    `graph(frames, regions, constraints)` stages all three and replays; constraints are the packed int64 tensor or the per-clip lists
    (packed to the captured shape, by `pack_phrases` where that is 4-D; ValueError for another shape).  A replay returns the eager
    call's (ids, scores, lens[, met]), static buffers, and synchronises nothing.  prefix=: kept as `graph.prefix`, as
    NBestBeamGraph keeps it."""

    extra = 'cons'

    def __init__(self, model, frames, regions, constraints, **options):
        self.options, self.prefix = _held_prefix(model, options, frames.device)
        self.cons = self._packed(model, constraints, frames.device).clone()
        super().__init__(model, frames, regions)

    @staticmethod
    def _packed(model, constraints, device, phrases=None):
        """constraints as a tensor; phrases: whether lists are phrases (None: as `constrained_nbest` decides)"""
        from .beam import has_phrases, pack_constraints, pack_phrases
        if torch.is_tensor(constraints):
            return constraints
        if has_phrases(constraints) if phrases is None else phrases:
            return pack_phrases(constraints, model.decoder.vocab, device)
        return pack_constraints(constraints, model.decoder.vocab, device)

    def _run(self):
        return self.model.constrained_beam_search(self.frames, self.regions, self.cons, **self.options)

    def _fitted(self, constraints):
        """the constraints as a tensor of the captured shape: per-clip lists are packed and padded to it; ValueError otherwise"""
        cons = self._packed(self.model, constraints, self.cons.device, self.cons.dim() == 4)
        if not torch.is_tensor(constraints) and cons.dim() == self.cons.dim() and cons.shape[0] == self.cons.shape[0] and \
                all(a <= b for a, b in zip(cons.shape, self.cons.shape)):
            wide = torch.full_like(self.cons, -1)
            wide[tuple(slice(0, a) for a in cons.shape)] = cons
            cons = wide
        return self._like_captured(cons, 'constraints')


class EnsembleBeamGraph(_InferenceGraph):
    """hipGraph-captured `ensemble.beam_search(frames, regions, **options)` (ensemble.Ensemble) for one batch shape: every member's
    encoder and decode steps, one `beam_select_ens` per word, the ranking.  The graph holds addresses into EVERY member's arena and
    every member's train / eval mode: `valid_for` and the stale-arena error cover all of them.  A replay returns (ids, scores,
    lens), static buffers, and synchronises nothing.  exclude=Exclusions: kept as `graph.exclude`, as NBestBeamGraph keeps it;
    prefix=: kept as `graph.prefix`, likewise."""

    def __init__(self, ensemble, frames, regions, **options):
        self.ensemble = ensemble
        self.options, self.exclude, self._search = _held_exclusions(options)
        self._search, self.prefix = _held_prefix(ensemble.members[0], self._search, frames.device)
        super().__init__(ensemble.members[0], frames, regions, ensemble.members)

    def _run(self):
        return self.ensemble.beam_search(self.frames, self.regions, **self._search)


class EnsembleSampleGraph(_SeededGraph):
    """hipGraph-captured `ensemble.sample(frames, regions, n, temperature, **options)` (ensemble.Ensemble) for one batch shape: every
    member's encoder and decode steps and one `sample_ens` per word.  The seed is read from a device word, like SampleGraph's, so every
    replay draws afresh; a replay with seed s gives the bits of the eager call with seed=s.  options: top_k, top_p, min_len,
    no_repeat_ngram, return_kept, fixed at capture; exclude=Exclusions: kept as `graph.exclude`, the graph's own copy of the two
    tables, as SampleGraph keeps it.  Like EnsembleBeamGraph it holds addresses into EVERY member's arena and every member's train /
    eval mode.  prefix= and share_encoder= are refused as `Ensemble.sample` refuses them.  Outputs are static buffers, valid until the
    next replay; nothing synchronises."""

    def __init__(self, ensemble, frames, regions, n=1, temperature=1.0, **options):
        from .beam import check_ensemble_sample
        self.ensemble, self.n, self.temperature = ensemble, n, temperature
        check_ensemble_sample(ensemble.ops, ensemble.decoder, frames.shape[0], frames.device, n, temperature,
                              **{key: v for key, v in options.items() if key != 'return_kept'})      # (refused before the warm-up runs)
        self.options, self.exclude, self._draw = _held_exclusions(options)
        super().__init__(ensemble.members[0], frames, regions, ensemble.members)

    def _run(self):
        return self.ensemble.sample(self.frames, self.regions, self.n, self.temperature, self.seed, **self._draw)


class ConsensusBeamGraph(_InferenceGraph):
    """hipGraph-captured `consensus.consensus_search(model_or_ensemble, frames, regions, reward, **options)` for one batch shape: the
    beam search of a model or an `ensemble.Ensemble` with every beam kept, the `dlsg_cider_consensus` launch and the gathers that
    reorder the beams.  A replay returns (ids, expected, lens, order) -- static buffers, valid until the next replay -- and
    synchronises nothing.  Like EnsembleBeamGraph it holds every member's arena and train / eval mode."""

    def __init__(self, model_or_ensemble, frames, regions, reward, **options):
        self.search, self.reward, self.options = model_or_ensemble, reward, options
        members = _members(model_or_ensemble)
        super().__init__(members[0], frames, regions, members)

    def _run(self):
        from .consensus import consensus_search
        return consensus_search(self.search, self.frames, self.regions, self.reward, **self.options)


class ScoreGraph(_InferenceGraph):
    """hipGraph-captured `rescore.score_captions(scorer, frames, regions, ids, **options)` for one batch shape and one shape of
    `ids`, which is a static buffer like the inputs: `graph(frames, regions, ids)` stages all three and replays.  options:
    length_penalty, return_tokens, return_ranks, fixed at capture (lens are always counted from <end>).  A replay returns the eager
    call's tuple, static buffers, and synchronises nothing.  It holds the arena and train / eval mode of every member of the
    scorer."""

    extra = 'ids'

    def __init__(self, scorer, frames, regions, ids, **options):
        if 'lens' in options:
            raise ValueError('ScoreGraph counts the captions\' lengths from <end>: it takes no lens')
        self.scorer, self.options = scorer, options
        self.ids = ids.clone()
        members = _members(scorer)
        super().__init__(members[0], frames, regions, members)

    def _run(self):
        from .rescore import score_captions
        return score_captions(self.scorer, self.frames, self.regions, self.ids, **self.options)

    def _fitted(self, ids):
        return self._like_captured(ids, 'ids')


class RescoreBeamGraph(_InferenceGraph):
    """hipGraph-captured `rescore.rescore_search(model_or_ensemble, scorer, frames, regions, **options)` for one batch shape: the
    beam search of a model or an `Ensemble` with every beam kept, the scorer's teacher-forced passes over the beams, the
    `dlsg_seq_logprob` launch and the gathers that reorder the beams.  A replay returns (ids, scores, lens, order) -- static
    buffers, valid until the next replay -- and synchronises nothing.  It holds the arena and train / eval mode of every model
    involved, the searcher's and the scorer's."""

    def __init__(self, model_or_ensemble, scorer, frames, regions, **options):
        self.search, self.scorer, self.options = model_or_ensemble, scorer, options
        models = _members(model_or_ensemble)
        models += [m for m in _members(scorer) if not any(m is x for x in models)]
        super().__init__(models[0], frames, regions, models)

    def _run(self):
        from .rescore import rescore_search
        return rescore_search(self.search, self.scorer, self.frames, self.regions, **self.options)

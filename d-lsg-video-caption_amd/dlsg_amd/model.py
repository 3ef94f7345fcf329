"""Drop-in model surface of the hot path: CapGnnModel / CapBaseline1 with the reference's construction and
forward() signatures (models/model.py:25-43,94-107), state_dict layout and
`.decoder.decode_tokens` / `update_beam_size`, running on the HIP kernels of libdlsg_hip.so.

`forward` is one torch.autograd.Function around the hand-scheduled engine, so reference-style callers
(`loss.backward()` + torch.optim, DDP wrapping) work unchanged; `Trainer` is the fast path the benchmark uses:
fused ragged cross-entropy, hand-scheduled backward into a flat gradient arena, bucketed RCCL all-reduce that
overlaps the encoder backward, and one fused Adam kernel over the flat parameter arena.
"""
import collections
import contextlib
import math
import os
import random

import torch
import torch.nn as nn

from . import abi
from . import engine as E
from .graphs import capture_segments, stage, expand_rows, GreedyGraph, SampleGraph, BeamGraph, NBestBeamGraph  # noqa: F401
from .modules import CapGnnEncoder, Decoder, EncoderVisual

_ALIGN = 64  # floats: every parameter starts 256-B aligned inside the arena (vector loads need 16 B)


def _default_ops():
    from .hip import HipOps
    return HipOps()


class _ArenaModule(nn.Module):
    """A module whose parameters are views of ONE flat fp32 arena (plus a gradient arena of the same layout) and that launches
    kernels through an `ops` handle: shared by the generator models and the critic (gan.DiscV2)."""

    def __init__(self):
        super().__init__()
        self._ops_obj = None
        self._flat = None
        self._gflat = None
        self._offsets = None

    # ------------------------------------------------------------------ copy / pickle
    def __getstate__(self):
        """copy.deepcopy(model) / torch.save(model): the ctypes library handle and the `random` module cannot be pickled and
        the arenas are rebuilt on first use (flatten_parameters_ notices that the copied parameters are not its views)."""
        st = dict(self.__dict__)
        st['_ops_obj'] = None
        if 'rng' in st:
            st['rng'] = None
        for k in ('_flat', '_gflat', '_offsets', '_G'):
            st[k] = None
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        if 'rng' in st:
            self.rng = random

    # ------------------------------------------------------------------ kernels handle
    @property
    def ops(self):
        if self._ops_obj is None:
            self._ops_obj = _default_ops()   # raises when the HIP library / GPU is missing: no fallback
        return self._ops_obj

    def set_ops(self, ops):
        self._ops_obj = ops
        return self

    # ------------------------------------------------------------------ arenas
    def _arena_ok(self):
        if self._flat is None:
            return False
        for name, p in self.named_parameters():
            o = self._offsets[name]
            if p.device != self._flat.device or p.data_ptr() != self._flat.data_ptr() + 4 * o:
                return False
        return True

    def flatten_parameters_(self):
        """(Re)pack all parameters into one flat fp32 arena (views keep the nn.Parameter objects alive, so
        state_dict / load_state_dict / optimizers keep working) and allocate the matching gradient arena."""
        dec = getattr(self, 'decoder', None)
        if dec is not None and getattr(dec, '_owner', None) is None:
            import weakref
            object.__setattr__(dec, '_owner', weakref.ref(self))        # (a deep copy / unpickled model: see _HipModel.__setattr__)
        if self._arena_ok():
            return
        named = list(self.named_parameters())
        dev = named[0][1].device
        offsets, tot = {}, 0
        for name, p in named:
            offsets[name] = tot
            tot += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        flat = torch.zeros(tot, dtype=torch.float32, device=dev)
        for name, p in named:
            view = flat[offsets[name]:offsets[name] + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
        self._flat, self._offsets = flat, offsets
        self._gflat = torch.zeros(tot, dtype=torch.float32, device=dev)
        self._G = E.Grads(named, self._gflat, offsets)

    def grad_views(self):
        return self._G


class _HipModel(_ArenaModule):
    """Shared machinery of the generator models: arenas, ops handle, autograd bridge."""

    def __init__(self):
        super().__init__()
        self.rng = random          # scheduled-sampling coins come from Python's `random`, like layer.py:432
        self.seed_counter = 0
        self.fused_o2v = True
        # GEMM arithmetic: 'fp32' = exact fp32 MFMA everywhere; 'x3_bwd' = split-bf16 (3 bf16 MFMAs per product,
        # ~1e-5 relative error) for the backward products only; 'x3_all' = split-bf16 for forward and backward.
        self.gemm_precision = 'fp32'

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if name == 'decoder' and isinstance(value, nn.Module):
            # Decoder.forward called on its own (models/layer.py:394) launches through the owning model's binding and arena
            import weakref
            object.__setattr__(value, '_owner', weakref.ref(self))

    @staticmethod
    def check_kernel_limits(args, attended_rows, what):
        """The fused decoder-step kernels (csrc/decstep.hip: MAXW, MAXP) hold one batch row's vectors in LDS: widths up to
        2048, at most 72 attended rows per attention stream (72 = the longest clip the reference's positional
        encoding admits, sublayer.py:87; the baseline decoders attend over the frame nodes).  Checked at construction, with names, instead of an EINVAL
        from the first launch."""
        for k in ('query_hidden_size', 'decode_hidden_size', 'visual_hidden_size'):
            if getattr(args, k) > 2048:
                raise ValueError('%s = %d: the fused decoder step supports widths up to 2048' % (k, getattr(args, k)))
        if attended_rows > 72:
            raise ValueError('%s = %d: the fused decoder step attends over at most 72 rows per stream' % (what, attended_rows))

    stream_k_in_backward = True        # False: the backward's products stay on the tiled kernels
    sk_backward_cu_budget = 0          # > 0 (a Trainer with several ranks sets it): workgroups of the backward's stream-K launches,
                                       # the other CUs are left to the gradient all-reduces that run beside the backward

    def _gemm_flags(self, backward):
        from .hip import F_BF16X3, F_NOSK
        mode = self.gemm_precision
        assert mode in ('fp32', 'x3_bwd', 'x3_all'), mode
        fl = F_BF16X3 if (mode == 'x3_all' or (mode == 'x3_bwd' and backward)) else 0
        if backward and not self.stream_k_in_backward:
            fl |= F_NOSK
        return fl

    def _gemm_policy(self, backward):
        """what every dlsg_gemm call of the pass that starts here carries: arithmetic + stream-K flags, the stream-K CU budget"""
        ops = self.ops
        ops.extra_flags = self._gemm_flags(backward)
        ops.sk_cu_budget = self.sk_backward_cu_budget if backward else 0
        if backward:
            ops.grad_written = set()        # engine._accum_flag: the first product into a gradient block stores, later ones add

    merge_weight_grads = True          # see engine.tn_grouped
    _defer_ok = True                   # weight gradients may be collected and launched grouped ...
    _flush_at_buckets = False          # ... at the end of the backward (one rank) or at every gradient bucket (set by a Trainer that reduces buckets)

    def next_seed(self):
        self.seed_counter += 1
        return (0x5DEECE66D * self.seed_counter + 0xB) & 0xFFFFFFFFFFFF

    # ------------------------------------------------------------------ to be provided by subclasses
    seq_per_clip_ok = False            # several captions per clip on one encoder pass: CapGnnModel

    def _memories(self, frames, regions, training, seed, sv):
        """the class's encoder on B clips -> the list of (B, P, H) tensors its decoder attends over, one per attention stream:
        their row means form the global feature, and `_public` hands the first and the last back as obj / mot proposals"""
        raise NotImplementedError

    def _engine_backward(self, sv, dlogits_tm, dobj, dmot, dalpha_tm, training, seed, on_bucket=None, seq_per_clip=1):
        raise NotImplementedError

    def _public(self, x, proposals, alpha):
        """what forward() returns for the logits or ids x (models/model.py:94-107: the frames-only variants return no proposals)"""
        return x, 0, 0, 0

    # ------------------------------------------------------------------ engine schedules shared by the classes
    def _check_seq_per_clip(self, seq_per_clip, clips, captions):
        """seq_per_clip = n >= 1 captions per clip: `captions` (None at inference) must have n rows per clip"""
        n = int(seq_per_clip)
        if n != 1 and not self.seq_per_clip_ok:
            raise ValueError('seq_per_clip > 1 (several captions per clip on one encoder pass) is implemented for CapGnnModel '
                             'only, not for %s' % type(self).__name__)
        if n < 1:
            raise ValueError('seq_per_clip must be >= 1, not %r' % (seq_per_clip,))
        if captions is not None and captions.shape[0] != n * clips:
            raise ValueError('%d caption rows for %d clips with seq_per_clip = %d: expected %d (rows b*n .. b*n+n-1 belong to clip b)'
                             % (captions.shape[0], clips, n, n * clips))
        return n

    def _encoder_pass(self, frames, regions, training, seed, sv, n=1):
        """What every forward pass begins with: the forward GEMM policy, the class's encoder on the B clips, and its memories fanned
        out to the B*n rows the decoder runs on (row b*n + i = clip b; sv keeps the B-row tensors).
        -> (the memories of the B clips, of the B*n rows)"""
        ops = self.ops
        self._gemm_policy(False)
        if getattr(ops, 'colsum_defer', None) is not None:
            ops.colsum_defer = None         # (a backward that raised half-way must not leave the collector armed)
        frames = frames.contiguous().float()
        regions = regions.contiguous().float()
        props = self._memories(frames, regions, training, seed, sv)
        sv['frames'], sv['regions'], sv['enc_out'] = frames, regions, props
        mems = props
        if n != 1:
            # seq_per_clip = n > 1: the encoder ran on the B clips, the decoder runs on their B*n caption rows
            mems = [torch.empty((x.shape[0] * n,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device) for x in props]
            for x, y in zip(props, mems):
                ops.rows_repeat(x, y, n)
        sv['dec_gsrc'] = list(mems)
        return props, mems

    def _engine_forward(self, frames, regions, captions, L, coins, training, seed, sv, dev_coins=None, outputs=True, seq_per_clip=1):
        n = self._check_seq_per_clip(seq_per_clip, frames.shape[0], captions)
        props, mems = self._encoder_pass(frames, regions, training, seed, sv, n)
        s = E.dec_fwd(self.ops, self.decoder, list(mems), sv, captions, L, coins, training, seed, dev_coins)
        if not outputs:            # fused trainer: the loss reads the time-major logits in place
            return None
        logits, alpha = E.dec_outputs(self.ops, s, alpha=self.decoder.multi_modal)
        return logits, props[0], props[-1], alpha

    @torch.no_grad()
    def _greedy_ids(self, frames, regions, seed, L=None):
        """eval-mode greedy decoding (no dropout, so the seed is immaterial) -> (ids (B, L), the encoder's memories)"""
        L = self.decoder.max_words if L is None else L
        sv = {}
        self._engine_forward(frames, regions, None, L, [False] * L, False, seed, sv)
        return sv['dec']['IDS'][1:].t().contiguous(), sv['enc_out']

    # ------------------------------------------------------------------ public forward
    def forward(self, visual_feats, region_feats, caption, max_words=None, teacher_forcing_ratio=1.0, seq_per_clip=1):
        n = self._check_seq_per_clip(seq_per_clip, visual_feats.shape[0], caption)
        self.flatten_parameters_()
        dec = self.decoder
        infer = caption is None
        L = dec.max_words if max_words is None else max_words
        if infer and n != 1:
            raise ValueError('seq_per_clip > 1 needs captions; for several decoded captions per clip use sample() or beam_search()')
        if infer and dec.beam_size != 1:
            from .beam import beam_infer
            return beam_infer(self, visual_feats, region_feats)
        coins = self._draw_coins(L, infer, teacher_forcing_ratio)
        seed = self.next_seed()
        if infer:
            ids, props = self._greedy_ids(visual_feats, region_feats, seed, L)
            return self._public(ids, props, [])
        params = [p for _, p in self.named_parameters()]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            out = _ModelFn.apply(self, visual_feats, region_feats, caption, L, coins, seed, n, *params)
        else:
            with torch.no_grad():
                out = self._engine_forward(visual_feats, region_feats, caption, L, coins, self.training, seed, {}, seq_per_clip=n)
        return self._public(out[0], out[1:3], out[3])

    def sample(self, visual_feats, region_feats, n=1, temperature=1.0, seed=None, share_encoder=False, top_k=0, top_p=1.0,
               min_len=0, no_repeat_ngram=0, return_kept=False, exclude=None, prefix=None):
        raise NotImplementedError('sampled decoding (self-critical training) is implemented for CapGnnModel only')

    def beam_search(self, visual_feats, region_feats, beam_size=None, n_best=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0,
                    num_groups=1, diversity_penalty=0.0, exclude=None, prefix=None):
        """The n_best (default: all) of `beam_size` (default: the decoder's, at most 8) beams per clip, entirely on the device:
        (ids (B, n, L) int64 padded with <end>, scores (B, n) float32 = log-prob / len^length_penalty in descending order, lens
        (B, n) int64 counting the <end>).  no_repeat_ngram = g > 0: no caption repeats a g-gram; min_len: at least that many words
        before <end>.  With the options off, row 0 is `model(frames, regions, None)` padded with <end> (`beam.beam_nbest`).
        num_groups = G > 1: diverse beam search -- G groups of beam_size / G beams, chosen in turn at every word; a word that
        earlier groups chose at that step costs a later group `diversity_penalty` per choice (inf: excluded).  scores do not
        contain the penalty.  exclude: the `Exclusions` `dlsg_amd.pack_exclusions` makes -- words and phrases no caption may contain,
        `<unk>`, bad endings, for all clips or per clip; a banned word takes log-prob -inf, nothing is renormalised (not together
        with num_groups > 1).  prefix: how every caption begins -- the (B, P) int64 tensor `dlsg_amd.pack_prefix` makes (-1 ends a
        clip's prefix; lengths may differ) or the per-clip list it takes: the words are forced whatever the bans say, the search goes
        on behind them as if it had chosen them (bans, min_len and exclusions see the prefix; the caller's own words are not checked
        against `exclude`), scores include their log-probs and lens count them (not together with num_groups > 1).
        Nothing synchronises with the host, so call `model.ops.check_persistent()` where the ids are read back."""
        from .beam import beam_search
        return beam_search(self, visual_feats, region_feats, beam_size, n_best=n_best, length_penalty=length_penalty,
                           no_repeat_ngram=no_repeat_ngram, min_len=min_len, num_groups=num_groups, diversity_penalty=diversity_penalty,
                           exclude=exclude, prefix=prefix)

    def sample_without_replacement(self, visual_feats, region_feats, n=5, temperature=1.0, seed=None, min_len=0, no_repeat_ngram=0,
                                   return_threshold=False, exclude=None, prefix=None):
        """n (at most 8) DISTINCT captions per clip, an exact ordered sample without replacement from softmax(logits /
        temperature) by stochastic beam search, entirely on the device: (ids (B, n, L) int64 padded with <end>, logp (B, n) float32
        the captions' log-probabilities, lens (B, n) int64 counting the <end>), rows in sampling order -- row 0 is distributed as
        one ordinary sample.  min_len, no_repeat_ngram as in `sample`: the model is renormalised over the words they leave.
        return_threshold=True (n at most 7) adds (gumbel (B, n) float64, kappa (B,) float64) for `dlsg_amd.importance_weights`.
        exclude: the `Exclusions` of `dlsg_amd.pack_exclusions`, as in `beam_search` -- but here the model is renormalised over the
        words the exclusions leave, like the other two bans, and the sample is one without replacement from that model.
        seed None draws the model's next seed, a given seed reproduces the draw.  The decode runs in eval mode whatever
        `self.training` is (`beam.stochastic_nbest`); nothing synchronises with the host.
        prefix: a forced beginning is not covered here; anything but None is a ValueError."""
        from .beam import stochastic_nbest
        return stochastic_nbest(self, visual_feats, region_feats, n=n, temperature=temperature, seed=seed, min_len=min_len,
                                no_repeat_ngram=no_repeat_ngram, return_threshold=return_threshold, exclude=exclude, prefix=prefix)

    def constrained_beam_search(self, visual_feats, region_feats, constraints, beam_size=None, n_best=None, length_penalty=0.0,
                                no_repeat_ngram=0, min_len=0, return_met=False, exclude=None, prefix=None):
        """`beam_search` whose captions must contain given words (lexically constrained beam search by dynamic beam allocation).
        constraints: per clip a list of constraints, each a word, a word id or a list of alternatives of which one must appear
        (at most 8 constraints of 8 alternatives), or the (B, C, W) int64 device tensor `dlsg_amd.pack_constraints` makes of them.
        Returns (ids, scores, lens) as `beam_search`, a clip's rows ordered by the number of constraints met, most first, then by
        score; return_met=True adds that number (B, n) int64.  Row 0 meets every constraint that has a word the model can emit; a
        caption ends only with all of them met (`beam.constrained_nbest`).  Nothing synchronises with the host.
        Multi-word phrases: lists in which a string holds whitespace ("hot dog"; a constraint is then a phrase or a list of
        alternative phrases, a phrase a string, a tuple of words or ids, or one word, at most 4 words), or the (B, C, W, P) tensor
        `dlsg_amd.pack_phrases` makes, require phrases as contiguous words; met then counts the constraints with a phrase in the row
        (`dlsg_amd.phrases_met`).  C_b phrase constraints of up to n words need C_b * n + 1 <= max_words; with no_repeat_ngram the
        next word of a phrase can be banned, the search is then best effort and a beam that cannot finish runs to max_words.
        exclude: exclusions are not covered here; anything but None is a ValueError.  prefix: a forced beginning as in
        `beam_search`; a prefix word meets a constraint or advances a phrase, and met counts it."""
        from .beam import constrained_nbest
        return constrained_nbest(self, visual_feats, region_feats, constraints, n_best=n_best, length_penalty=length_penalty,
                                 no_repeat_ngram=no_repeat_ngram, min_len=min_len, beam_size=beam_size, return_met=return_met,
                                 exclude=exclude, prefix=prefix)

    def score(self, visual_feats, region_feats, ids, **options):
        """The log-probability of GIVEN captions under this model: `rescore.score_captions(self, ...)` -- ids (B, L) or (B, n, L)
        int64, <end>-padded; options lens, length_penalty, return_tokens, return_ranks.  -> (scores, lens[, tok_lp][, tok_rank]).
        One teacher-forced pass without dropout and one `seq_logprob` launch; rescoring the model's own `beam_search` output
        gives that search's scores and lens."""
        from .rescore import score_captions
        return score_captions(self, visual_feats, region_feats, ids, **options)

    def _draw_coins(self, L, infer, tf_ratio):
        # reference draws one coin per step only when not inferring (layer.py:432)
        if infer:
            return [False] * L
        return [self.rng.random() < tf_ratio for _ in range(L)]


class _ModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, frames, regions, captions, L, coins, seed, seq_per_clip, *params):
        sv = {}
        training = model.training
        outs = model._engine_forward(frames, regions, captions, L, coins, training, seed, sv, seq_per_clip=seq_per_clip)
        ctx.model, ctx.sv, ctx.seed, ctx.training, ctx.seq_per_clip = model, sv, seed, training, seq_per_clip
        ctx.nparams = len(params)
        return outs

    @staticmethod
    def backward(ctx, dlogits, dobj, dmot, dalpha):
        model, ops = ctx.model, ctx.model.ops
        Bn, L, V = dlogits.shape
        dl_tm = torch.empty(L, Bn, V, dtype=torch.float32, device=dlogits.device)
        ops.permute_tb(dlogits.contiguous(), dl_tm)          # (B,L,V) -> (L,B,V)
        da_tm = None
        if dalpha is not None and dalpha.numel() > 0:
            da_tm = torch.empty(L, Bn, dalpha.shape[-1], dtype=torch.float32, device=dlogits.device)
            ops.permute_tb(dalpha.contiguous(), da_tm)
        model._engine_backward(ctx.sv, dl_tm, dobj, dmot, da_tm, ctx.training, ctx.seed, seq_per_clip=ctx.seq_per_clip)
        G = model.grad_views()
        grads = []
        for name, p in model.named_parameters():
            grads.append(G[name].clone() if (name not in model.unused_parameters and p.requires_grad) else None)
        ctx.sv = None
        return (None,) * 8 + tuple(grads)


class CapGnnModel(_HipModel):
    """models/model.py:25-43.  forward(visual_feats, region_feats, caption, max_words=None,
    teacher_forcing_ratio=1.0, seq_per_clip=1) -> (outputs, obj_proposals, motion_proposals, alpha_all).

    seq_per_clip = n > 1: `caption` holds n captions for each of the B clips (rows b*n .. b*n+n-1 belong to clip b, the layout
    `sample` returns).  The encoder runs once on the B clips, its proposals are fanned out to the B*n caption rows
    (`rows_repeat`) and the decoder runs on those; the backward folds the caption rows' gradients back onto the clips
    (`clip_fold`) before the encoder's backward, which runs on B rows.  outputs and alpha_all have B*n rows, the proposals B.
    Dropout: the encoder's masks are keyed by the clip row 0..B-1, so the n captions of a clip see the same encoder masks;
    decoder and word dropout stay keyed by the B*n caption rows.  Under one seed these are the masks of
    `sample(..., share_encoder=True)`, not those of a pass over the clips repeated n times."""

    @property
    def unused_parameters(self):
        """constructed by the reference but never used in forward: they get no gradient;
        with num_obj < 5 the graph is skipped (layer.py:181-182) and obj_visual_norm is unused too."""
        names = ['encoder.obj_encoder.att_l2l_norm.weight', 'encoder.obj_encoder.att_l2l_norm.bias',
                 'encoder.motion_encoder.att_l2l_norm.weight', 'encoder.motion_encoder.att_l2l_norm.bias',
                 'decoder.context_layernorm.weight', 'decoder.context_layernorm.bias']
        if not self.encoder.obj_encoder.has_obj:
            for e in ('obj_encoder', 'motion_encoder'):
                names += ['encoder.%s.obj_visual_norm.1.weight' % e, 'encoder.%s.obj_visual_norm.1.bias' % e]
        return frozenset(names)

    seq_per_clip_ok = True

    def __init__(self, args, vocab):
        super().__init__()
        self.check_kernel_limits(args, args.num_proposals, 'num_proposals')
        self.use_visual_gan = args.use_visual_gan
        self.encoder = CapGnnEncoder(args)
        self.decoder = Decoder(args, vocab, multi_modal=True)

    def update_beam_size(self, beam_size):
        self.decoder.update_beam_size(beam_size)

    def load_encoder(self, model, model_path):
        """models/model.py:45-53: load `model_path` into `model`, graft its `.encoder` and `.decoder.word_embed` into this
        model and freeze the word embedding.  The grafted modules are shared objects, as in the reference; this model's
        arenas are re-packed around them on the next use (the donor is not meant to be used afterwards, run_gun.py keeps
        only the grafted model).  `Trainer` leaves parameters with `requires_grad == False` untouched."""
        if model_path is not None:
            model.load_state_dict(torch.load(model_path, map_location=next(self.parameters()).device))
        self.encoder = model.encoder
        self.decoder.word_embed = model.decoder.word_embed
        for param in self.decoder.word_embed.parameters():
            param.requires_grad = False
        self._flat = None                   # parameters changed identity: re-pack

    # ------------------------------------------------------------------ engine schedules
    def _encode(self, frames, regions, training, seed, sv):
        """CapGnnEncoder.forward (models/model.py:69-73).  The frame nodes of both streams are computed first (the motion
        stream's come out of the BiLSTM pre-encoder), then the object->frame graph of BOTH streams runs as one launch."""
        ops, enc = self.ops, self.encoder
        B, T, F = frames.shape
        A = enc.a_feature_size
        f2 = frames.view(B * T, F)
        # the object stream's visual_embed (independent of everything else) rides in the pre-encoder's first launch
        pre, extra = {}, []
        oe = enc.obj_encoder
        if oe.use_embed:
            pre['encoder.obj_encoder'] = torch.empty(B * T, oe.visual_embed.weight.shape[0], dtype=torch.float32, device=frames.device)
            extra.append((f2[:, :A], oe.visual_embed.weight, pre['encoder.obj_encoder'], oe.visual_embed.bias))
        mot_in = E.encvis_fwd(ops, enc.motion_pre_encoder, 'encoder.motion_pre_encoder', f2, B, T, sv, training, seed, extra=extra)
        E.tun_frames_multi(ops, [(enc.obj_encoder, 'encoder.obj_encoder', f2[:, :A]), (enc.motion_encoder, 'encoder.motion_encoder', mot_in)],
                           regions, sv, pre)
        # the region projections (the step's longest launch) go HERE, behind the frame path's matrix kernels, not first in the
        # step: directly behind the previous step's Adam -- 0.5 ms of pure memory traffic -- the same launch takes 11 % longer
        # (1 722 us against 1 555 back to back, tools/archive/sk_sequence_probe.py: the clock the chip holds, not the caches)
        ys = [None, None]
        if regions.shape[2] >= 5 and enc.obj_encoder.obj_embed.weight.shape == enc.motion_encoder.obj_embed.weight.shape:
            ys = E.region_projections(ops, [enc.obj_encoder, enc.motion_encoder], regions)
        E.tun_graph(ops, [(enc.obj_encoder, 'encoder.obj_encoder', ys[0]), (enc.motion_encoder, 'encoder.motion_encoder', ys[1])],
                    regions, sv, self.fused_o2v)
        obj, mot = E.tun_latent_multi(ops, [(enc.obj_encoder, 'encoder.obj_encoder', E.SITE_PSL_OBJ),
                                            (enc.motion_encoder, 'encoder.motion_encoder', E.SITE_PSL_MOT)], regions, sv, training, seed)
        return obj, mot

    def _memories(self, frames, regions, training, seed, sv):
        return list(self._encode(frames, regions, training, seed, sv))

    def _public(self, x, proposals, alpha):
        return x, proposals[0], proposals[-1], alpha

    def _engine_backward(self, sv, dlogits_tm, dobj, dmot, dalpha_tm, training, seed, on_bucket=None, seq_per_clip=1):
        ops, enc = self.ops, self.encoder
        n = int(seq_per_clip)
        self._gemm_policy(True)
        G = self._G
        ops.fill(self._gflat, 0.0)
        if self.merge_weight_grads and self._defer_ok:
            sv['tn_defer'] = []             # mid-size weight gradients of every module: launched together at the end
        collect = hasattr(ops, 'colsum_flush')
        if collect:
            ops.colsum_defer = []           # short column sums (LayerNorm / bias gradients): grouped launches (hip.py)
        frames, regions = sv['frames'], sv['regions']
        B, T, F = frames.shape
        H = self.decoder.visual_hidden_size
        dmems, dgfeat = E.dec_bwd(ops, self.decoder, sv, G, dlogits_tm, seed, training, dalpha_tm)

        def bucket(key):
            # a bucket's gradients must be complete when it is handed to the all-reduce: the weight gradients deferred so far
            # go out now, as one grouped launch per height (with one process nothing is reduced and they wait for the end)
            if on_bucket:
                if self._flush_at_buckets:
                    if sv.get('tn_defer'):
                        E.tn_grouped(ops, sv['tn_defer'])
                        sv['tn_defer'] = []
                    if collect:
                        ops.colsum_flush(keep_collecting=True)
                on_bucket(key)
        bucket('decoder')
        dob, dmo = dmems
        if n == 1:
            ops.mean_rows_bwd(dgfeat[:, :H], dob, accum=True)
            ops.mean_rows_bwd(dgfeat[:, H:], dmo, accum=True)
        else:
            # the decoder's backward ran on the B*n caption rows: one pass per stream folds a clip's n rows -- proposals'
            # gradient and the backward of their mean -- onto the clip, in a fixed order; the encoder's backward runs on B rows
            folded = []
            for i, dm in enumerate(dmems):
                dx = torch.empty((B,) + tuple(dm.shape[1:]), dtype=torch.float32, device=dm.device)
                ops.clip_fold(dm, dgfeat[:, i * H:(i + 1) * H], dx, n)
                folded.append(dx)
            dob, dmo = folded
        if dobj is not None:
            ops.copy2d(dobj.reshape(-1, H), dob.view(-1, H), accum=True)
        if dmot is not None:
            ops.copy2d(dmot.reshape(-1, H), dmo.view(-1, H), accum=True)
        f2 = frames.view(B * T, F)
        # the obj_embed weight gradients of the two streams (the deepest products of the step) are issued together at the
        # end, so the two small TUN buckets (12 MB each) are reduced last; the 151 MB motion_pre_encoder bucket still
        # travels under the object stream's backward
        deep = []
        mot, obj = (enc.motion_encoder, 'encoder.motion_encoder'), (enc.obj_encoder, 'encoder.obj_encoder')
        # both streams' LatentPSL / obj_visual_norm backward first, so that the object->frame graph of BOTH streams runs its
        # backward as one launch per pass (2 x 64 clips: two object chunks per clip instead of four)
        E.tun_bwd_head_multi(ops, [(mot[0], mot[1], dmo), (obj[0], obj[1], dob)], regions, sv, G, training, seed)
        E.tun_graph_bwd(ops, [mot, obj], regions, sv, G)
        dmot_in = E.tun_bwd_tail(ops, mot[0], mot[1], regions, sv, G, defer_dw=deep)
        E.encvis_bwd(ops, enc.motion_pre_encoder, 'encoder.motion_pre_encoder', f2, B, T, sv, G, dmot_in, training, seed)
        bucket('encoder.motion_pre_encoder')
        E.tun_bwd_tail(ops, obj[0], obj[1], regions, sv, G, defer_dw=deep)
        if on_bucket and self._flush_at_buckets and len(deep) == 2:
            # several ranks: what trails the backward is exposed.  Everything of the two graph modules but their obj_embed weights
            # is complete here and travels under the deep weight-gradient products (1.8 ms); those run one stream at a time, so the
            # motion stream's 8 MB ride under the object stream's product and only obj_encoder.obj_embed.weight (8 MB of the 25)
            # is reduced after the last launch of the backward.  (One rank: the two products share ONE launch.)
            bucket(('encoder.motion_encoder:rest', 'encoder.obj_encoder:rest'))
            for item, (_, pfx) in zip(deep, (mot, obj)):
                E.gemm_tn_deep(ops, [item], frames)
                on_bucket(pfx + ':obj_embed.weight')
            if collect:
                ops.colsum_flush()
            return
        E.gemm_tn_deep(ops, deep, frames)
        if 'tn_defer' in sv:
            E.tn_grouped(ops, sv.pop('tn_defer'))
        if collect:
            ops.colsum_flush()
        if on_bucket:
            on_bucket(('encoder.motion_encoder', 'encoder.obj_encoder'))

    @torch.no_grad()
    def sample(self, visual_feats, region_feats, n=1, temperature=1.0, seed=None, share_encoder=False, top_k=0, top_p=1.0,
               min_len=0, no_repeat_ngram=0, return_kept=False, exclude=None, prefix=None):
        """Draw n captions per clip from softmax(logits / temperature) (self-critical training; temperature 0 is greedy).
        Returns (ids (B*n, L) int64, logp (B*n, L) float32 log-probabilities of the drawn words, lens (B*n,) int64: first
        <end> position + 1, else L); clip b's samples are rows b*n .. b*n + n - 1.  The clips are repeated n times before the
        encoder (it runs on B*n rows, with their own dropout rows).  Dropout follows `self.training`.  seed None draws the next
        seed of the model's sequence; a given seed reproduces the draw -- and the dropout masks of a train step on the same
        rows with that seed, so the sampled words are on-policy for it.
        share_encoder=True: the encoder runs once, on the B clips, and only the sampled decoding runs on B*n rows (the proposals
        are fanned out with `rows_repeat`).  The encoder's dropout masks are then keyed by the clip row 0..B-1 -- the n samples
        of a clip share them -- while decoder and word dropout stay keyed by the B*n caption rows: these are the masks of a train
        pass `forward(..., seq_per_clip=n)` / `Trainer.step(..., seq_per_clip=n)` with the same seed, so the draw is on-policy for
        that pass; they are not the masks of the unshared draw, which is why sharing is opt-in.
        Sampling controls, applied in this order at every word (`dlsg_sample_filter_embed`): min_len -- no <end> before that many
        words; no_repeat_ngram = g > 0 -- no caption repeats a g-gram; top_k > 0 -- only the k likeliest words (ties at the k-th
        kept); top_p < 1 -- of those, the smallest set of likeliest words whose probability reaches top_p.  logp is then the
        log-probability under the truncated, renormalised distribution.  A word's Gumbel noise does not depend on the controls.
        return_kept=True adds a fourth value, (B*n, L) int32: how many words each draw chose from (needs a control on).
        exclude: the `Exclusions` of `dlsg_amd.pack_exclusions` -- words and phrases no sample may contain, `<unk>`, bad endings, for
        all clips (shared) or per clip (per_clip (B, NC, P): the B clips, not their B*n rows).  A word is banned for a row when it
        would complete an entry whose earlier words are the row's last words; the bans join those of min_len and no_repeat_ngram,
        come before top_k and top_p and renormalise like them (`dlsg_sample_excl_embed`; `beam_search` does not renormalise).  It is
        a control of its own: the others may be off.  Words behind a row's first <end> are not part of its caption.  None, or
        two empty tables, launches what the call launched without the keyword.
        prefix: how the samples begin -- the (B, P) int64 tensor `dlsg_amd.pack_prefix` makes, for the B clips, not their B*n rows
        (-1 ends a clip's prefix; lengths may differ), or the per-clip list it takes.  The n rows of clip b hold prefix[b, t] at the
        steps t < p_b whatever the controls say, and draw from p_b on as they would behind these words: the n-gram ban, min_len and
        the exclusions see the prefix (the caller's own words are not checked against `exclude`).  logp at a forced position is the
        word's plain log-probability under softmax(logits / temperature) -- no control applied, at temperature 0 under the
        untempered softmax: what the plain sampler reports for a word it draws -- so the sum from p_b on is the conditional
        log-probability; kept is 1 there.  One `sample_force_prefix` launch behind the step of each of the first P words; None, or
        P == 0, launches what the call launched without the keyword."""
        L = self.decoder.max_words
        filtered = E.check_sample_options(L, top_k, top_p, min_len, no_repeat_ngram, self.decoder.vocab_size)
        excluding = E.sample_exclusions(exclude, visual_feats.shape[0], visual_feats.device, L, self.decoder.vocab_size) is not None
        if excluding:
            from .beam import require_excl_step
            require_excl_step(self.ops, 'sample_excl_embed')
        if prefix is not None:
            from .beam import check_prefix, require_prefix_step
            prefix = check_prefix(prefix, visual_feats.shape[0], visual_feats.device, L, self.decoder.vocab)
            if prefix is not None:
                require_prefix_step(self.ops, 'sample_force_prefix')
        if return_kept and not (filtered or excluding):
            raise ValueError('return_kept needs one of top_k, top_p, min_len, no_repeat_ngram, exclude switched on')
        self.flatten_parameters_()
        if seed is None:
            seed = self.next_seed()
        per_clip = int(n)               # rows of one clip, whichever form runs
        if not share_encoder:           # the clips repeated n times, then the shared form with one row per clip
            visual_feats, region_feats, n = expand_rows(visual_feats, n), expand_rows(region_feats, n), 1
        sv = {}
        _, mems = self._encoder_pass(visual_feats, region_feats, self.training, seed, sv, int(n))
        s = E.dec_sample(self.ops, self.decoder, list(mems), sv, L, self.training, seed, temperature, top_k=top_k, top_p=top_p,
                         min_len=min_len, no_repeat_ngram=no_repeat_ngram, exclude=exclude if excluding else None,
                         rows_per_clip=per_clip, prefix=prefix)
        out = s['IDS'][1:].t().contiguous(), s['LOGP'].t().contiguous(), s['LENS']
        return out + (s['KEPT'].t().contiguous(),) if return_kept else out


class CapBaseline1(_HipModel):
    """models/model.py:94-107: frames-only variant, EncoderVisual(baseline) + Decoder(baseline)."""
    unused_parameters = frozenset(['decoder.context_layernorm.weight', 'decoder.context_layernorm.bias'])

    def __init__(self, args, vocab):
        super().__init__()
        self.check_kernel_limits(args, args.max_frames, 'max_frames (baseline decoders attend over the frame nodes)')
        self.use_visual_gan = args.use_visual_gan
        self.encoder = EncoderVisual(args, baseline=True)
        self.decoder = Decoder(args, vocab, multi_modal=False, baseline=True)

    def update_beam_size(self, beam_size):
        self.decoder.update_beam_size(beam_size)

    def _memories(self, frames, regions, training, seed, sv):
        B, T, F = frames.shape
        enc = E.encvis_fwd(self.ops, self.encoder, 'encoder', frames.view(B * T, F), B, T, sv, training, seed)
        return [enc.view(B, T, -1)]

    def _engine_backward(self, sv, dlogits_tm, dobj, dmot, dalpha_tm, training, seed, on_bucket=None, seq_per_clip=1):
        ops = self.ops
        self._gemm_policy(True)
        G = self._G
        ops.fill(self._gflat, 0.0)
        frames = sv['frames']
        B, T, F = frames.shape
        dmems, dgfeat = E.dec_bwd(ops, self.decoder, sv, G, dlogits_tm, seed, training, None)
        denc = dmems[0]
        ops.mean_rows_bwd(dgfeat, denc, accum=True)
        E.encvis_bwd(ops, self.encoder, 'encoder', frames.view(B * T, F), B, T, sv, G, denc.view(B * T, -1), training, seed)
        if on_bucket:
            on_bucket(('decoder', 'encoder'))


class CapBaselineModel(_HipModel):
    """models/model.py:76-91: CapGnnEncoder(baseline=True) -- the TUN streams return their frame nodes instead of latent
    proposals -- and a baseline Decoder (one attention) on the motion stream only.  The reference also runs the object
    stream and drops its output; that work is skipped here (no output or gradient depends on it), and the 24 parameters
    the reference leaves without a gradient (object stream, LatentPSL of the motion stream, linear_baseline, ...) are
    reported as unused."""

    @property
    def unused_parameters(self):
        names = ['decoder.context_layernorm.weight', 'decoder.context_layernorm.bias', 'linear_baseline.weight',
                 'linear_baseline.bias']
        for n, _ in self.encoder.obj_encoder.named_parameters():
            names.append('encoder.obj_encoder.' + n)
        me = 'encoder.motion_encoder.'
        names += [me + 'att_l2l_norm.weight', me + 'att_l2l_norm.bias', me + 'v2l_layer.theta',
                  me + 'v2l_layer.out_norm.1.weight', me + 'v2l_layer.out_norm.1.bias']
        if not self.encoder.motion_encoder.has_obj:
            names += [me + 'obj_visual_norm.1.weight', me + 'obj_visual_norm.1.bias']
        return frozenset(names)

    def __init__(self, args, vocab):
        super().__init__()
        self.check_kernel_limits(args, args.max_frames, 'max_frames (baseline decoders attend over the frame nodes)')
        self.use_visual_gan = args.use_visual_gan
        self.encoder = CapGnnEncoder(args, baseline=True)
        self.linear_baseline = nn.Linear(args.visual_hidden_size * 2, args.visual_hidden_size)
        self.decoder = Decoder(args, vocab, multi_modal=False, baseline=True)

    def update_beam_size(self, beam_size):
        self.decoder.update_beam_size(beam_size)

    def _memories(self, frames, regions, training, seed, sv):
        ops, enc = self.ops, self.encoder
        B, T, F = frames.shape
        f2 = frames.view(B * T, F)
        mot_in = E.encvis_fwd(ops, enc.motion_pre_encoder, 'encoder.motion_pre_encoder', f2, B, T, sv, training, seed)
        mot = E.tun_fwd(ops, enc.motion_encoder, 'encoder.motion_encoder', mot_in, regions, sv, training, seed,
                        E.SITE_PSL_MOT, self.fused_o2v)
        return [mot.view(B, T, -1)]

    def _engine_backward(self, sv, dlogits_tm, dobj, dmot, dalpha_tm, training, seed, on_bucket=None, seq_per_clip=1):
        ops, enc = self.ops, self.encoder
        self._gemm_policy(True)
        G = self._G
        ops.fill(self._gflat, 0.0)
        frames, regions = sv['frames'], sv['regions']
        B, T, F = frames.shape
        dmems, dgfeat = E.dec_bwd(ops, self.decoder, sv, G, dlogits_tm, seed, training, None)
        dmo = dmems[0]
        ops.mean_rows_bwd(dgfeat, dmo, accum=True)
        dmot_in = E.tun_bwd(ops, enc.motion_encoder, 'encoder.motion_encoder', regions, sv, G, dmo, training, seed)
        E.encvis_bwd(ops, enc.motion_pre_encoder, 'encoder.motion_pre_encoder', frames.view(B * T, F), B, T, sv, G, dmot_in,
                     training, seed)
        if on_bucket:
            on_bucket(('decoder', 'linear_baseline', 'encoder.obj_encoder', 'encoder.motion_pre_encoder', 'encoder.motion_encoder'))


def _h2d(values, dtype, device):
    from .hip import host_to_device
    return host_to_device(values, dtype, device)


def _copy_h2d(dst, values):
    from .hip import copy_to_device
    copy_to_device(dst, values)


# ================================================================================================ fast training path
def ss_epsilon(epoch, ss_factor=20):
    """scheduled-sampling probability, run_gun.py:136"""
    return max(0.6, ss_factor / (ss_factor + math.exp(epoch / ss_factor)))


def multistep_lr(epoch, base_lr=1.6e-4, milestones=(4, 7), gamma=0.5):
    """learning rate of `MultiStepLR(optimizer, milestones=[4, 7], gamma=0.5)` (run_gun.py:94-95) at the start of `epoch`;
    assign it to `Trainer.lr` (the replayed graphs read the rate from device memory every step)."""
    return base_lr * gamma ** sum(1 for m in milestones if epoch >= m)


class Trainer(object):
    """The reference's per-iteration use of the model (run_gun.py:153-160,181-198,233-234) as one fused schedule:
    forward -> ragged CrossEntropy (mean over sum(cap_lens) rows) -> backward -> [RCCL all-reduce] -> Adam.

    Data parallel: one process per GPU; every rank runs its own shard, gradients are summed with
    torch.distributed all_reduce (RCCL over xGMI) bucket by bucket as the backward finishes each module group and
    divided by world size inside the Adam kernel (DDP mean-of-means semantics, run_gun.py:63-64).

    use_graphs: capture the step into hipGraphs (one per backward bucket, so the collectives stay between graph
    replays and still overlap the rest of the backward).  The step is ~1200 kernel launches, i.e. launch-bound from
    Python; replaying removes the host from the loop.  Everything that changes between steps is read from device
    memory: inputs (static buffers), the dropout seed, the scheduled-sampling coins, the Adam bias corrections."""

    def __init__(self, model, lr=1.6e-4, betas=(0.5, 0.9), eps=1e-8, process_group=None, world_size=1, use_graphs=False,
                 device_coins=None, graph_fallback=False, comm='auto', check_every=100, rehearse_ranks=0, max_grad_norm=None,
                 clip_grad_value=None, label_smoothing=0.0, teacher=None, distill_weight=0.0, weight_decay=0.0,
                 decoupled_weight_decay=True, decay_filter=None, ema_decay=None, ema_warmup=False):
        """comm: how the gradient buckets are summed over ranks.
          'rccl'  -- librccl through the C ABI (dlsg_allreduce_bucket) on a side stream forked by an event: the collectives
                     are part of the captured step, so one iteration is ONE hipGraph replay and a bucket's all-reduce runs
                     under the backward that follows it;
          'torch' -- torch.distributed.all_reduce(async_op=True) issued by the host between hipGraph segments (any backend:
                     this is what the CPU / gloo tests run);
          'auto'  -- 'rccl' when the model lives on a GPU, else 'torch'.
        rehearse_ranks: N > 1 with world_size == 1 runs, on ONE GPU, exactly the step a rank of an N-rank job runs -- the
          multi-rank kernel choices of `_use_multi_rank_schedule`, weight gradients flushed at every bucket, every bucket handed
          to the communicator (world 1: the all-reduce is the identity, Adam's 1 / world stays 1) -- so that this schedule can be
          checked against the oracle and timed where only one device exists (tests/test_gpu_bench_parity.py, bench.py's
          `dp_schedule_world1`).  `rehearse_cotenant` adds the chip-sharing a real all-reduce brings.
        max_grad_norm: clip the gradient to this global 2-norm before Adam (torch.nn.utils.clip_grad_norm_), on the device and as
          part of the step -- captured with it, no host read.  The norm is that of the gradient Adam applies: over the trainable
          ranges, after the all-reduce, of the mean over the ranks; every rank reduces the same bits in the same order, so all
          ranks clip -- or skip -- alike without a collective of their own.  float('inf') clips nothing but still reports and skips.
        clip_grad_value: clamp every element of that gradient to +-value instead (clip_grad_value_).  At most one of the two.
          With either set, `last_grad_norm` is a 0-d device view of the last step's norm (float() reads it, and synchronises) and a
          step whose gradient holds an inf or a NaN updates nothing -- weights and both moments keep their bits -- and adds one
          to the device counter `skipped_steps`.  `t` advances on a skipped step all the same: the bias corrections are sent
          from the host before the outcome exists, so the step after a skipped one uses corrections one step further on.
          With both None the step issues exactly the launches it issued before these options existed.
        label_smoothing: eps in [0, 1) -- the loss is the CrossEntropy against (1 - eps) * onehot + eps / V at every counted
          position, `torch.nn.CrossEntropyLoss(label_smoothing=eps)`.
        teacher, distill_weight: word-level knowledge distillation (Kim & Rush 2016).  teacher is an `Ensemble`, or one model
          (wrapped as `Ensemble([model])`), of the trained model's vocabulary and device; distill_weight = alpha in (0, 1] is its
          share of the target row: (1 - alpha) * (the hard or smoothed target) + alpha * q, q the members' word distributions
          combined by the ensemble's weights and mode ('logprob': renormalised).  Every step runs the members' teacher-forced
          forward passes without dropout first (`Ensemble.teacher_logits`; their `.training` flags, parameters and `.grad` are
          left alone: the teacher gets no gradient, no Adam moments and no all-reduce, and each rank runs it on its own shard),
          then the student, then one `dlsg_ce_ragged_soft` launch in place of the CrossEntropy's -- all inside the captured
          step with use_graphs.  The teacher is ALWAYS teacher-forced on the ground truth, also when tf_ratio < 1 feeds the
          student its own words at some positions (the usual word-level recipe: q is the teacher's answer to the reference
          prefix).  With either option on, `step` returns the mixed loss and `last_loss_parts` is a 3-float device view {mixed
          loss, plain NLL of the targets, CrossEntropy against q} of the last step -- the NLL stays comparable with a run
          without the options.  seq_weights, seq_per_clip, extra_dlogits and clipping compose as before.  With the defaults
          (0.0, None, 0.0) the step issues exactly the launches it issued before these options existed.
        weight_decay, decoupled_weight_decay: wd >= 0, applied inside Adam's launch (dlsg_adamw_ema).  Decoupled (the default,
          torch.optim.AdamW): p *= 1 - lr * wd in front of the update, with the plain lr.  Not decoupled (torch.optim.Adam's
          weight_decay, L2): g += wd * p behind the clip, so `last_grad_norm` never holds the decay term.
        decay_filter: None decays every trainable parameter; else a callable (name, parameter) -> bool, e.g. lambda n, p: p.ndim > 1
          for "no decay on biases and LayerNorm gains".  Parameters in `model.unused_parameters` are never decayed (torch skips
          parameters without a gradient), frozen ones are outside the update altogether.
        ema_decay: d in (0, 1) keeps `ema`, an fp32 arena laid out as the weights' (a copy of them at first), and moves it in the
          same launch: ema += (1 - d) * (p_new - ema).  ema_warmup: d_t = min(d, (1 + t) / (10 + t)), t the step count, which
          advances on a skipped step as the bias corrections do.  A skipped step (non-finite gradient, time-out word) leaves `ema`
          as it is.  `averaged()`, `ema_state_dict()` and `load_ema_state_dict()` use the average.
          With (0.0, None) the step issues exactly the launches it issued before these options existed."""
        assert comm in ('auto', 'rccl', 'torch'), comm
        if not float(weight_decay) >= 0.0 or math.isinf(float(weight_decay)):
            raise ValueError('weight_decay must be a finite number >= 0, not %r' % (weight_decay,))
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError('ema_decay must be in (0, 1), not %r' % (ema_decay,))
        if ema_warmup and ema_decay is None:
            raise ValueError('ema_warmup needs ema_decay')
        if decay_filter is not None and not callable(decay_filter):
            raise ValueError('decay_filter must be None or a callable (name, parameter) -> bool')
        self.weight_decay, self.decoupled_weight_decay = float(weight_decay), bool(decoupled_weight_decay)
        self.decay_filter = decay_filter
        self.ema_decay, self.ema_warmup = None if ema_decay is None else float(ema_decay), bool(ema_warmup)
        self.ema = None
        self._decay_tabs = {}
        self._averaging = False
        eps_ls, alpha = float(label_smoothing), float(distill_weight)
        if not 0.0 <= eps_ls < 1.0:
            raise ValueError('label_smoothing must be in [0, 1), not %r' % (label_smoothing,))
        if not 0.0 <= alpha <= 1.0:
            raise ValueError('distill_weight must be in [0, 1], not %r' % (distill_weight,))
        if (alpha > 0.0) != (teacher is not None):
            raise ValueError('distill_weight > 0 needs a teacher, and a teacher needs distill_weight > 0 (got %r, %s)'
                             % (distill_weight, 'a teacher' if teacher is not None else 'no teacher'))
        if teacher is not None:
            from .ensemble import Ensemble, _device
            if not isinstance(teacher, Ensemble):
                teacher = Ensemble([teacher])
            if any(m is model for m in teacher.members):
                raise ValueError('the trained model is a member of its own teacher: distil from a copy (copy.deepcopy)')
            v0, v = model.decoder.vocab, teacher.decoder.vocab
            if len(v0) != len(v) or v0.word2idx != v.word2idx or v0.idx2word != v.idx2word:
                raise ValueError("the teacher's vocabulary differs from the model's")
            if _device(teacher.members[0]) != _device(model):
                raise ValueError('the teacher is on %s, the model on %s' % (_device(teacher.members[0]), _device(model)))
        self.label_smoothing, self.teacher, self.distill_weight = eps_ls, teacher, alpha
        self._soft = eps_ls > 0.0 or teacher is not None    # the loss launch is dlsg_ce_ragged_soft
        self._teacher_flats = []
        self.last_loss_parts = None
        if max_grad_norm is not None and clip_grad_value is not None:
            raise ValueError('max_grad_norm and clip_grad_value exclude each other: set at most one')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError('max_grad_norm must be >= 0, not %r' % (max_grad_norm,))
        if clip_grad_value is not None and not (0.0 < float(clip_grad_value) < float('inf')):
            raise ValueError('clip_grad_value must be a positive finite number, not %r' % (clip_grad_value,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.clip_grad_value = None if clip_grad_value is None else float(clip_grad_value)
        self._clip = max_grad_norm is not None or clip_grad_value is not None
        self._clip_slots = self._clip_rec = self._skipped = None
        self.last_grad_norm = self.skipped_steps = None
        self.comm = comm
        # every `check_every` steps the persistent kernels' time-out word is read back (one host synchronisation): a launch that
        # was not co-resident (GPU shared with another process) raises here; meanwhile dlsg_adam's guard kept the weights intact
        self.check_every = check_every
        self._rccl = None
        self._comm_stream = None
        self._comm_pending = False
        self.model = model
        self.lr, self.betas, self.eps = lr, betas, eps
        self.t = 0
        self.world_size = world_size
        self.pg = process_group
        self.use_graphs = use_graphs
        self.device_coins = use_graphs if device_coins is None else device_coins
        self.graph_fallback = graph_fallback   # True: a failed capture downgrades to eager launches (with a warning)
        self.force_graph_cuts = False   # test hook: segment the capture at bucket boundaries even on one GPU
        self.force_collectives = False  # test hook: issue the all-reduces even with one rank (RCCL path on a 1-GPU box)
        # rehearsal hook (one GPU): None, or dict(workgroups=32, passes=n) -- behind every bucket's all-reduce the side stream also
        # runs dlsg_comm_rehearsal over the bucket: `workgroups` x 256 threads streaming it `passes` times, i.e. the CUs and the
        # HBM share a ring all-reduce over xGMI would hold while the backward goes on (values unchanged)
        self.rehearse_cotenant = None
        self.rehearse_ranks = int(rehearse_ranks)
        self._works = []
        self._graphs = None
        self._contact_checked = False
        self._hook_mode, self._hook_sv = False, None
        self._weighted_mode = False     # the captured graphs weight the CrossEntropy per caption (step(seq_weights=...))
        self._spc_mode = 1              # captions per clip of the captured graphs (step(seq_per_clip=...))
        self._risk_mode = None          # (n, alpha, length_penalty) of the captured graphs' minimum-risk loss (step(risk=...)), or None
        self.last_risk = None           # step(risk=...): device views {'Q', 's', 'R', 'stats'} of the last such step
        self.m = self.v = None
        if world_size > 1 or self.rehearse_ranks > 1:
            assert world_size == 1 or not self.rehearse_ranks, 'rehearse_ranks is for one-rank runs'
            self._use_multi_rank_schedule()
            self.force_collectives = self.force_collectives or self.rehearse_ranks > 1
        self._bind()

    # CUs a bucket's all-reduce holds while the backward runs beside it: RCCL launches one 256-thread workgroup per channel (up
    # to 32 on this part).  What a stream-K launch would be budgeted to leave free (`model.sk_backward_cu_budget = cus - COMM_CUS`).
    COMM_CUS = 32

    def _use_multi_rank_schedule(self):
        """The kernel choices of a rank that shares its GPU with gradient all-reduces (set once, at construction, for
        world_size > 1 and for one-GPU rehearsals of it; run_gun.py:63-64 leaves all of this to DDP + NCCL).
        * The persistent BiLSTM kernels need all of their workgroups (one per CU at H = 1024, 152 KB of LDS each) resident
          together.  The encoder's backward runs while the decoder bucket's all-reduce is in flight: a CU that hosts an RCCL
          workgroup has no room for a 152-KB one, so the launch would sit half-resident, its workgroups polling for partners that
          cannot start, until the collective ends -- no deadlock (RCCL does not depend on it), but the CUs it holds and the overlap
          window are lost.  The backward through time therefore runs step by step (0.60 against 0.50 ms); the forward keeps the
          persistent launch (no collective is in flight there: the previous step's all-reduces are joined before its Adam).
        * The stream-K GEMM (csrc/gemm_sk.hip) is one workgroup per CU with the whole register file of its SIMDs, so beside a
          collective its last workgroups start only when CUs come free.  Round 5 put the backward on the tiled kernels for that
          reason, unmeasured.  Round 6 measured it (bench.py `dp_schedule_world1`, DESIGN.md section 6: this schedule on one GPU
          with a co-tenant of RCCL's launch shape -- 32 x 256 threads streaming every bucket for the ~1.1 ms per 180 MB an 8-rank
          ring takes -- on the side stream): stream-K on every CU 14.79 ms per step, tiled backward 15.07, stream-K on a budget
          of 224 workgroups (the 32 CUs left free) 15.33; batch 128: 24.17 / 25.39 / 25.10; without the co-tenant 12.99 / 13.38 /
          13.49 against 12.93 for the one-rank schedule.  The kernel never waits for a workgroup that has not started (shares
          are given away, csrc/gemm_sk.hip), so a launch that is not co-resident is slower by what the co-tenant holds, not by a
          round.  Hence: the backward KEEPS the stream-K launches, on every CU (`model.sk_backward_cu_budget = 0`); the budget
          and `model.stream_k_in_backward = False` remain as switches."""
        model = self.model
        if hasattr(model.ops, 'persistent_bilstm_bwd'):
            model.ops.persistent_bilstm_bwd = False
        model.stream_k_in_backward = True
        model.sk_backward_cu_budget = 0

    def _bind(self):
        """(Re)attach to the model's arenas: Adam moments, bucket ranges, trainable ranges.  Runs again whenever the model
        re-packed its parameters (load_encoder grafts modules) or a parameter's requires_grad changed."""
        model = self.model
        model.flatten_parameters_()
        old_m, old_v = self.m, self.v
        self.m = torch.zeros_like(model._flat)
        self.v = torch.zeros_like(model._flat)
        same = old_m is not None and old_m.shape == self.m.shape and old_m.device == self.m.device
        if same:
            self.m.copy_(old_m); self.v.copy_(old_v)      # same layout (only the frozen set changed): keep the moments
        if self.ema_decay is not None and not (same and self.ema is not None and self.ema.shape == self.m.shape
                                               and self.ema.device == self.m.device):
            self.ema = model._flat.clone()                # the average starts at the weights; kept across a re-bind like m and v
        self._arena = model._flat
        self._graphs = None
        self._bind_teacher()
        # contiguous arena range of each backward bucket (named_parameters order == arena order)
        self._ranges = {}
        frozen = []
        for name, p in model.named_parameters():
            key = name.split('.')[0] if not name.startswith('encoder.') or not hasattr(model.encoder, 'obj_encoder') \
                else '.'.join(name.split('.')[:2])
            o = model._offsets[name]
            end = o + (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
            lo, hi = self._ranges.get(key, (o, end))
            self._ranges[key] = (min(lo, o), max(hi, end))
            if not p.requires_grad:
                frozen.append((o, end))
            if name.endswith('_encoder.obj_embed.weight') and key != name:
                # the deepest weight gradient of a graph module is its last: its range and the rest of the module are buckets of
                # their own (the weight is the module's first parameter: the rest is one contiguous range behind it)
                self._ranges[key + ':obj_embed.weight'] = (o, end)
        for key in [k for k in self._ranges if k.endswith(':obj_embed.weight')]:
            mod = key[:-len(':obj_embed.weight')]
            (wlo, whi), (mlo, mhi) = self._ranges[key], self._ranges[mod]
            if wlo == mlo:
                self._ranges[mod + ':rest'] = (whi, mhi)
            else:
                del self._ranges[key]
        self._frozen = tuple(frozen)
        # maximal runs of trainable parameters: Adam and the all-reduces cover exactly these (torch.optim skips parameters
        # without a gradient; DDP does not reduce them)
        self._train_ranges = self._minus_frozen(0, model._flat.numel())
        self._bind_decay()
        if self._clip:
            # scratch of the clip launches, allocated here and never inside a capture: one block of float64 partials per trainable
            # range (written in full by every dlsg_grad_sumsq launch), the record dlsg_clip_coef writes, the skipped-step counter
            dev = model._flat.device
            slots = abi.defines['DLSG_GRAD_SUMSQ_SLOTS'] * max(1, len(self._train_ranges))
            if self._clip_slots is None or self._clip_slots.numel() != slots or self._clip_slots.device != dev:
                self._clip_slots = torch.zeros(slots, dtype=torch.float64, device=dev)
            if self._clip_rec is None or self._clip_rec.device != dev:
                self._clip_rec = torch.zeros(abi.defines['DLSG_CLIP_RECORD_FLOATS'], dtype=torch.float32, device=dev)
                old = self._skipped
                self._skipped = torch.zeros(1, dtype=torch.int64, device=dev)
                if old is not None:
                    self._skipped.copy_(old)
                self.last_grad_norm = self._clip_rec[abi.defines['DLSG_CLIP_NORM']]
                self.skipped_steps = self._skipped[0]

    @property
    def _ext(self):
        """weight decay or the averaged weights are on: the update is dlsg_adamw_ema's, with four hyper words"""
        return self.weight_decay > 0.0 or self.ema_decay is not None

    def _decayed_names(self):
        """the parameters `decay_filter` puts into the decayed param group, in named_parameters order (what
        `torch.optim.AdamW([{'params': decayed}, {'params': rest, 'weight_decay': 0}])` would be given)"""
        return [n for n, p in self.model.named_parameters() if self.decay_filter is None or self.decay_filter(n, p)]

    def _bind_decay(self):
        """per trainable range the device table of its decayed intervals (dlsg_adamw_ema's decay_ranges, relative to the range):
        (weight decay of the range's launch, table or None for "all of it").  Uploaded here, never inside a capture."""
        self._decay_tabs = {}
        if not self.weight_decay > 0.0:
            return
        model = self.model
        chosen = set(self._decayed_names())
        runs = []                                         # [lo, hi, padded end]: runs of decayed parameters, joined over the padding
        for name, p in model.named_parameters():
            if name not in chosen or name in model.unused_parameters or not p.requires_grad or p.numel() == 0:
                continue
            o = model._offsets[name]
            end = o + (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
            if runs and runs[-1][2] == o:
                runs[-1][1:] = [o + p.numel(), end]
            else:
                runs.append([o, o + p.numel(), end])
        limit = abi.defines['DLSG_ADAM_MAX_RANGES']
        for lo, hi in self._train_ranges:
            tab = [(a - lo, b - lo) for a, b, _ in runs if a >= lo and b <= hi]
            if not tab:
                self._decay_tabs[(lo, hi)] = (0.0, None)
            elif len(tab) == 1 and tab[0][0] == 0 and (tab[0][1] + _ALIGN - 1) // _ALIGN * _ALIGN == hi - lo:
                self._decay_tabs[(lo, hi)] = (self.weight_decay, None)
            else:
                if len(tab) > limit:
                    raise ValueError('%d decayed intervals in one trainable range: dlsg_adamw_ema takes %d' % (len(tab), limit))
                self._decay_tabs[(lo, hi)] = (self.weight_decay, _h2d(tab, torch.int64, model._flat.device).view(-1, 2))

    def _minus_frozen(self, lo, hi):
        out, cur = [], lo
        for a, b in self._frozen:
            if b <= lo or a >= hi:
                continue
            if a > cur:
                out.append((cur, a))
            cur = max(cur, b)
        if cur < hi:
            out.append((cur, hi))
        return out

    def _bind_teacher(self):
        """flatten every teacher member (never inside a capture) and note its arena: captured graphs hold addresses into it"""
        if self.teacher is not None:
            for m in self.teacher.members:
                m.flatten_parameters_()
            self._teacher_flats = [(m, m._flat) for m in self.teacher.members]

    def _check_binding(self):
        model = self.model
        model.flatten_parameters_()
        if self.teacher is not None:
            for m in self.teacher.members:
                m.flatten_parameters_()
            if any(m._flat is not flat for m, flat in self._teacher_flats):
                # a member re-packed its parameters (load_state_dict into a copy, .to()): graphs captured on the old arena go
                self._graphs = None
                self._bind_teacher()
        frozen = tuple((model._offsets[n], model._offsets[n] + (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN)
                       for n, p in model.named_parameters() if not p.requires_grad)
        if self._arena is not model._flat or frozen != self._frozen:
            self._bind()

    def _clip_grads(self):
        """the clip launches, between the join of the collectives and the update: the sum of squares of every trainable range of
        the (all-reduced) gradient arena, then the record {norm, coefficient, non-finite} that `_adam` hands to dlsg_adam_clipped"""
        if not self._clip:
            return
        model, ops = self.model, self.model.ops
        n = abi.defines['DLSG_GRAD_SUMSQ_SLOTS']
        for i, (lo, hi) in enumerate(self._train_ranges):
            ops.grad_sumsq(model._gflat[lo:hi], self._clip_slots[i * n:(i + 1) * n])
        ops.clip_coef(self._clip_slots, 1.0 / self.world_size, float('inf') if self.max_grad_norm is None else self.max_grad_norm,
                      self._clip_rec, self._skipped)

    def _adam(self, step, hyper=None, ranges=None):
        model, ops = self.model, self.model.ops
        ext = self._ext
        for lo, hi in (self._train_ranges if ranges is None else ranges):
            if ext:
                # weight decay and / or the averaged weights: one launch does clip, decay, update and average
                wd, tab = self._decay_tabs[(lo, hi)] if self.weight_decay > 0.0 else (0.0, None)
                ops.adamw_ema(model._flat[lo:hi], model._gflat[lo:hi], self.m[lo:hi], self.v[lo:hi], self.lr, self.betas[0],
                              self.betas[1], self.eps, step, 1.0 / self.world_size, weight_decay=wd,
                              decoupled=self.decoupled_weight_decay, ema=None if self.ema is None else self.ema[lo:hi],
                              ema_decay=self._ema_decay_at(step), hyper=hyper, record=self._clip_rec if self._clip else None,
                              clip_value=self.clip_grad_value or 0.0, decay_ranges=tab)
                continue
            if self._clip:
                ops.adam_clipped(model._flat[lo:hi], model._gflat[lo:hi], self.m[lo:hi], self.v[lo:hi], self.lr, self.betas[0],
                                 self.betas[1], self.eps, step, 1.0 / self.world_size, hyper=hyper, record=self._clip_rec,
                                 clip_value=self.clip_grad_value or 0.0)
                continue
            ops.adam(model._flat[lo:hi], model._gflat[lo:hi], self.m[lo:hi], self.v[lo:hi], self.lr, self.betas[0],
                     self.betas[1], self.eps, step, 1.0 / self.world_size, hyper=hyper)

    # ------------------------------------------------------------------ checkpoint compatibility (run_gun.py:302-310)
    def optimizer_state_dict(self):
        """The Adam state in the layout of `torch.optim.Adam(model.parameters(), ...).state_dict()` -- what the reference
        stores as `optimizer_state_dict` in its checkpoints.  Parameters that never receive a gradient have no entry,
        as in torch (Adam creates state lazily for parameters with a gradient)."""
        model = self.model
        state = {}
        params = dict(model.named_parameters())
        order, split = self._state_order()
        for i, name in enumerate(order):
            p = params[name]
            if name in model.unused_parameters or not p.requires_grad or self.t == 0:
                continue
            o = model._offsets[name]
            state[i] = {'step': torch.tensor(float(self.t)),
                        'exp_avg': self.m[o:o + p.numel()].view(p.shape).clone(),
                        'exp_avg_sq': self.v[o:o + p.numel()].view(p.shape).clone()}
        wd = self.weight_decay if self.weight_decay > 0.0 else 0
        group = {'lr': self.lr, 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': wd, 'amsgrad': False,
                 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                 'decoupled_weight_decay': bool(wd and self.decoupled_weight_decay), 'params': list(range(len(order)))}
        if split is None:
            return {'state': state, 'param_groups': [group]}
        # with a filter: torch's idiom AdamW([{'params': decayed}, {'params': rest, 'weight_decay': 0}]) -- two groups, the state
        # numbered over their concatenation
        rest = dict(group, weight_decay=0, params=list(range(split, len(order))))
        group['params'] = list(range(split))
        return {'state': state, 'param_groups': [group, rest]}

    def _state_order(self):
        """-> (parameter names in the order torch numbers the optimizer state, size of the decayed group or None for one group)"""
        names = [n for n, _ in self.model.named_parameters()]
        if self.decay_filter is None:
            return names, None
        chosen = self._decayed_names()
        seen = set(chosen)
        return chosen + [n for n in names if n not in seen], len(chosen)

    def load_optimizer_state_dict(self, sd):
        """Resume from a reference checkpoint's `optimizer_state_dict` (torch.optim.Adam layout: one param group), or from what
        `optimizer_state_dict` wrote with a decay_filter (two groups, decayed parameters first; this trainer's filter says which
        they are).  lr, betas, eps, weight_decay and decoupled_weight_decay are taken from group 0."""
        model = self.model
        model.flatten_parameters_()
        groups = sd['param_groups']
        params = dict(model.named_parameters())
        if len(groups) == 1:
            order = list(params)
        else:
            order, split = self._state_order()
            if len(groups) != 2 or split is None or [len(g['params']) for g in groups] != [split, len(order) - split]:
                raise ValueError('%d param groups of %s parameters: not a layout this trainer (decay_filter %s) can resume'
                                 % (len(groups), [len(g['params']) for g in groups], 'set' if split is not None else 'None'))
        self.m.zero_()
        self.v.zero_()
        steps = set()
        for i, name in enumerate(order):
            p = params[name]
            st = sd['state'].get(i, sd['state'].get(str(i)))
            if st is None:
                continue
            o = model._offsets[name]
            self.m[o:o + p.numel()].view(p.shape).copy_(st['exp_avg'])
            self.v[o:o + p.numel()].view(p.shape).copy_(st['exp_avg_sq'])
            steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError('per-parameter step counts differ (%s): not a state this trainer can resume' % sorted(steps))
        self.t = steps.pop() if steps else 0
        g = sd['param_groups'][0]
        self.lr, self.betas, self.eps = g['lr'], tuple(g['betas']), g['eps']
        wd = float(g.get('weight_decay', 0))
        if wd != self.weight_decay or (wd > 0.0 and 'decoupled_weight_decay' in g
                                       and bool(g['decoupled_weight_decay']) != self.decoupled_weight_decay):
            if not wd >= 0.0:
                raise ValueError('weight_decay %r in the state dict' % (g.get('weight_decay'),))
            self.weight_decay = wd
            if wd > 0.0:
                self.decoupled_weight_decay = bool(g.get('decoupled_weight_decay', self.decoupled_weight_decay))
            self._bind_decay()
        self._graphs = None          # captured graphs bake nothing of this state, but recapture keeps the invariants simple

    # ------------------------------------------------------------------ the averaged weights
    def _ema_decay_at(self, t):
        if self.ema_decay is None:
            return 0.0
        return min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay

    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError('this trainer keeps no averaged weights: build it with ema_decay')
        self._check_binding()

    @contextlib.contextmanager
    def averaged(self):
        """`with tr.averaged():` -- the model computes with the averaged weights inside the block: the bits of the weight arena
        and of `ema` are exchanged in place (dlsg_swap_f32) and exchanged back on exit, also when the block raises.  No address
        changes, so every captured graph -- this trainer's and the inference graphs of graphs.py -- sees the averaged weights
        without recapture.  What `scoring.evaluate`, `gather_results` and `perplexity` run under; `step` inside raises."""
        self._need_ema()
        if self._averaging:
            raise RuntimeError('averaged() is already active')
        ops, flat, ema = self.model.ops, self.model._flat, self.ema
        ops.swap(flat, ema)
        self._averaging = True
        try:
            yield self.model
        finally:
            self._averaging = False
            ops.swap(flat, ema)

    def ema_state_dict(self):
        """the model's state dict (its keys and shapes) with every parameter taken from `ema`, as clones: loads with
        `load_state_dict` into a `copy.deepcopy(model)`, e.g. to put the averaged model into an `Ensemble` beside the raw one"""
        self._need_ema()
        if self._averaging:
            raise RuntimeError('inside averaged() the arenas are exchanged: take the state dict outside the block')
        model = self.model
        sd = collections.OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items())
        for name, p in model.named_parameters():
            o = model._offsets[name]
            sd[name] = self.ema[o:o + p.numel()].view(p.shape).clone()
        return sd

    def load_ema_state_dict(self, sd):
        """restore the average from what `ema_state_dict` returned (resume)"""
        self._need_ema()
        if self._averaging:
            raise RuntimeError('inside averaged() the arenas are exchanged: load the average outside the block')
        model = self.model
        missing = [n for n, _ in model.named_parameters() if n not in sd]
        if missing:
            raise KeyError('the EMA state dict lacks %s' % missing[:5])
        for name, p in model.named_parameters():
            o = model._offsets[name]
            self.ema[o:o + p.numel()].view(p.shape).copy_(sd[name])

    # ------------------------------------------------------------------ collectives
    def _comm_mode(self):
        """'none' | 'rccl' | 'torch' for this trainer's next step"""
        if self.world_size <= 1 and not self.force_collectives:
            return 'none'
        if self.comm == 'torch':
            return 'torch'
        on_gpu = self.model._flat is not None and self.model._flat.is_cuda
        if self.comm == 'rccl' and not on_gpu:
            raise RuntimeError("comm='rccl' needs the model on a GPU")
        return 'rccl' if on_gpu else 'torch'

    def _rccl_comm(self):
        if self._rccl is None:
            from .comm import RcclComm
            rank = 0
            if self.world_size > 1:
                import torch.distributed as dist
                rank = dist.get_rank(self.pg)
            self._rccl = RcclComm(self.world_size, rank, self.pg, lib=getattr(self.model.ops, 'lib', None))
            self._side_stream()
            self._first_contact(rank)
        return self._rccl

    def _first_contact(self, rank):
        """One eager all-reduce of a rank-id pattern through the new communicator before anything is captured: every element must
        come back as 0 + 1 + ... + (N - 1) on every rank.  A communicator that is wired wrongly (a rank on the wrong device, two
        jobs sharing an id, a transport that drops data) is found here, with the list of ranks that saw a wrong sum, instead
        of as diverging replicas or a hang inside a replayed graph (run_gun.py:63-64 relies on DDP's own constructor checks)."""
        if self.world_size <= 1:
            return
        import torch.distributed as dist
        dev = self.model._flat.device
        side = self._side_stream()
        t = torch.full((4096,), float(rank), dtype=torch.float32, device=dev)
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        self._rccl.allreduce([t], side)
        side.synchronize()
        want = self.world_size * (self.world_size - 1) / 2.0
        ok = bool((t == want).all().item())
        every = [None] * self.world_size
        dist.all_gather_object(every, (rank, ok, float(t[0].item())), group=self.pg)
        bad = [(r, v) for r, o, v in every if not o]
        if bad:
            raise RuntimeError('RCCL first-contact check failed: the all-reduced rank pattern should be %g everywhere; wrong on ranks %s'
                               % (want, ', '.join('%d (got %g)' % rv for rv in bad)))

    def _side_stream(self):
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=self.model._flat.device)
        return self._comm_stream

    def _allreduce(self, key):
        """key: a bucket name or a tuple of bucket names whose gradients are complete: hand them to the reduction.  (Adam per
        bucket on the side stream right behind its all-reduce was measured and removed: 14.87 ms per step against 14.47 -- the
        update's 1.4 GB stream evicts the Infinity-Cache-resident operands of the backward that is still running.)"""
        mode = self._comm_mode()
        ranges = [r for k in (key if isinstance(key, tuple) else (key,)) for r in self._minus_frozen(*self._ranges[k])]
        views = [self.model._gflat[lo:hi] for lo, hi in ranges]
        if mode == 'torch':
            import torch.distributed as dist
            for v in views:
                self._works.append(dist.all_reduce(v, group=self.pg, async_op=True))
            return
        if mode == 'none':
            return
        comm = self._rccl_comm()
        side = self._side_stream()
        # fork: the side stream waits for everything enqueued so far (the bucket's gradients), the main stream goes on
        # with the rest of the backward; under stream capture both become edges of the step's graph
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        comm.allreduce(views, side)
        if self.rehearse_cotenant and self.world_size == 1:
            co = self.rehearse_cotenant
            with torch.cuda.stream(side):
                for v in views:
                    self.model.ops.comm_rehearsal(v, int(co.get('workgroups', self.COMM_CUS)), int(co['passes']))
        self._comm_pending = True

    def _reduce_guard(self):
        """The persistent kernels' time-out word (BiLSTM, critic LSTM), max over the ranks, BEHIND the last launch of the backward
        and in front of Adam: dlsg_adam's guard then skips the update on every rank or on none -- a rank skipping alone would leave
        the replicas diverged, its invalid gradients already summed into everybody's.  (Until round 5 the word rode with the FIRST
        bucket: a time-out in the encoder's backward, behind that bucket, was not agreed.)  Four bytes behind the step's last,
        already exposed bucket on the same side stream."""
        mode = self._comm_mode()
        if mode == 'none':
            return
        # (the word is created here if no persistent kernel has run yet: whether a rank takes part in this collective must not
        #  depend on what its kernels happened to do)
        mk = getattr(self.model.ops, 'guard_word', None)
        if mk is None:
            return
        word = mk(self.model._flat.device)
        if mode == 'torch':
            import torch.distributed as dist
            self._works.append(dist.all_reduce(word, op=dist.ReduceOp.MAX, group=self.pg, async_op=True))
            return
        comm = self._rccl_comm()
        side = self._side_stream()
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        comm.allreduce_max_word(word, side)
        self._comm_pending = True

    def _join_comm(self):
        """the main stream waits for the side stream's collectives (before Adam; before a capture segment ends)"""
        if self._comm_pending:
            ev = torch.cuda.Event()
            ev.record(self._comm_stream)
            torch.cuda.current_stream().wait_event(ev)
            self._comm_pending = False

    def collectives_info(self):
        mode = self._comm_mode()
        info = {'mode': {'none': 'none (one rank)', 'rccl': 'RCCL through the C ABI (dlsg_allreduce_bucket), side stream',
                         'torch': 'torch.distributed all_reduce(async_op=True) issued by the host'}[mode],
                'where': None if mode == 'none' else ('inside the step\'s hipGraph' if (mode == 'rccl' and self.use_graphs and
                                                      self._graphs is not None and len(self._graphs) == 1)
                                                     else ('between hipGraph segments' if self.use_graphs and self._graphs is not None
                                                           else 'between eager launches')),
                'graph_replays_per_step': len(self._graphs) if (self.use_graphs and self._graphs is not None) else 0,
                'buckets_MB': {k: round(4e-6 * sum(hi - lo for lo, hi in self._minus_frozen(*r)), 1) for k, r in self._ranges.items()}}
        if self._rccl is not None:
            info['rccl_version'] = self._rccl.rccl_version
        return info

    def check(self):
        """Raise if a persistent kernel's inter-workgroup wait timed out since the last call (ops.check_persistent).  A host
        synchronisation: call it where the loss is read back (per logging interval / epoch), not per step."""
        ops = self.model.ops
        chk = getattr(ops, 'check_persistent', None)
        if chk is None:
            return
        w = ops.persist_word_or_none()
        code = int(w.item()) if w is not None else 0
        if self._rccl is not None:
            ae = self._rccl.async_error()
            if ae:
                import sys
                sys.stderr.write('dlsg_amd.Trainer: RCCL reports asynchronous error %d on this rank (ncclCommGetAsyncError)\n' % ae)
                code = code or 100 + ae
        if self.world_size > 1:
            # every rank learns the worst code before any of them raises: one rank leaving alone would strand its peers in the
            # next step's in-graph all-reduce (a private communicator has no time-out)
            from .comm import _agree_min
            code = _agree_min(code, self.pg, negate=True)
        if code:
            self._graphs = None            # captured on the persistent schedule: the next step captures again
            if code >= 100:
                raise RuntimeError('RCCL asynchronous error %d on at least one rank (ncclCommGetAsyncError): the gradient exchange '
                                   'of the steps since the last check is not to be trusted' % (code - 100))
            if w is not None and int(w.item()) == 0:
                w.fill_(code)              # (another rank's time-out: the same exception here)
            chk(code=code)

    def close(self):
        """destroy the RCCL communicator (collective: every rank calls it)"""
        self.check()
        if self._rccl is not None:
            torch.cuda.synchronize()
            self._rccl.close()
            self._rccl = None

    # ------------------------------------------------------------------ one step, as a schedule
    def _schedule(self, frames, regions, captions, cap_lens, coins, seed, dev_coins, on_bucket, extra_dlogits=None, seq_weights=None,
                  seq_per_clip=1, risk=None):
        model, ops = self.model, self.model.ops
        L = captions.shape[1]
        sv = {}
        training = model.training
        # seq_per_clip = n > 1: frames / regions hold B clips, captions / cap_lens / seq_weights their B*n caption rows
        # a bucket handed to a reduction (or closing a graph segment) must be complete: deferred weight gradients go out there
        model._flush_at_buckets = self._comm_mode() != 'none' or self.force_graph_cuts
        teachers = ()
        if self.teacher is not None:
            # the teacher first: its workspaces are free again before the student allocates; only the members' logits stay
            teachers = self.teacher.teacher_logits(frames, regions, captions, seq_per_clip=seq_per_clip)
        model._engine_forward(frames, regions, captions, L, coins, training, seed, sv, dev_coins, outputs=False, seq_per_clip=seq_per_clip)
        s = sv['dec']
        Bn = captions.shape[0]
        dl = torch.empty_like(s['LOGITS'])
        if risk is not None:
            # minimum-risk training: the expected reward over each clip's n candidate rows; its two launches stand where the
            # CrossEntropy's one stood (the weights depend on this pass's log-probabilities: they cannot be handed in)
            n = risk['n']
            f64 = dict(dtype=torch.float64, device=dl.device)
            lse, tok_lp = (torch.empty(L * Bn, dtype=torch.float32, device=dl.device) for _ in range(2))
            out = dict(Q=torch.empty(Bn // n, n, **f64), s=torch.empty(Bn // n, n, **f64), R=torch.empty(Bn // n, **f64),
                       stats=torch.empty(4, **f64))
            loss = torch.empty(1, dtype=torch.float32, device=dl.device)
            ops.risk_rows(s['LOGITS'], captions, cap_lens, lse, tok_lp, n, time_major=True)
            ops.risk_grad(s['LOGITS'], captions, cap_lens, lse, tok_lp, risk['rewards'], risk['mask'], dl, out['Q'], out['s'], out['R'],
                          loss, out['stats'], n, time_major=True, alpha=risk['alpha'], length_penalty=risk['length_penalty'])
            self.last_risk = out
            model._engine_backward(sv, dl, None, None, None, training, seed, on_bucket=on_bucket, seq_per_clip=seq_per_clip)
            return loss
        row_loss = torch.empty((3 if self._soft else 1) * L * Bn, dtype=torch.float32, device=dl.device)
        loss = torch.empty(3 if self._soft else 1, dtype=torch.float32, device=dl.device)
        if self._soft:
            from .ensemble import MODES
            ops.ce_ragged_soft(s['LOGITS'], captions, cap_lens, dl, row_loss, loss, time_major=True, smoothing=self.label_smoothing,
                               weights=seq_weights, teachers=teachers,
                               teacher_weights=self.teacher.weights if teachers else None,
                               mode=MODES[self.teacher.mode] if teachers else 0, alpha=self.distill_weight)
            self.last_loss_parts = loss
            loss = loss[0:1]
        elif seq_weights is None:
            ops.ce_ragged(s['LOGITS'], captions, cap_lens, dl, row_loss, loss, time_major=True)
        else:
            # policy gradient of self-critical training: caption b's CrossEntropy weighted by its advantage
            ops.ce_ragged_weighted(s['LOGITS'], captions, cap_lens, seq_weights, dl, row_loss, loss, time_major=True)
        if extra_dlogits is not None:
            # another loss on the logits (the GAN term of run_gun.py:218-231): its gradient joins the CrossEntropy's
            sv['loss_dev'] = loss
            g = extra_dlogits(s['LOGITS'], sv)
            V = dl.shape[-1]
            ops.copy2d(g.contiguous().view(-1, V), dl.view(-1, V), accum=True)
        model._engine_backward(sv, dl, None, None, None, training, seed, on_bucket=on_bucket, seq_per_clip=seq_per_clip)
        return loss

    def _hyper(self):
        b1, b2 = self.betas
        h = [self.lr / (1.0 - b1 ** self.t), math.sqrt(1.0 - b2 ** self.t)]
        if self._ext:
            # dlsg_adamw_ema's two further words, in float64 like the first two and rounded once on the way to the device: the decay
            # factor (of the plain lr) and the average's weight 1 - d_t
            h += [1.0 - self.lr * self.weight_decay if self.decoupled_weight_decay else self.weight_decay,
                  1.0 - self._ema_decay_at(self.t)]
        return h

    @torch.no_grad()
    def step(self, frames, regions, captions, cap_lens, tf_ratio, max_len=26, extra_dlogits=None, seed=None, seq_weights=None,
             seq_per_clip=1, risk=None):
        """One optimisation step.  Returns the (device) scalar loss of this rank's shard.
        extra_dlogits: optional callable (logits (L,B,V) time-major, saved-state dict) -> (L,B,V) gradient of an additional
        loss on the logits, added to the CrossEntropy's before the backward.  With use_graphs the captured step is cut at
        that point: forward + CrossEntropy replay, the callable runs (on the graphs' static logits / saved state), its result
        is copied into a static buffer that the replayed backward adds to the CrossEntropy gradient.
        seed: the dropout seed of the step (None: the model's next one) -- a self-critical step passes the seed its samples were
        drawn with, so that the masks are those of the sampling pass.
        seq_weights: optional (B,) per-caption weights of the CrossEntropy (`ce_ragged_weighted`; the advantages of self-critical
        training); with use_graphs that form of the step is captured on its own, the weights read from a static device buffer.
        seq_per_clip = n > 1 (CapGnnModel): frames / regions hold B clips and captions / cap_lens / seq_weights their B*n caption
        rows, clip b's in rows b*n .. b*n+n-1.  The encoder and its backward run once per clip (`CapGnnModel.forward`), the loss
        is the same ragged CrossEntropy over all B*n captions, and the gradient arena, buckets, clipping and Adam are those of
        any step.  Encoder dropout is keyed by the clip row, decoder and word dropout by the caption row.  With use_graphs the
        captured step is for one n and one pair of row counts; other batches run kernel by kernel.
        risk: dict(rewards=, n=, mask=None, alpha=, length_penalty=0.0) -- minimum-risk training (Shen et al. 2016): captions holds
        n candidate captions per clip, clip b's in rows b*n .. b*n+n-1, rewards (rows,) float64 or float32 their rewards and mask
        (rows,) bool which of them count (None: all).  The loss is the negative expected reward under the model renormalised
        over each clip's list, Q_bi ~ exp(alpha * s_bi / len_bi^length_penalty) with s_bi the caption's log-probability in THIS
        pass; its two launches (`risk_rows`, `risk_grad`; include/addons/dlsg_risk.h has the arithmetic and the rules for masked
        candidates and bad targets) replace the CrossEntropy's and everything else is the step as it was: seq_per_clip (= n: one
        encoder pass per clip) or rows expanded n-fold, clipping, weight decay, the averaged weights, the data-parallel schedule.
        The step returns the loss and `last_risk` holds device views 'Q' and 's' (B, n) float64, 'R' (B,) float64 and 'stats' (4,)
        float64 {loss, mean reward and mean length of the counted candidates, mean R_b}.  With use_graphs this form of the step
        is captured on its own for one (n, alpha, length_penalty), rewards and mask read from static buffers.  seq_weights,
        extra_dlogits, label_smoothing, a teacher and tf_ratio != 1 are refused with it."""
        model, ops = self.model, self.model.ops
        if risk is not None:
            risk = self._check_risk(risk, captions, max_len, tf_ratio, extra_dlogits, seq_weights)
        if self._averaging:
            raise RuntimeError('step inside `with trainer.averaged():` -- the weight arena holds the averaged weights')
        n_seq = model._check_seq_per_clip(seq_per_clip, frames.shape[0], captions)
        self._check_binding()
        captions = captions[:, :max_len].contiguous()
        if not (torch.is_tensor(cap_lens) and cap_lens.device == captions.device and cap_lens.dtype == torch.int64):
            cap_lens = _h2d(cap_lens, torch.int64, captions.device)
        L = captions.shape[1]
        coins = model._draw_coins(L, False, tf_ratio)
        seed = model.next_seed() if seed is None else int(seed)
        self.t += 1
        hook = extra_dlogits is not None
        weighted = seq_weights is not None
        if weighted and not (torch.is_tensor(seq_weights) and seq_weights.device == captions.device
                             and seq_weights.dtype == torch.float32):
            seq_weights = _h2d(seq_weights, torch.float32, captions.device)
        risk_key = None if risk is None else (risk['n'], risk['alpha'], risk['length_penalty'])
        if self.use_graphs and (self._graphs is None or (self._hook_mode == hook and self._weighted_mode == weighted
                                                         and self._spc_mode == n_seq and self._risk_mode == risk_key)):
            loss = self._step_graphs(frames, regions, captions, cap_lens, coins, seed, extra_dlogits, seq_weights, n_seq, risk)
        else:
            # (a trainer's graphs are captured for one form of the step; the other forms run kernel by kernel)
            loss = self._eager_step(frames, regions, captions, cap_lens, coins, seed, counted=True, extra_dlogits=extra_dlogits,
                                    seq_weights=seq_weights, seq_per_clip=n_seq, risk=risk)
        if self.check_every and self.t % self.check_every == 0:
            self.check()
        return loss

    RISK_MAX_N, RISK_MAX_L = 32, 64    # csrc/risk.hip: one lane per candidate, words per caption

    def _check_risk(self, risk, captions, max_len, tf_ratio, extra_dlogits, seq_weights):
        """step(risk=...) as `_schedule` takes it: n int, alpha and length_penalty floats, rewards float64 and mask bool (or None)
        on the captions' device; ValueError for what the minimum-risk step does not cover"""
        for what, on in (('seq_weights', seq_weights is not None), ('extra_dlogits', extra_dlogits is not None),
                         ('label_smoothing', self.label_smoothing > 0.0), ('teacher', self.teacher is not None),
                         ('tf_ratio != 1', float(tf_ratio) != 1.0)):
            if on:
                raise ValueError('risk with %s: the minimum-risk loss replaces the CrossEntropy, teacher-forced on the candidates; '
                                 '%s belongs to the CrossEntropy step' % (what, what))
        if not isinstance(risk, dict) or set(risk) - {'rewards', 'n', 'mask', 'alpha', 'length_penalty'} \
                or not {'rewards', 'n', 'alpha'} <= set(risk):
            raise ValueError('risk must be dict(rewards=, n=, mask=None, alpha=, length_penalty=0.0), not %r'
                             % (sorted(risk) if isinstance(risk, dict) else risk,))
        n, alpha, lp = int(risk['n']), float(risk['alpha']), float(risk.get('length_penalty', 0.0))
        rows, L = captions.shape[0], min(captions.shape[1], max_len)
        if not 1 <= n <= self.RISK_MAX_N or n != risk['n'] or rows % n:
            raise ValueError('risk: n must be in 1..%d and divide the %d caption rows, not %r' % (self.RISK_MAX_N, rows, risk['n']))
        if L > self.RISK_MAX_L:
            raise ValueError('risk: captions of %d words; the minimum-risk kernels take %d' % (L, self.RISK_MAX_L))
        if not (alpha >= 0.0 and math.isfinite(alpha) and math.isfinite(lp)):
            raise ValueError('risk: alpha must be finite and >= 0 and length_penalty finite, not %r, %r' % (risk['alpha'], lp))
        rewards, mask = risk['rewards'], risk.get('mask')
        if not (torch.is_tensor(rewards) and rewards.device == captions.device and rewards.shape == (rows,)
                and rewards.dtype in (torch.float64, torch.float32)):
            raise ValueError('risk: rewards must be a (%d,) float64 or float32 tensor on %s' % (rows, captions.device))
        if mask is not None and not (torch.is_tensor(mask) and mask.device == captions.device and mask.shape == (rows,)
                                     and mask.dtype == torch.bool):
            raise ValueError('risk: mask must be None or a (%d,) bool tensor on %s' % (rows, captions.device))
        return dict(rewards=rewards.to(torch.float64).contiguous(), mask=None if mask is None else mask.contiguous(), n=n,
                    alpha=alpha, length_penalty=lp)

    def _eager_step(self, frames, regions, captions, cap_lens, coins, seed, counted=False, extra_dlogits=None, seq_weights=None,
                    seq_per_clip=1, risk=None):
        model, ops = self.model, self.model.ops
        if not counted:
            self.t += 1
        dev_coins = None
        if self.device_coins:
            dev_coins = _h2d([int(c) for c in coins], torch.int32, captions.device)
        self._works = []
        loss = self._schedule(frames, regions, captions, cap_lens, coins, seed, dev_coins, self._allreduce, extra_dlogits, seq_weights,
                              seq_per_clip, risk)
        self._reduce_guard()
        for w in self._works:
            w.wait()
        self._join_comm()
        if not self._clip and not self._soft and not self._ext:
            self._adam(self.t)
            return loss
        # a clipping (or label-smoothing / distilling / decaying / averaging) trainer's eager step (a batch of another shape than the captured one, or
        # use_graphs=False) reads the bias corrections from device words the host computed, as the captured step does: one arithmetic for both, so the two forms
        # of a step give the same bits (dlsg_adam's own float powf / sqrtf differ from them in the last place)
        hyper = _h2d(self._hyper(), torch.float32, captions.device)
        self._clip_grads()
        self._adam(self.t, hyper=hyper)
        return loss

    # ------------------------------------------------------------------ hipGraph path
    def _capture(self, frames, regions, captions, cap_lens, hook=False, weighted=False, seq_per_clip=1, risk=None):
        dev = frames.device
        L = captions.shape[1]
        self._hook_mode, self._hook_sv = hook, None
        self._weighted_mode = weighted
        self._spc_mode = seq_per_clip
        self._risk_mode = None if risk is None else (risk['n'], risk['alpha'], risk['length_penalty'])
        st = self._static = dict(frames=frames.clone(), regions=regions.clone(), captions=captions.clone(),
                                 lens=cap_lens.clone())
        st['weights'] = torch.ones(captions.shape[0], dtype=torch.float32, device=dev) if weighted else None
        # the minimum-risk form reads rewards and mask from static buffers (a step without a mask fills it with True: every
        # candidate counts, the bits of mask=None); n, alpha and length_penalty are constants of the captured launches
        st['risk'] = None if risk is None else dict(risk, rewards=torch.zeros(captions.shape[0], dtype=torch.float64, device=dev),
                                                    mask=torch.ones(captions.shape[0], dtype=torch.bool, device=dev))
        # what changes every step besides the batch -- the scheduled-sampling coins, the dropout seed, Adam's bias corrections --
        # lives in ONE device buffer (int32 words: coins | seed (int64) | hyper (2 x float32; 4 with weight decay or averaged
        # weights)), so that a step sends it as one copy
        Lp = (L + 1) // 2 * 2
        nh = st['n_hyper'] = 4 if self._ext else 2
        st['scalars'] = torch.zeros(Lp + 2 + nh, dtype=torch.int32, device=dev)
        st['coins'] = st['scalars'][:L]
        st['coins'].fill_(1)
        st['seed'] = st['scalars'][Lp:Lp + 2].view(torch.int64)
        st['hyper'] = st['scalars'][Lp + 2:Lp + 2 + nh].view(torch.float32)
        mode = self._comm_mode()
        # host-issued collectives need the capture cut at every bucket; RCCL's own launches are captured with the step
        cuts = mode == 'torch' or self.force_graph_cuts
        if mode == 'rccl':
            self._rccl_comm()              # communicator setup (a collective itself) outside any capture

        def warmup():
            # (with RCCL the warm-up also runs the collectives once: channel buffers are set up before the capture;
            #  nothing is updated: Adam is not part of the schedule)
            self._schedule(st['frames'], st['regions'], st['captions'], st['lens'], None, st['seed'], st['coins'],
                           self._allreduce if mode == 'rccl' else None, seq_weights=st['weights'], seq_per_clip=seq_per_clip,
                           risk=st['risk'])
            if mode == 'rccl':
                self._reduce_guard()
            self._join_comm()
            if self._comm_stream is not None:
                self._comm_stream.synchronize()

        def body(hard_cut):
            def cut(key):
                if mode != 'torch':
                    self._allreduce(key)               # captured: fork to the side stream (collective and / or Adam)
                    if cuts:
                        self._join_comm()              # a capture segment must end with its forks joined
                if cuts:
                    hard_cut(key if mode == 'torch' else None)

            def placeholder(logits, sv):
                # the graphs end here and resume after the caller's term: what it will read (logits, saved state, the
                # loss) lives in the graphs' pool, what it returns is copied into st['extra'] before the next replay
                # (allocated BETWEEN the two captures: inside one, its zero fill would be replayed over the copy)
                def alloc():
                    st['extra'] = torch.zeros_like(logits)
                hard_cut('hook', alloc)
                self._hook_sv = (logits, sv)
                return st['extra']

            loss = self._schedule(st['frames'], st['regions'], st['captions'], st['lens'], None, st['seed'], st['coins'], cut,
                                  placeholder if hook else None, st['weights'], seq_per_clip, st['risk'])
            if mode != 'torch':
                # no host-issued collective between backward and update: Adam is part of the graph, behind the join of the
                # side stream's collectives; with host-issued collectives it follows their waits
                self._reduce_guard()
                self._join_comm()
                self._clip_grads()
                self._adam(1, hyper=st['hyper'])
            return loss

        try:
            graphs, loss = capture_segments(dev, body, warmup)
        except BaseException:
            # (the capture is ended and its partial graphs are dropped by now: what is left is this trainer's own state)
            self._graphs = None
            self._comm_pending = False
            raise
        self._graphs, self._loss = graphs, loss
        st['parts'] = self.last_loss_parts        # (the captured launch's three floats: every replay rewrites them)
        st['risk_out'] = self.last_risk if risk is not None else None
        self._adam_in_graph = mode != 'torch'

    def _capture_agreed(self, frames, regions, captions, cap_lens, hook, weighted=False, seq_per_clip=1, risk=None):
        """`_capture`, and with several ranks the agreement on its outcome: returns None when EVERY rank captured, else the error
        (this rank's own, or a stand-in when only another rank failed) after dropping this rank's graphs -- so that all ranks take
        the same fallback together"""
        err = None
        try:
            self._capture(frames, regions, captions, cap_lens, hook, weighted, seq_per_clip, risk)
        except Exception as e:            # (any failure votes: an AssertionError on one rank must not leave the others in the vote)
            err = e
        if self.world_size > 1:
            from .comm import _agree_min
            if _agree_min(0 if err is not None else 1, self.pg) == 0 and err is None:
                err = RuntimeError('hipGraph capture failed on another rank')
                self._graphs = None
        return err

    @torch.no_grad()
    def forward_only(self, frames, regions, captions, tf_ratio, max_len=26, time_major=False, seq_per_clip=1):
        """The no-grad generator forward of the GAN iteration (run_gun.py:167) from the captured step's FIRST graph (forward +
        CrossEntropy): same coin / dropout-seed draws as `model(frames, regions, captions, max_len, tf_ratio)`, returns
        (logits (B,L,V), obj, mot, alpha (B,L,2P)) as views of the graphs' static buffers -- valid until the next replay --
        or None when this trainer has no cut graphs for that batch shape (the caller then calls the model).
        seq_per_clip = n: as in `step` -- B clips, B*n caption rows; logits and alpha have B*n rows, obj and mot B, as the model
        returns them; None unless the graphs were captured for that n."""
        if not (self.use_graphs and self._graphs is not None and self._hook_mode and self._hook_sv is not None
                and self.model.training and self._spc_mode == int(seq_per_clip)):
            return None
        st = self._static
        captions = captions[:, :max_len].contiguous()
        if (frames.shape, regions.shape, captions.shape) != (st['frames'].shape, st['regions'].shape, st['captions'].shape):
            return None
        self._check_binding()
        model = self.model
        coins = model._draw_coins(captions.shape[1], False, tf_ratio)
        seed = model.next_seed()
        for k, src in (('frames', frames), ('regions', regions), ('captions', captions)):
            stage(st[k], src)
        self._send_scalars(coins, seed, None)
        self._graphs[0][0].replay()
        logits_tm, sv = self._hook_sv
        # time_major: the logits as the decoder wrote them, (L,B,V) -- what the critic's schedule reads (gan.GanTrainer)
        enc_out = sv['enc_out'] if self._spc_mode != 1 else sv['dec_gsrc']      # (the B-row proposals, as the model returns them)
        return (logits_tm if time_major else logits_tm.transpose(0, 1)), enc_out[0], enc_out[1], \
            sv['dec']['ALPHA'].transpose(0, 1)

    def _send_scalars(self, coins, seed, hyper):
        """coins, dropout seed and (optionally) Adam's bias corrections of this step into the graphs' static words: one host buffer,
        one asynchronous copy (hyper None: the words keep their value)"""
        st = self._static
        n = st['scalars'].numel()
        L = st['coins'].numel()
        nh = st['n_hyper']
        host = torch.empty(n, dtype=torch.int32)
        host[:L] = torch.tensor([int(c) for c in coins], dtype=torch.int32)
        host[L:n - nh - 2] = 0
        host[n - nh - 2:n - nh].view(torch.int64)[0] = seed
        if hyper is None:
            _copy_h2d(st['scalars'][:n - nh], host[:n - nh])
            return
        host[n - nh:].view(torch.float32).copy_(torch.tensor(hyper, dtype=torch.float32))
        _copy_h2d(st['scalars'], host)

    def static_inputs(self):
        """The captured graphs read their batch from these device buffers: (frames, regions, captions, cap_lens), or None
        before the first replayed step (captured with seq_per_clip = n: frames / regions of B rows, captions / cap_lens of B*n).  A producer that fills them in place (the HBM-resident feature store gathers a batch
        straight into them, `ResidentFeatures.batch(ids, out=...)`) and then passes the very same tensors to `step` saves the
        device-to-device staging copy of the batch (258 MB per step at batch 64, MSVD-shaped)."""
        if self._graphs is None:
            return None
        st = self._static
        return st['frames'], st['regions'], st['captions'], st['lens']

    def _step_graphs(self, frames, regions, captions, cap_lens, coins, seed, extra_dlogits=None, seq_weights=None, seq_per_clip=1,
                     risk=None):
        model, ops = self.model, self.model.ops
        hook = extra_dlogits is not None
        weighted = seq_weights is not None
        if self._graphs is None:
            err = self._capture_agreed(frames, regions, captions, cap_lens, hook, weighted, seq_per_clip, risk)
            if err is not None and self.graph_fallback and self._comm_mode() == 'rccl' and self.world_size > 1:
                # the in-graph RCCL capture was refused somewhere: EVERY rank retries the segmented form (torch.distributed
                # collectives issued by the host between graph segments) -- a rank replaying graphs that hold private-communicator
                # collectives next to ranks issuing host collectives would hang the job
                import warnings
                warnings.warn('capture with in-graph RCCL collectives failed (%s: %s); all ranks retry with host-issued '
                              'torch.distributed collectives between graph segments' % (type(err).__name__, err))
                torch.cuda.synchronize()
                self.comm = 'torch'
                err = self._capture_agreed(frames, regions, captions, cap_lens, hook, weighted, seq_per_clip, risk)
            if err is not None:
                if not self.graph_fallback:
                    raise err
                # opted in: keep the run alive on kernel-by-kernel launches -- on every rank
                import warnings
                warnings.warn('hipGraph capture failed (%s: %s); continuing with eager launches' % (type(err).__name__, err))
                torch.cuda.synchronize()
                self.use_graphs, self._graphs = False, None
                return self._eager_step(frames, regions, captions, cap_lens, coins, seed, counted=True, extra_dlogits=extra_dlogits,
                                        seq_weights=seq_weights, seq_per_clip=seq_per_clip, risk=risk)
        st = self._static
        if (frames.shape, regions.shape, captions.shape) != (st['frames'].shape, st['regions'].shape, st['captions'].shape):
            # a batch of another shape (the short last batch of an epoch; other clip or caption row counts): the captured graphs
            # are for one shape only
            return self._eager_step(frames, regions, captions, cap_lens, coins, seed, counted=True, extra_dlogits=extra_dlogits,
                                    seq_weights=seq_weights, seq_per_clip=seq_per_clip, risk=risk)
        for k, src in (('frames', frames), ('regions', regions), ('captions', captions), ('lens', cap_lens)):
            stage(st[k], src)
        if weighted:
            st['weights'].copy_(seq_weights, non_blocking=True)
        if risk is not None:
            st['risk']['rewards'].copy_(risk['rewards'], non_blocking=True)
            if risk['mask'] is None:
                st['risk']['mask'].fill_(True)
            else:
                st['risk']['mask'].copy_(risk['mask'], non_blocking=True)
            self.last_risk = st['risk_out']
        self._send_scalars(coins, seed, self._hyper())
        self.last_loss_parts = st['parts']
        self._works = []
        for g, key in self._graphs:
            g.replay()
            if key == 'hook':
                if getattr(extra_dlogits, 'takes_dst', False):
                    extra_dlogits(*self._hook_sv, dst=st['extra'])         # writes the static buffer itself: no staging copy
                else:
                    st['extra'].copy_(extra_dlogits(*self._hook_sv))
            elif key is not None:
                self._allreduce(key)
        if not self._adam_in_graph:
            self._reduce_guard()
            for w in self._works:
                w.wait()
            # same arithmetic as the captured Adam launch (bias corrections read from the device word the host just wrote),
            # so a segmented step is bit-identical to the single-graph step
            self._clip_grads()
            self._adam(self.t, hyper=st['hyper'])
        # the loss lives in the graphs' static memory: hand out a copy, so losses kept across steps do not alias
        return self._loss.clone()

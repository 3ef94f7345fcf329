"""Test helper: the ordered sequence of calls a path of the host code makes into `ops`, recorded through the kernel emulation.

`TraceEmul` notes every public op call with what the schedule decides about it: the op's name, shape / strides / storage offset /
dtype of every tensor argument (lists, tuples and dicts of tensors included) and the value of every int / float / bool / str
scalar.  `PATHS` names the paths -- public API only, so the same code records a commit and its parent -- and `record_all()` runs
each on fresh, seeded models of the `small_msvd` fixture's config.  A path's entry holds the number of calls, the calls per op
and a SHA-256 of the detailed trace -- the op names in order are part of what is hashed, they are not stored, which keeps the
fixture small (tests/golden/make_launch_traces.py writes it, tests/test_launch_traces.py compares)."""
import hashlib
import json
import random
from collections import OrderedDict

import torch

import dlsg_amd
from dlsg_amd.synth import synth_batch, synth_state_dict
from emul_phrases import PhraseEmul
from emul_sbs import SbsEmul
from helpers import load_case
from test_scst_host import LengthReward
from test_seq_per_clip_host import SeqEmul, captions_for


def describe(x):
    """what a launch depends on in an argument, as JSON-able data"""
    if torch.is_tensor(x):
        return ['T', str(x.dtype).replace('torch.', ''), list(x.shape), list(x.stride()), x.storage_offset()]
    if isinstance(x, (list, tuple)):
        return [describe(v) for v in x]
    if isinstance(x, dict):
        return {str(k): describe(x[k]) for k in sorted(x, key=str)}
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return type(x).__name__


class TraceEmul(SeqEmul, SbsEmul, PhraseEmul):
    """every emulated op (train step, sampling, seq_per_clip, the beam searches: SbsEmul brings the ensemble, group and consensus
    ops with the stochastic step, PhraseEmul the constrained ones, words and phrases); `trace` (a list) collects the calls"""

    trace = None

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        trace = object.__getattribute__(self, '__dict__').get('trace')
        if trace is not None and not name.startswith('_') and callable(v):
            def call(*a, **k):
                trace.append([name, describe(a), describe(k)])
                return v(*a, **k)
            return call
        return v


MODELS = OrderedDict([('capgnn', dlsg_amd.CapGnnModel), ('baseline1', dlsg_amd.CapBaseline1),
                      ('baselinemodel', dlsg_amd.CapBaselineModel)])
DROPOUT = 0.3


def fresh(kind, train=False, beam=1, end_bias=0.0):
    """a new model of `kind` on the small_msvd config with seeded weights, its 3 clips and one caption per clip"""
    args, vocab, g, _ = load_case('small_msvd')
    args.dropout = DROPOUT
    seed, V, B = int(g['meta.seed']), int(g['meta.V']), int(g['meta.B'])
    torch.manual_seed(0)
    net = MODELS[kind](args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), seed)
    sd['decoder.word_restore.bias'][vocab('<end>')] += end_bias
    net.load_state_dict(sd)
    net.set_ops(TraceEmul())
    net.update_beam_size(beam)
    net.train(train)
    frames, regions, caps, lens = synth_batch(args, V, B, seed + 1)
    assert B == 3
    random.seed(3)
    return net, args, vocab, frames, regions, caps, lens


def traced(net, fn):
    net.flatten_parameters_()
    net.ops.trace = []
    fn()
    trace, net.ops.trace = net.ops.trace, None
    return trace


# ---------------------------------------------------------------------------------------------- the paths
def _autograd(kind, tf):
    net, args, vocab, frames, regions, caps, lens = fresh(kind, train=True)

    def run():
        out = net(frames, regions, caps, 26, tf)
        out[0].sum().backward()
    return traced(net, run)


def _nograd(kind):
    net, args, vocab, frames, regions, caps, lens = fresh(kind)

    def run():
        with torch.no_grad():
            net(frames, regions, caps, 26, 1.0)
    return traced(net, run)


def _infer(kind, beam, end_bias=0.0):
    net, args, vocab, frames, regions, caps, lens = fresh(kind, beam=beam, end_bias=end_bias)

    def run():
        with torch.no_grad():
            ids = net(frames, regions, None)[0]
        assert end_bias == 0.0 or ids.shape[1] < 26            # the early exit was taken
    return traced(net, run)


def _trainer(kind, device_coins, n=1, weights=False):
    net, args, vocab, frames, regions, caps, lens = fresh(kind, train=True)
    if n != 1:
        caps, lens = captions_for(args, vocab, 3 * n, 45)
    kw = {}
    if n != 1:
        kw['seq_per_clip'] = n
    if weights:
        kw['seq_weights'] = torch.linspace(-1.0, 1.5, caps.shape[0])
    tr = dlsg_amd.Trainer(net, lr=1e-3, device_coins=device_coins)
    return traced(net, lambda: tr.step(frames, regions, caps, lens, 0.8, **kw))


def _sample(share):
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn', train=True)
    kw = {'share_encoder': True} if share else {}
    return traced(net, lambda: net.sample(frames, regions, n=3, seed=9, **kw))


def _nbest(options):
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn')
    kw = dict(n_best=2, length_penalty=0.7, no_repeat_ngram=2, min_len=2) if options else {}
    return traced(net, lambda: net.beam_search(frames, regions, beam_size=3, **kw))


def _sbs(threshold):
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn')
    kw = dict(temperature=0.7, min_len=2, no_repeat_ngram=2, return_threshold=True) if threshold else {}
    return traced(net, lambda: net.sample_without_replacement(frames, regions, n=3, seed=9, **kw))


def _constrained(options):
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn')
    kw = dict(n_best=2, length_penalty=0.7, no_repeat_ngram=2, min_len=2, return_met=True) if options else {}
    per_clip = [[[5, 6], 7], [], [8]]
    return traced(net, lambda: net.constrained_beam_search(frames, regions, per_clip, beam_size=3, **kw))


def _phrases(options, tensor=False):
    """phrase constraints: a two-word string, a tuple of ids, a list of alternative phrases and an empty clip -- as the per-clip
    lists, or (tensor) as the 4-D tensor `pack_phrases` makes of them"""
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn')
    kw = dict(n_best=2, length_penalty=0.7, no_repeat_ngram=2, min_len=2, return_met=True) if options else {}
    w = vocab.idx2word
    cons = [['%s %s' % (w[5], w[6]), (7, 8, 9)], [], [[(10, 11), w[12], '%s %s' % (w[13], w[5])]]]
    if tensor:
        cons = dlsg_amd.pack_phrases(cons, vocab)
    return traced(net, lambda: net.constrained_beam_search(frames, regions, cons, beam_size=3, **kw))


def _ensemble(groups):
    """the three model classes as one ensemble on one traced op set"""
    nets = [fresh(kind) for kind in MODELS]
    frames, regions = nets[0][3:5]
    for member in nets[1:]:
        member[0].set_ops(nets[0][0].ops)
        member[0].flatten_parameters_()
    ens = dlsg_amd.Ensemble([member[0] for member in nets], weights=[0.5, 0.3, 0.2], mode='logprob' if groups else 'prob')
    kw = dict(num_groups=2, diversity_penalty=0.5) if groups else {}
    return traced(nets[0][0], lambda: ens.beam_search(frames, regions, beam_size=4, n_best=2, length_penalty=0.7, no_repeat_ngram=2,
                                                      min_len=2, **kw))


def _decoder(kind, mode, feats2, step):
    """Decoder.forward on its own: mode 'tf' (train mode, scheduled sampling), 'greedy' or 'beam'"""
    net, args, vocab, frames, regions, caps, lens = fresh(kind, train=mode == 'tf', beam=3 if mode == 'beam' else 1)
    gen = torch.Generator().manual_seed(5)
    H = args.visual_hidden_size
    f1 = torch.randn(3, args.num_proposals, H, generator=gen)
    f2 = torch.randn(3, args.num_proposals, H, generator=gen) if feats2 else None
    G = H * (2 if feats2 else 1)
    sf = torch.randn(3, G, generator=gen) if step else None
    captions = caps if mode == 'tf' else None
    L = None if mode == 'beam' else 26
    return traced(net, lambda: net.decoder(f1, captions, L, 0.8, cnn_feats_2=f2, step_feats=sf))


def _scst(baseline, share):
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn', train=True)
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=3, baseline=baseline, share_encoder=share, lr=1e-3)
    return traced(net, lambda: tr.step(frames, regions, ['0', '1', '2']))


def _paths():
    P = OrderedDict()
    for kind in MODELS:
        for tf in (1.0, 0.5):
            P['%s/autograd_tf%.1f' % (kind, tf)] = lambda kind=kind, tf=tf: _autograd(kind, tf)
        P['%s/nograd_forward' % kind] = lambda kind=kind: _nograd(kind)
        P['%s/greedy' % kind] = lambda kind=kind: _infer(kind, 1)
        P['%s/beam3' % kind] = lambda kind=kind: _infer(kind, 3)
        P['%s/beam3_early_exit' % kind] = lambda kind=kind: _infer(kind, 3, end_bias=30.0)
        for dc in (False, True):
            P['%s/trainer_step_%s_coins' % (kind, 'device' if dc else 'host')] = lambda kind=kind, dc=dc: _trainer(kind, dc)
    for n, w in ((3, False), (1, True), (3, True)):
        P['capgnn/trainer_step_n%d%s' % (n, '_weighted' if w else '')] = lambda n=n, w=w: _trainer('capgnn', False, n, w)
    for share in (False, True):
        P['capgnn/sample_n3%s' % ('_shared' if share else '')] = lambda share=share: _sample(share)
    for opt in (True, False):
        P['capgnn/beam_search_%s' % ('options' if opt else 'plain')] = lambda opt=opt: _nbest(opt)
    for flag in (False, True):
        P['capgnn/sample_without_replacement%s' % ('_threshold' if flag else '')] = lambda flag=flag: _sbs(flag)
        P['capgnn/constrained_beam_search_%s' % ('options' if flag else 'plain')] = lambda flag=flag: _constrained(flag)
        P['ensemble/beam_search%s' % ('_groups' if flag else '')] = lambda flag=flag: _ensemble(flag)
    for flag in (False, True):
        P['capgnn/constrained_beam_search_phrases_%s' % ('options' if flag else 'plain')] = lambda flag=flag: _phrases(flag)
    P['capgnn/constrained_beam_search_phrases_tensor'] = lambda: _phrases(False, tensor=True)
    for kind, feats2 in (('capgnn', True), ('baseline1', False)):
        for step in (False, True):
            for mode in ('tf', 'greedy', 'beam'):
                P['%s/decoder_%s%s' % (kind, mode, '_stepfeats' if step else '')] = \
                    lambda kind=kind, feats2=feats2, step=step, mode=mode: _decoder(kind, mode, feats2, step)
    for baseline in ('mean', 'greedy'):
        for share in (False, True):
            P['capgnn/scst_%s%s' % (baseline, '_shared' if share else '')] = lambda b=baseline, s=share: _scst(b, s)
    return P


PATHS = _paths()


def summarise(trace):
    names = [c[0] for c in trace]
    counts = OrderedDict((nm, names.count(nm)) for nm in sorted(set(names)))
    digest = hashlib.sha256(json.dumps(trace, sort_keys=True).encode()).hexdigest()
    return OrderedDict([('calls', len(names)), ('sha256', digest), ('counts', counts)])


def record_all(only=None):
    return OrderedDict((name, summarise(fn())) for name, fn in PATHS.items() if only is None or name in only)

"""CPU: `Ensemble.sample` (`beam.ensemble_sample`, `EnsembleSampleGraph`, `dlsg_amd.sample`) through the emulated kernels -- the
sampled word step of an ensemble is tests/emul_ens_sample.py, by composition of the existing emulators.  What the draw promises
about its captions, which op a word launches, the controls, the refusals, the captured form.  The members are the three of
tests/test_ensemble_host.py: two CapGnnModels of different hidden sizes and a CapBaseline1.  The GPU side is
tests/test_gpu_ens_sample.py."""
import functools

import pytest
import torch

import dlsg_amd
from dlsg_amd import graphs
from dlsg_amd.beam import exclusions_hit, pack_exclusions
from emul_ens_sample import EnsSampleEmul
from helpers import small_args
from test_ensemble_host import build_members
from test_sample_filter_host import repeated_bigrams

CLIPS, N, SEED = 4, 3, 21
WEIGHTS = {'prob': [0.5, 0.3, 0.2], 'logprob': [1.0, 2.0, 1.0]}


def ensemble(mode='prob', members=slice(None)):
    nets, frames, regions = build_members(ops=EnsSampleEmul())
    nets = nets[members]
    return dlsg_amd.Ensemble(nets, WEIGHTS[mode][members], mode), frames[:CLIPS], regions[:CLIPS]


@functools.lru_cache(maxsize=None)
def drawn(mode, seed):
    """one plain draw of the three-member ensemble (computed once per setting, never modified)"""
    ens, frames, regions = ensemble(mode)
    return ens.sample(frames, regions, n=N, seed=seed)


@pytest.mark.parametrize('mode', ['prob', 'logprob'])
def test_shapes_lengths_and_seeds(mode):
    ens, frames, regions = ensemble(mode)
    L, end = ens.decoder.max_words, ens.decoder.vocab('<end>')
    ids, logp, lens = drawn(mode, SEED)
    assert ids.shape == (CLIPS * N, L) and logp.shape == (CLIPS * N, L) and lens.shape == (CLIPS * N,)
    assert ids.dtype == torch.int64 and logp.dtype == torch.float32 and lens.dtype == torch.int64
    assert ids.is_contiguous() and logp.is_contiguous()
    for r in range(CLIPS * N):
        hits = (ids[r] == end).nonzero()
        assert int(lens[r]) == (int(hits[0]) + 1 if len(hits) else L)
    assert (lens < L).any() and (logp <= 0).all() and torch.isfinite(logp).all()
    again = ens.sample(frames, regions, n=N, seed=SEED)
    assert all(torch.equal(a, b) for a, b in zip(again, (ids, logp, lens)))
    assert not torch.equal(drawn(mode, SEED + 1)[0], ids)
    for b in range(CLIPS):                                             # the n rows of a clip are streams of their own
        assert not all(torch.equal(ids[b * N], ids[b * N + i]) for i in range(1, N)), b
    # the function form is the object's own sampler
    assert torch.equal(dlsg_amd.sample(ens, frames, regions, n=N, seed=SEED)[0], ids)


def test_the_two_modes_draw_from_different_distributions():
    assert not torch.equal(drawn('prob', SEED)[1], drawn('logprob', SEED)[1])


def test_seed_none_draws_the_first_members_next_seed():
    ens, frames, regions = ensemble()
    first = ens.members[0]
    c0, others = first.seed_counter, [m.seed_counter for m in ens.members[1:]]
    got = ens.sample(frames, regions, n=2)
    want_seed = (0x5DEECE66D * (c0 + 1) + 0xB) & 0xFFFFFFFFFFFF
    assert first.seed_counter > c0
    want = ens.sample(frames, regions, n=2, seed=want_seed)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(ens.sample(frames, regions, n=2)[0], got[0])         # the next call draws the next seed
    assert all(m.seed_counter > c for m, c in zip(ens.members[1:], others))     # (their encoders drew their own)


def test_one_sample_ens_per_word_and_no_other_word_choice():
    ens, frames, regions = ensemble()
    L = ens.decoder.max_words
    ex = pack_exclusions(ens.decoder.vocab, words=[10])
    for opts in (dict(), dict(top_k=3, top_p=0.8, min_len=2, no_repeat_ngram=2), dict(exclude=ex), dict(temperature=0.0)):
        ens.ops.recording = []
        ens.sample(frames, regions, n=N, seed=SEED, **opts)
        log, ens.ops.recording = ens.ops.recording, None
        assert log.count('sample_ens') == L, opts
        choosers = [name for name in set(log) if name.startswith(('sample_', 'beam_select', 'argmax', 'select_embed'))]
        assert choosers == ['sample_ens'], (opts, choosers)
        # every member steps on R = CLIPS * N rows: one state gather and one embedding per member and word
        assert log.count('embed_fwd') == 3 * L and log.count('gather_rows_multi') == 3 * (L - 1), opts


def test_exclusions_never_appear():
    ens, frames, regions = ensemble()
    vocab = ens.decoder.vocab
    plain = drawn('prob', SEED)
    common = torch.bincount(plain[0].flatten(), minlength=len(vocab)).topk(4)[1].tolist()
    common = [w for w in common if w != vocab('<end>')][:3]
    shared = pack_exclusions(vocab, words=common[:2], bad_endings=True)
    clipped = pack_exclusions(vocab, per_clip=[[common[0]], [common[1]], [], [(common[0], common[1]), common[2]]])
    assert int(exclusions_hit(plain[0].view(CLIPS, N, -1), plain[2].view(CLIPS, N), shared).sum()) > 0
    assert int(exclusions_hit(plain[0].view(CLIPS, N, -1), plain[2].view(CLIPS, N), clipped).sum()) > 0
    for ex in (shared, clipped):
        ids, logp, lens, kept = ens.sample(frames, regions, n=N, seed=SEED, exclude=ex, return_kept=True)
        assert int(exclusions_hit(ids.view(CLIPS, N, -1), lens.view(CLIPS, N), ex).sum()) == 0
        assert torch.isfinite(logp).all() and (kept < len(vocab)).any() and (kept >= 1).all()
    # a per-clip table is indexed by clip, not by caption row
    rows = pack_exclusions(vocab, per_clip=[[10]] * (CLIPS * N))
    with pytest.raises(ValueError, match='holds %d clips, the batch %d' % (CLIPS * N, CLIPS)):
        ens.sample(frames, regions, n=N, exclude=rows)


def test_min_len_and_no_repeat_ngram_hold():
    ens, frames, regions = ensemble()
    L, end = ens.decoder.max_words, ens.decoder.vocab('<end>')
    assert (drawn('prob', SEED)[2] <= 6).any()
    ids, logp, lens = ens.sample(frames, regions, n=N, seed=SEED, min_len=6)
    assert (lens > 6).all() and (ids[:, :6] != end).all() and torch.isfinite(logp).all()
    sharp = ens.sample(frames, regions, n=N, seed=SEED, temperature=0.25, min_len=L - 1)
    assert repeated_bigrams(sharp[0], sharp[2])                        # sharp sampling loops without the control
    ids, logp, lens, kept = ens.sample(frames, regions, n=N, seed=SEED, temperature=0.25, min_len=L - 1, no_repeat_ngram=2,
                                       return_kept=True)
    assert repeated_bigrams(ids, lens) == [] and torch.isfinite(logp).all()
    assert (kept < len(ens.decoder.vocab) - 1).any()


@pytest.mark.parametrize('mode', ['prob', 'logprob'])
def test_top_k_one_is_temperature_zero_is_greedy(mode):
    ens, frames, regions = ensemble(mode)
    cold = ens.sample(frames, regions, n=N, temperature=0.0, seed=SEED)
    one = ens.sample(frames, regions, n=N, seed=SEED + 5, top_k=1, return_kept=True)
    assert torch.equal(one[0], cold[0]) and torch.equal(one[2], cold[2])
    assert (one[1] == 0).all() and (one[3] == 1).all() and one[3].dtype == torch.int32 and one[3].shape == one[0].shape
    greedy = ens.greedy(frames, regions)
    for r in range(CLIPS * N):
        n = int(cold[2][r])
        assert cold[0][r, :n].tolist() == greedy[r // N, :n].tolist(), r
    assert (cold[2] < ens.decoder.max_words).any()


def test_what_is_refused():
    ens, frames, regions = ensemble()
    E = dlsg_amd.EnsembleSampleNotCovered
    assert issubclass(E, ValueError)
    ens.ops.recording = []
    with pytest.raises(E, match='prefix and Ensemble.sample'):
        ens.sample(frames, regions, prefix=[['a']] * CLIPS)
    with pytest.raises(E, match='share_encoder and Ensemble.sample'):
        ens.sample(frames, regions, share_encoder=True)
    with pytest.raises(E, match='share_encoder and Ensemble.sample'):
        dlsg_amd.sample(ens, frames, regions, share_encoder=False)
    with pytest.raises(E, match='prefix and Ensemble.sample'):
        dlsg_amd.EnsembleSampleGraph(ens, frames, regions, N, prefix=torch.zeros(CLIPS, 1, dtype=torch.int64))
    with pytest.raises(TypeError):
        ens.sample(frames, regions, beam_size=3)
    L = ens.decoder.max_words
    for bad in (dict(n=0), dict(n=1.5), dict(temperature=-1.0), dict(temperature=float('nan')), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(min_len=L + 1), dict(no_repeat_ngram=-1), dict(exclude=[10])):
        with pytest.raises(ValueError):
            ens.sample(frames, regions, **bad)
    assert ens.ops.recording == []                                     # refused before any encoder ran
    ens.ops.recording = None
    with pytest.raises(ValueError, match='an Ensemble in SCSTTrainer'):
        dlsg_amd.SCSTTrainer(ens, None)

    class OldOps(EnsSampleEmul):
        """an ops object written before the step existed"""
        def __getattribute__(self, name):
            if name == 'sample_ens':
                raise AttributeError(name)
            return super().__getattribute__(name)
    for m in ens.members:
        m.set_ops(OldOps())
    with pytest.raises(E, match='OldOps has no sample_ens'):
        ens.sample(frames, regions)
    # captions longer than the step's history
    long_nets = [dlsg_amd.CapGnnModel(small_args(dropout=0.0, max_words=65), dlsg_amd.make_vocab(50)).eval().set_ops(EnsSampleEmul())]
    with pytest.raises(ValueError, match='max_words 65'):
        dlsg_amd.Ensemble(long_nets).sample(frames, regions)


def test_a_baseline_member_alone_samples():
    """the eval-mode sampler the baseline classes lack: their own `.sample` still raises"""
    ens, frames, regions = ensemble(members=slice(2, 3))
    net = ens.members[0]
    assert isinstance(net, dlsg_amd.CapBaseline1)
    with pytest.raises(NotImplementedError):
        net.sample(frames, regions)
    ids, logp, lens = ens.sample(frames, regions, n=N, seed=SEED)
    L = ens.decoder.max_words
    assert ids.shape == (CLIPS * N, L) and torch.isfinite(logp).all() and not torch.equal(ids[0], ids[1])
    cold = ens.sample(frames, regions, temperature=0.0)
    greedy = net.beam_search(frames, regions, beam_size=1, n_best=1)[0][:, 0]
    for b in range(CLIPS):
        assert cold[0][b, :int(cold[2][b])].tolist() == greedy[b, :int(cold[2][b])].tolist()
    # one member of weight 1: logp is the member's own log-softmax of the drawn word
    tok = ens.score(frames, regions, ids.view(CLIPS, N, L), return_tokens=True)[2].view(CLIPS * N, L)
    for r in range(CLIPS * N):
        n = int(lens[r])
        assert torch.allclose(logp[r, :n], tok[r, :n], rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------------------------- the graph class
class Rerun(object):
    """stands in for a captured graph: a replay runs the body again and copies what it returns into the first run's tensors"""

    def __init__(self, body, out):
        self.body, self.out = body, out

    def replay(self):
        for dst, src in zip(self.out, self.body()):
            dst.copy_(src)


def fake_capture(dev, body, warmup=None):
    out = body()
    return Rerun(body, out), out


def test_the_graph_replays_the_eager_bits(monkeypatch):
    monkeypatch.setattr(graphs, 'capture', fake_capture)
    ens, frames, regions = ensemble('logprob')
    ex = pack_exclusions(ens.decoder.vocab, words=[10, 11])
    opts = dict(top_k=8, min_len=2, return_kept=True)
    g = dlsg_amd.EnsembleSampleGraph(ens, frames, regions, N, 0.8, exclude=ex, **opts)
    assert g.options == opts and g.n == N and g.temperature == 0.8 and g.seed.dtype == torch.int64 and g.seed.shape == (1,)
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(g.exclude, ex) if a is not None)
    assert [m for m, _, _ in g.held] == ens.members and g.valid_for(frames, regions)
    for seed in (SEED, SEED + 1):
        want = ens.sample(frames, regions, N, 0.8, seed, exclude=ex, **opts)
        got = g(frames, regions, seed)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want)), seed
    # the graph's own table is what the next replay bans
    g.exclude.shared.copy_(torch.tensor([[12], [13]]))
    want = ens.sample(frames, regions, N, 0.8, SEED, exclude=pack_exclusions(ens.decoder.vocab, words=[12, 13]), **opts)
    assert torch.equal(g(frames, regions, SEED)[0], want[0])
    # validity covers every member's arena and mode
    ens.members[2].train()
    assert not g.valid_for(frames, regions)
    ens.members[2].eval()
    assert g.valid_for(frames, regions) and not g.valid_for(frames[:2], regions[:2])
    with pytest.raises(TypeError):
        g(frames, regions)


# ---------------------------------------------------------------------------------------------- the entry point's header
def test_the_extension_header_is_read_bound_and_documented():
    """include/dlsg_sample_ens.h is held to what tests/test_abi.py holds include/dlsg.h to: two independent readings agree, the
    library exports the symbol with the derived prototype, INTEGRATION.md names it; dlsg.h's own list and version are as they were"""
    import os
    import re
    from dlsg_amd import abi, hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'dlsg_sample_ens.h')).read(), flags=re.S)
    names = sorted(set(re.findall(r'\b(?:int|int64_t)\s+(dlsg_\w+)\s*\(', txt)))
    assert names == ['dlsg_sample_ens'] == sorted(abi.extensions) and not set(abi.extensions) & set(abi.functions)
    assert abi.EXTENSION_HEADERS == ('dlsg_sample_ens.h',) and abi.defines['DLSG_ABI_VERSION'] == 8
    restype, argtypes = abi.extensions['dlsg_sample_ens']
    params = re.search(r'dlsg_sample_ens\s*\(([^()]*)\)', txt).group(1).split(',')
    assert len(argtypes) == len(params) == 33 and restype is abi.SCALARS['int']
    # the members as dlsg_beam_select_ens takes them, then the arguments of dlsg_sample_excl_embed without E, out, ldo, W, p, site_word
    ens, excl = abi.functions['dlsg_beam_select_ens'][1], abi.functions['dlsg_sample_excl_embed'][1]
    assert argtypes[:6] == ens[1:7] and len(argtypes) == 6 + 1 + len(excl) - 8
    lib = hip.load_library()
    assert lib.dlsg_sample_ens.argtypes == argtypes and lib.dlsg_sample_ens.restype is restype
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    assert 'dlsg_sample_ens' in doc and 'include/dlsg_sample_ens.h' in doc
    with pytest.raises(ValueError, match='line 1'):
        abi.parse('float dlsg_bad(void);')

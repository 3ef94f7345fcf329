"""CPU: ensemble beam search (`dlsg_amd.Ensemble`, `beam.ensemble_nbest`) through the emulated kernels (tests/emul_ensemble.py)
against the restated search of tests/test_beam_nbest_host.py driven by an ensemble step: every member's oracle decode step on the
shared words, the members' log-probs combined in float64.  The GPU side is tests/test_gpu_ensemble.py, which imports the case
from here."""
import functools
import math

import pytest
import torch

import dlsg_amd
from dlsg_amd.hip import normalised_weights
from dlsg_amd.synth import synth_state_dict, synth_batch
from emul_ensemble import EnsembleEmul
from helpers import load_case, weights_and_inputs, small_args
from test_beam_nbest_host import MODELS, close, has_repeat, oracle_stepper, reference_rank, reference_search, words_of

NEAR_TIE = 2e-3                                     # tests/test_gpu_beam_nbest.py: the two sides' logits differ by up to 1e-3
SEED, CLIPS, K, G, MIN_LEN, ALPHA = 15, 8, 3, 2, 4, 0.7
SETTINGS = {'prob': [1.0, 1.0, 1.0], 'logprob': [0.5, 0.3, 0.2]}
OPTS = dict(beam_size=K, length_penalty=ALPHA, no_repeat_ngram=G, min_len=MIN_LEN)


def member_specs():
    return [('capgnn', small_args(dropout=0.0), SEED),
            ('capgnn', small_args(dropout=0.0, decode_hidden_size=80, query_hidden_size=32), SEED + 1000),
            ('baseline1', small_args(dropout=0.0), SEED + 2000)]


def build_members(ops=None, oracles=False):
    """the three members of the case (two CapGnnModels of different hidden sizes and a CapBaseline1, vocabulary 50, <end> lifted by
    1.0) and the eight clips: (nets or oracles, frames, regions)"""
    vocab = dlsg_amd.make_vocab(50)
    out = []
    for kind, args, seed in member_specs():
        torch.manual_seed(0)
        net = MODELS[kind][0](args, vocab).eval()
        sd = synth_state_dict(net.state_dict(), seed)
        sd['decoder.word_restore.bias'][net.decoder.vocab('<end>')] += 1.0
        if oracles:
            net = MODELS[kind][1](args, vocab).eval()
        net.load_state_dict(sd)
        if ops is not None:
            net.set_ops(ops)
        out.append(net)
    frames, regions, _, _ = synth_batch(member_specs()[0][1], 50, CLIPS, SEED + 1)
    return out, frames, regions


def ensemble_stepper(orcs, weights, mode, frames, regions):
    """`oracle_stepper` of an ensemble: every member's step on the shared `last`, the members' states under prefixed keys
    (`reference_search` reorders every state tensor by the same parent rows), the combined log-probs in float64 -> float32"""
    parts = [oracle_stepper(o, frames, regions) for o in orcs]
    w = normalised_weights(weights)

    def step_fn(last, st):
        new, logp = {}, []
        for i, part in enumerate(parts):
            pre = 'm%d.' % i
            lp, s = part[0](last, {key[len(pre):]: v for key, v in st.items() if key.startswith(pre)})
            logp.append(lp.double())
            new.update({pre + key: v for key, v in s.items()})
        if mode == 'prob':
            c = torch.logsumexp(torch.stack([l + math.log(wm) for l, wm in zip(logp, w)]), 0)
        else:
            c = sum(wm * l for l, wm in zip(logp, w))
        return c.float(), new

    state = {'m%d.%s' % (i, key): v for i, part in enumerate(parts) for key, v in part[2].items()}
    return (step_fn,) + parts[0][1:2] + (state,) + parts[0][3:]


def searched(step):
    step_fn, start, state, end, L = step
    toks, lps, gap = reference_search(step_fn, start, state, end, L, K, G, MIN_LEN)
    ids, sc, lens, rank_gap = reference_rank(toks, lps, end, ALPHA, K)
    return ids, sc, lens, [min(a, b) for a, b in zip(gap, rank_gap)], end, L


@functools.lru_cache(maxsize=None)
def restated(setting):
    """the restated ensemble search of a setting (computed once, never modified): ids, scores, lens, gap per clip, end, L"""
    orcs, frames, regions = build_members(oracles=True)
    return searched(ensemble_stepper(orcs, SETTINGS[setting], setting, frames, regions))


@functools.lru_cache(maxsize=None)
def restated_members():
    """every member's own restated search: [ids per member]"""
    orcs, frames, regions = build_members(oracles=True)
    return [searched(oracle_stepper(o, frames, regions))[0] for o in orcs]


def kept(setting):
    return [b for b in range(CLIPS) if restated(setting)[3][b] >= NEAR_TIE]


def check_against_restated(setting, ids, scores, lens):
    """what both the emulated and the HIP search owe the restatement: kept clips exact (scores to 1e-4), every clip well-formed"""
    want_ids, want_sc, want_len, gap, end, L = restated(setting)
    assert ids.shape == (CLIPS, K, L) and scores.shape == (CLIPS, K) and lens.shape == (CLIPS, K)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and lens.dtype == torch.int64
    keep = kept(setting)
    assert len(keep) >= 7
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b], b
        close(scores[b].numpy(), want_sc[b], 1e-4)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    for row in ids.view(-1, L).tolist():
        words = words_of(row, end)
        assert not has_repeat(words, G) and len(words) >= MIN_LEN, row
        assert all(w == end for w in row[len(words):])


@functools.lru_cache(maxsize=None)
def emulated(setting):
    nets, frames, regions = build_members(ops=EnsembleEmul())
    return dlsg_amd.Ensemble(nets, SETTINGS[setting], setting).beam_search(frames, regions, **OPTS)


# ---------------------------------------------------------------------------------------------- tests
def test_restated_case_is_decisive_and_an_ensemble():
    """on the restatement alone: at most one clip in eight is a near-tie, the captions have several lengths, the ensemble's best
    caption is not a member's in at least half of the clips, and the two settings differ in at least half"""
    own = restated_members()
    for setting in SETTINGS:
        ids, _, lens, gap, end, L = restated(setting)
        print(setting, 'smallest gaps', ['%.1e' % x for x in gap], 'lengths', sorted({l for c in lens for l in c}))
        assert len(kept(setting)) >= 7
        assert len({l for c in lens for l in c}) > 2
        for m, mine in enumerate(own):
            differ = sum(ids[b][0] != mine[b][0] for b in range(CLIPS))
            print(setting, 'member', m, 'top caption differs in', differ)
            assert 2 * differ >= CLIPS, (setting, m, differ)
    differ = sum(restated('prob')[0][b][0] != restated('logprob')[0][b][0] for b in range(CLIPS))
    assert 2 * differ >= CLIPS, differ


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_ensemble_matches_the_restated_search(setting):
    check_against_restated(setting, *emulated(setting))


def golden_member(tag, ops):
    args, vocab, g, kind = load_case(tag)
    torch.manual_seed(0)
    net = MODELS[kind][0](args, vocab).eval()
    net.set_ops(ops)
    sd, frames, regions, _, _ = weights_and_inputs(net, g, args)
    net.load_state_dict(sd)
    return net, frames, regions


@pytest.mark.parametrize('opts', [dict(beam_size=5), dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=2, min_len=4)])
@pytest.mark.parametrize('mode', ['prob', 'logprob'])
@pytest.mark.parametrize('tag', ['small_msvd', 'small_baseline1'])
def test_one_member_is_the_models_own_search(tag, mode, opts):
    net, frames, regions = golden_member(tag, EnsembleEmul())
    want = net.beam_search(frames, regions, **opts)
    got = dlsg_amd.Ensemble([net], mode=mode).beam_search(frames, regions, **opts)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    close(got[1].numpy(), want[1].numpy(), 1e-6)


def test_the_public_forms_agree():
    """n_best is a prefix of the ranking; greedy is the one-beam row; calling the ensemble gives the best beam at the first
    member's beam size; no member's beam size changes"""
    nets, frames, regions = build_members(ops=EnsembleEmul())
    ens = dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob')
    assert ens.members == nets and ens.mode == 'prob' and ens.decoder is nets[0].decoder and ens.ops is nets[0].ops
    assert ens.weights == [1.0 / 3] * 3 and dlsg_amd.Ensemble(nets).weights == ens.weights
    assert dlsg_amd.Ensemble(nets, [2, 1, 1], 'logprob').weights == [0.5, 0.25, 0.25]
    full = emulated('prob')
    ids, scores, lens = ens.beam_search(frames, regions, n_best=2, **OPTS)
    assert ids.is_contiguous() and ids.shape[:2] == (CLIPS, 2)
    assert torch.equal(ids, full[0][:, :2]) and torch.equal(scores, full[1][:, :2]) and torch.equal(lens, full[2][:, :2])
    L = nets[0].decoder.max_words
    one = ens.beam_search(frames, regions, beam_size=1, n_best=1)[0][:, 0]
    assert torch.equal(ens.greedy(frames, regions), one) and one.shape == (CLIPS, L)
    out = ens(frames, regions, None)
    assert len(out) == 4 and torch.equal(out[0], ens.beam_search(frames, regions, n_best=1)[0][:, 0])
    assert torch.equal(out[0], ens.beam_search(frames, regions, beam_size=5, n_best=1)[0][:, 0])      # small_args' own beam size
    assert not torch.equal(out[0], one)
    assert [n.decoder.beam_size for n in nets] == [5, 5, 5]
    with pytest.raises(ValueError):
        ens(frames, regions, torch.zeros(CLIPS, L, dtype=torch.long))


def test_gather_results_takes_an_ensemble():
    from dlsg_amd import scoring as S
    nets, frames, regions = build_members(ops=EnsembleEmul())
    ens = dlsg_amd.Ensemble(nets[:2], [0.6, 0.4], 'logprob')
    f, r = frames[:3], regions[:3]
    loader = [(f, r, None, ['v0', 'v1', 'v2'])]
    opts = dict(beam_size=3, no_repeat_ngram=2, min_len=4, length_penalty=0.7)
    got = S.gather_results(ens, loader, decode=opts)
    ids = ens.beam_search(f, r, n_best=1, **opts)[0][:, 0]
    assert got == {'v%d' % i: ens.decoder.decode_tokens(ids[i]) for i in range(3)}
    plain = S.gather_results(ens, loader)
    assert plain == {'v%d' % i: ens.decoder.decode_tokens(row) for i, row in enumerate(ens(f, r, None)[0])}
    assert plain != got


def test_value_errors():
    nets, frames, regions = build_members(ops=EnsembleEmul())
    E = dlsg_amd.Ensemble
    other = dlsg_amd.CapGnnModel(small_args(dropout=0.0), dlsg_amd.make_vocab(51))
    renamed = dlsg_amd.CapGnnModel(small_args(dropout=0.0), dlsg_amd.make_vocab(50))
    v = renamed.decoder.vocab
    a, b = v.idx2word[10], v.idx2word[11]
    v.idx2word[10], v.idx2word[11], v.word2idx[a], v.word2idx[b] = b, a, 11, 10             # same length, two words swapped
    longer = dlsg_amd.CapGnnModel(small_args(dropout=0.0, max_words=20), dlsg_amd.make_vocab(50))
    assert longer.decoder.max_words != nets[0].decoder.max_words
    meta = dlsg_amd.CapGnnModel(small_args(dropout=0.0), dlsg_amd.make_vocab(50)).to('meta')
    for bad in (lambda: E([]), lambda: E(nets * 3), lambda: E([nets[0], other]), lambda: E([nets[0], renamed]),
                lambda: E([nets[0], longer]), lambda: E([nets[0], meta]), lambda: E(nets, [1.0, 1.0]), lambda: E(nets, [1.0, 0.0, 1.0]),
                lambda: E(nets, [1.0, -1.0, 1.0]), lambda: E(nets, [1.0, float('inf'), 1.0]), lambda: E(nets, [1.0, float('nan'), 1.0]),
                lambda: E(nets, mode='mean')):
        with pytest.raises(ValueError):
            bad()
    assert len(E(nets * 2 + nets[:2]).members) == 8
    ens = E(nets)
    L = nets[0].decoder.max_words
    for bad in (dict(n_best=6), dict(n_best=0), dict(beam_size=9), dict(no_repeat_ngram=-1), dict(min_len=-1), dict(min_len=L),
                dict(beam_size=3, n_best=4)):
        with pytest.raises(ValueError):
            ens.beam_search(frames, regions, **bad)
    tiny = [dlsg_amd.CapGnnModel(small_args(dropout=0.0), dlsg_amd.make_vocab(6)).eval().set_ops(EnsembleEmul())]
    with pytest.raises(ValueError, match='too small'):
        E(tiny).beam_search(frames, regions, beam_size=7)

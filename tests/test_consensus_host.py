"""CPU: consensus (minimum Bayes risk) reranking -- `CiderD.pairwise` / `consensus` against the scorer's own `_score`, the numpy
restatement of the kernel (tests/emul_consensus.py) on id rows against them on the decoded strings, ordering and validity, and the
public forms (`consensus_rerank`, `consensus_search`, `gather_results(decode=dict(consensus=...))`) through the emulated ops on
the small host model of tests/test_groups_host.py.  The GPU side is tests/test_gpu_consensus.py."""
import math
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.scoring import _ngrams
from emul_consensus import ConsensusEmul, emul_cider_consensus
from test_beam_nbest_host import synth_pair
from test_cider_device_host import corpus_for, host_words, random_corpus, vocab_of
from test_ensemble_host import SETTINGS, build_members

TOL = dict(rtol=1e-12, atol=1e-12)


def host_consensus(dc, ids, scores=None, temperature=1.0):
    """`CiderD.pairwise` / `consensus` per clip on the decoded strings of ids (B, n, L): (util, expected, order) numpy arrays"""
    ids = ids.cpu()
    U, E, O = [], [], []
    for b in range(ids.shape[0]):
        hyps = [host_words(dc.vocab, r, dc.end_id) for r in ids[b].tolist()]
        U.append(dc.cider.pairwise(hyps))
        o, e = dc.cider.consensus(hyps, None if scores is None else scores[b].cpu().numpy(), temperature)
        E.append(e)
        O.append(o)
    return np.stack(U), np.stack(E), np.stack(O)


def check_order(expected, order):
    """order is a permutation that sorts expected descending, equal values in index order"""
    expected, order = np.asarray(expected), np.asarray(order)
    for e, o in zip(expected, order):
        assert sorted(o.tolist()) == list(range(len(e)))
        for a, b in zip(o[:-1], o[1:]):
            assert e[a] > e[b] or (e[a] == e[b] and a < b), (e.tolist(), o.tolist())


def near_duplicates(vocab, refs, rng, B, n, L, special=True):
    """(B, n, L) id rows: the candidates of a clip share a stem (a reference with words swapped) and differ in their last words, so
    most pairs share n-grams; with `special` (and room for it) clip 0 gets two identical candidates, one empty, one without <end>,
    and clip 1 ids outside the vocabulary"""
    V, end = len(vocab), vocab('<end>')
    rows = []
    vids = sorted(refs)
    for b in range(B):
        stem = [vocab(w) for w in rng.choice(refs[vids[b % len(vids)]]).split()][:max(L - 3, 1)]
        if len(stem) < 2:
            stem = [rng.randrange(V // 2, V)]                         # a rare word (idf > 0), swapped in one candidate of five only
        clip = []
        for i in range(n):
            ws = list(stem)
            for _ in range(1 + i % 3 if len(stem) > 1 else i % 5 == 4):
                ws[-1 - rng.randrange(min(3, len(ws)))] = rng.randrange(4, min(V, 40))
            if i % 4 == 3:
                ws = ws + [rng.randrange(4, min(V, 40))]
            clip.append((ws + [end] + [rng.randrange(V) for _ in range(L)])[:L])
        rows.append(clip)
    if special and n >= 2:
        rows[0][1] = list(rows[0][0])
    if special and n >= 5:
        rows[0][2] = [end] + rows[0][2][1:]
        rows[0][3] = [w if w != end else 5 for w in rows[0][3]]
        for i, bad in enumerate([-1, V, 1 << 40, -(1 << 62)]):
            rows[1][i][i % min(L, 4)] = bad
            rows[1][i + 1][(i + 1) % min(L, 4)] = bad
            if L > 6:
                rows[1][i][5] = bad                                   # an n-gram that ends in the word, one that starts with it
    return torch.tensor(rows, dtype=torch.int64)


def small_scorer(n=4, seed=0):
    rng = random.Random(seed)
    words = ['w%d' % i for i in range(14)]
    refs = random_corpus(rng, 9, 5, words)
    vocab = vocab_of(words[:11])                          # w11..w13 appear in references only
    return S.DeviceCiderD(refs, vocab, n=n, device='cpu'), refs, vocab, rng


# ------------------------------------------------------------------------------------------------ the host scorer
@pytest.mark.parametrize('n', [1, 4])
def test_pairwise_is_the_score_against_a_single_reference(n):
    dc, refs, vocab, rng = small_scorer(n)
    cd = dc.cider
    hyps = [' '.join(rng.choice(['w%d' % i for i in range(12)]) for _ in range(rng.randint(1, 9))) for _ in range(6)] + ['']
    hyps[3] = hyps[1]
    U = cd.pairwise(hyps)
    assert U.shape == (7, 7) and U.dtype == np.float64
    for j, hj in enumerate(hyps):
        cd.ref_vecs['scratch'] = [cd._vec(_ngrams(hj.split(), n))]
        for i, hi in enumerate(hyps):
            assert abs(U[i, j] - cd._score('scratch', hi)) <= 1e-12, (i, j)
    assert (U[:6, :6] > 0).sum() > 18 and not np.allclose(U, U.T, rtol=0, atol=1e-9) and (U[6] == 0).all() and (U[:, 6] == 0).all()
    # uniform consensus: the score against the list of all the others
    order, expected = cd.consensus(hyps)
    for i, hi in enumerate(hyps):
        cd.ref_vecs['scratch'] = [cd._vec(_ngrams(h.split(), n)) for j, h in enumerate(hyps) if j != i]
        assert abs(expected[i] - cd._score('scratch', hi)) <= 1e-12, i
    del cd.ref_vecs['scratch']
    check_order([expected], [order])
    assert order.dtype == np.int64


# ------------------------------------------------------------------------------------------------ the emulator on id rows
@pytest.mark.parametrize('n', [1, 4])
def test_emulator_on_id_rows_equals_the_host_scorer_on_strings(n):
    dc, refs, vocab, rng = small_scorer(n, seed=1)
    V = len(vocab)
    for cands, L in ((1, 1), (2, 5), (5, 26), (8, 64), (32, 12)):
        ids = near_duplicates(vocab, refs, rng, 3, cands, L)
        sc = torch.tensor([[-0.3 * i - 0.1 * b for i in range(cands)] for b in range(3)], dtype=torch.float32)
        for scores, temp in ((None, 1.0), (sc, 1.0)):
            u, e, o = emul_cider_consensus(dc, ids, dc.end_id, scores, temp)
            U, E, O = host_consensus(dc, ids, scores, temp)
            assert np.isfinite(u).all() and np.allclose(u, U, **TOL) and np.allclose(e, E, **TOL)
            check_order(e, o)
        if cands >= 5:
            assert np.array_equal(u[0, 0], u[0, 1]) and np.array_equal(u[0, :, 0], u[0, :, 1])          # identical candidates
            assert (u[0, 2] == 0).all() and (u[0, :, 2] == 0).all()                                     # the empty one
            assert (ids[0, 3] != dc.end_id).all()
            words = ' '.join(host_words(vocab, r, dc.end_id) for r in ids[1].tolist())
            assert words.count('<out-of-range-id>') >= 6 and ((ids[1] < 0) | (ids[1] >= V)).sum() >= 8
            if L > 4:
                assert (U[:, :cands, :cands] > 0).sum() > cands * cands * 3 // 2


def test_the_out_of_vocabulary_word_matches_itself_across_candidates():
    dc, refs, vocab, rng = small_scorer()
    V, end = len(vocab), dc.end_id
    a = vocab.word2idx['w1']
    ids = torch.tensor([[[a, V + 3, -7, end], [a, 1 << 40, V, end], [a, a, a, end]]], dtype=torch.int64)
    u, e, o = emul_cider_consensus(dc, ids, end)
    U, E, O = host_consensus(dc, ids)
    assert np.allclose(u, U, **TOL)
    assert abs(u[0, 0, 1] - u[0, 0, 0]) <= 1e-12 and u[0, 0, 1] > u[0, 0, 2] > 0          # rows 0 and 1 are the same caption


# ------------------------------------------------------------------------------------------------ ordering and validity
def test_ties_invalid_scores_single_candidates_and_posterior_weights():
    dc, refs, vocab, rng = small_scorer()
    end = dc.end_id
    w = [vocab.word2idx['w%d' % i] for i in range(8)]
    # candidates 0, 2 and 3 are one caption, 1 shares nothing: 0, 2, 3 tie, 1 comes last with 0
    ids = torch.tensor([[[w[0], w[1], w[2], end], [w[5], w[6], w[7], end], [w[0], w[1], w[2], end], [w[0], w[1], w[2], end]]])
    u, e, o = emul_cider_consensus(dc, ids, end)
    assert e[0, 0] == e[0, 2] == e[0, 3] > 0 and e[0, 1] == 0 and o[0].tolist() == [0, 2, 3, 1]
    # all different words: every expected utility is 0 and the order is the input's
    ids = torch.tensor([[[w[i], end, 0, 0] for i in range(5)]])
    u, e, o = emul_cider_consensus(dc, ids, end)
    assert (e == 0).all() and o[0].tolist() == [0, 1, 2, 3, 4]
    # invalid scores
    ids = near_duplicates(vocab, refs, rng, 2, 5, 12, special=False)
    sc = torch.tensor([[-1.0, -math.inf, -2.0, math.nan, -0.5], [-math.inf, -math.inf, -3.0, -math.inf, math.nan]])
    for temp in (0.5, 2.0, math.inf):
        u, e, o = emul_cider_consensus(dc, ids, end, sc, temp)
        U, E, O = host_consensus(dc, ids, sc, temp)
        assert np.array_equal(np.isneginf(e), ~(sc > -math.inf).numpy()) and np.array_equal(o, O)
        assert np.allclose(e, E, **TOL)
        check_order(e, o)
        assert set(o[0, 3:].tolist()) == {1, 3} and o[1].tolist() == [2, 0, 1, 3, 4] and e[1, 2] == 0
        # the formula, written out
        if temp != math.inf:
            q = np.exp((np.array([-1.0, -2.0, -0.5]) + 0.5) / temp)
            for i, row in zip((0, 2, 4), range(3)):
                others = [x for x in range(3) if x != row]
                want = sum(q[x] * u[0, i, (0, 2, 4)[x]] for x in others) / sum(q[x] for x in others)
                assert abs(e[0, i] - want) <= 1e-12
        else:
            assert abs(e[0, 0] - (u[0, 0, 2] + u[0, 0, 4]) / 2) <= 1e-12
    # posterior weights change the ranking's input: a sharp posterior follows the best-scored candidate's row of U
    u, e, o = emul_cider_consensus(dc, ids, end, torch.tensor([[0.0, -50.0, -50.0, -50.0, -50.0]] * 2), 0.5)
    assert np.allclose(e[:, 1:], u[:, 1:, 0], rtol=1e-9, atol=1e-12)
    # one candidate
    u, e, o = emul_cider_consensus(dc, ids[:, :1], end)
    assert (o == 0).all() and (e == 0).all() and o.shape == (2, 1)
    assert dc.cider.consensus(['w1 w2'])[1].tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ the public forms
def host_model(batch=4):
    net, orc, frames, regions = synth_pair(11, batch, ops=ConsensusEmul())
    reward = S.CiderD(corpus_for(net.decoder.vocab, 5)).to_device(net.decoder.vocab, device='cpu')
    reward.ops = net.ops
    return net, reward, frames, regions


OPTS = dict(beam_size=6, num_groups=3, diversity_penalty=0.5, length_penalty=0.7)


def logged(ops, fn):
    ops.recording = []
    out = fn()
    log, ops.recording = ops.recording, None
    return out, log


def test_consensus_device_and_rerank_permute_the_beam_search_rows():
    net, reward, frames, regions = host_model()
    ids, scores, lens = net.beam_search(frames, regions, **OPTS)
    order, expected, util = reward.consensus_device(ids, return_utility=True)
    U, E, O = host_consensus(reward, ids)
    assert order.dtype == torch.int64 and expected.dtype == util.dtype == torch.float64
    assert np.allclose(util.numpy(), U, **TOL) and np.allclose(expected.numpy(), E, **TOL)
    check_order(expected.numpy(), order.numpy())
    assert (order != torch.arange(6)).any()                                    # the consensus says something here
    for weights, temp in (('uniform', 1.0), ('posterior', 0.5)):
        for keep in (None, 1, 4):
            got = dlsg_amd.consensus_rerank(reward, ids, scores, lens, weights=weights, temperature=temp, n_best=keep)
            o, e = reward.consensus_device(ids, scores, temp if weights == 'posterior' else math.inf)
            k = 6 if keep is None else keep
            assert torch.equal(got[3], o[:, :k]) and got[0].shape == (4, k, ids.shape[2])
            for b in range(4):
                assert torch.equal(got[0][b], ids[b, o[b, :k]]) and torch.equal(got[2][b], lens[b, o[b, :k]])
                assert torch.equal(got[1][b], e[b, o[b, :k]])
            assert bool((got[1][:, :-1] >= got[1][:, 1:]).all())
    # uniform weights ignore the values of the scores (every beam here is valid)
    a = dlsg_amd.consensus_rerank(reward, ids, scores, lens)
    b = dlsg_amd.consensus_rerank(reward, ids, None, None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[2] is None
    # ... but not their validity
    bad = scores.clone()
    bad[:, 0] = -math.inf
    c = dlsg_amd.consensus_rerank(reward, ids, bad, lens)
    assert (c[3][:, -1] == 0).all() and torch.isneginf(c[1][:, -1]).all()
    # samples viewed as (B, n, L)
    s = net.sample(frames, regions, n=3, seed=5)[0]
    got = dlsg_amd.consensus_rerank(reward, s.view(4, 3, -1))
    assert got[0].shape == (4, 3, s.shape[1]) and sorted(got[3][0].tolist()) == [0, 1, 2]


def test_consensus_search_is_the_beam_search_plus_one_launch():
    net, reward, frames, regions = host_model()
    want, beam_log = logged(net.ops, lambda: net.beam_search(frames, regions, **OPTS))
    got, log = logged(net.ops, lambda: dlsg_amd.consensus_search(net, frames, regions, reward, n_best=6, **OPTS))
    assert log == beam_log + ['cider_consensus']
    ref = dlsg_amd.consensus_rerank(reward, *want)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    one = dlsg_amd.consensus_search(net, frames, regions, reward, **OPTS)
    assert one[0].shape[1] == 1 and torch.equal(one[0][:, 0], got[0][:, 0])
    post = dlsg_amd.consensus_search(net, frames, regions, reward, n_best=6, weights='posterior', temperature=2.0, **OPTS)
    assert torch.equal(post[3], reward.consensus_device(want[0], want[1], 2.0)[0])


def test_consensus_search_with_an_ensemble_and_the_baselines():
    nets, frames, regions = build_members(ops=ConsensusEmul())
    reward = S.CiderD(corpus_for(nets[0].decoder.vocab, 5)).to_device(nets[0].decoder.vocab, device='cpu')
    reward.ops = nets[0].ops
    for search in (dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob'), nets[1], nets[2]):
        want = search.beam_search(frames, regions, **OPTS)
        got = dlsg_amd.consensus_search(search, frames, regions, reward, n_best=3, **OPTS)
        ref = dlsg_amd.consensus_rerank(reward, *want, n_best=3)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))


def test_gather_results_and_evaluate_take_the_consensus_key():
    net, reward, frames, regions = host_model(3)
    loader = [(frames, regions, None, ['v0', 'v1', 'v2'])]
    plain, plain_log = logged(net.ops, lambda: S.gather_results(net, loader, decode=OPTS))
    greedy_log = logged(net.ops, lambda: S.gather_results(net, loader))[1]
    got, log = logged(net.ops, lambda: S.gather_results(net, loader, decode=dict(OPTS, consensus=reward)))
    ids = dlsg_amd.consensus_search(net, frames, regions, reward, **OPTS)[0][:, 0]
    assert got == {'v%d' % i: net.decoder.decode_tokens(ids[i]) for i in range(3)}
    assert [c for c in log if c != 'cider_consensus'] == plain_log and log.count('cider_consensus') == 1
    assert 'cider_consensus' not in plain_log and 'cider_consensus' not in greedy_log
    # without the key the launches are what they were: n_best = 1 of the search, and the greedy pass (then the time-out check)
    tail = ['check_persistent']
    assert plain_log == logged(net.ops, lambda: net.beam_search(frames, regions, n_best=1, **OPTS))[1] + tail
    assert greedy_log == logged(net.ops, lambda: net(frames, regions, None))[1] + tail
    post = S.gather_results(net, loader, decode=dict(OPTS, consensus=reward, consensus_weights='posterior', consensus_temperature=0.5))
    ids = dlsg_amd.consensus_search(net, frames, regions, reward, weights='posterior', temperature=0.5, **OPTS)[0][:, 0]
    assert post == {'v%d' % i: net.decoder.decode_tokens(ids[i]) for i in range(3)}
    refs = {'v%d' % i: [{u'video_id': 'v%d' % i, u'cap_id': 0, u'caption': got['v%d' % i]}] for i in range(3)}
    scores, result = S.evaluate(net, loader, refs, decode=dict(OPTS, consensus=reward))
    assert result == got and scores['Bleu_1'] == pytest.approx(1.0)


def test_value_errors():
    net, reward, frames, regions = host_model(2)
    ids, scores, lens = net.beam_search(frames, regions, **OPTS)
    L = ids.shape[2]
    for bad in (torch.zeros(2, 33, L, dtype=torch.int64), torch.zeros(2, 4, 65, dtype=torch.int64), torch.zeros(8, L, dtype=torch.int64),
                torch.zeros(1, 2, 4, L, dtype=torch.int64)):
        with pytest.raises(ValueError):
            reward.consensus_device(bad)
    for temp in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            reward.consensus_device(ids, scores, temp)
        with pytest.raises(ValueError):
            reward.cider.consensus(['a b', 'a c'], [0.0, -1.0], temp)
        with pytest.raises(ValueError):
            dlsg_amd.consensus_rerank(reward, ids, scores, lens, weights='posterior', temperature=temp)
    with pytest.raises(ValueError):
        dlsg_amd.consensus_rerank(reward, ids, None, lens, weights='posterior')
    with pytest.raises(ValueError):
        dlsg_amd.consensus_search(net, frames, regions, reward, weights='softmax', **OPTS)
    for keep in (0, 7):
        with pytest.raises(ValueError):
            dlsg_amd.consensus_rerank(reward, ids, scores, lens, n_best=keep)
    with pytest.raises(ValueError):
        dlsg_amd.consensus_rerank(reward, ids[0], scores[0], lens[0])
    assert reward.consensus_device(torch.zeros(2, 32, 64, dtype=torch.int64))[0].shape == (2, 32)

"""GPU: consensus reranking on the MI355X -- `dlsg_cider_consensus` against `CiderD.pairwise` / `consensus` on the decoded
strings, its ordering, determinism on relaunch and graph replay, and `consensus_search` / `ConsensusBeamGraph` end to end.  The
CPU side is tests/test_consensus_host.py."""
import functools
import math
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from test_cider_device_host import host_words
from test_consensus_host import check_order, host_consensus, near_duplicates
from test_gpu_cider_device import no_host_sync, scst_corpus, zipf_corpus
from test_gpu_scst import gpu_net

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = dict(rtol=1e-12, atol=1e-12)
B = 3


@functools.lru_cache(maxsize=None)
def scorer():
    """50 clips x 20 references, V = 3000; built once, never modified"""
    vocab = dlsg_amd.make_vocab(3000)
    refs, _ = zipf_corpus(vocab, 50, 20, 21)
    return S.DeviceCiderD(refs, vocab), refs, vocab


def case(n, L):
    """the id rows of a shape and their float32 scores (candidate 1 of clip 2 invalid when there is one)"""
    dc, refs, vocab = scorer()
    rng = random.Random(1000 * n + L)
    ids = near_duplicates(vocab, refs, rng, B, n, L)
    sc = torch.tensor([[-0.4 * rng.random() * (i + 1) for i in range(n)] for _ in range(B)], dtype=torch.float32)
    if n >= 2:
        sc[2, 1] = -math.inf
    return ids, sc


def positive_share(U):
    n = U.shape[1]
    off = ~np.eye(n, dtype=bool)
    return float((U[:, off] > 0).mean()) if n > 1 else 1.0


@pytest.mark.parametrize('L', [1, 26, 64])
@pytest.mark.parametrize('n', [1, 2, 5, 8, 32])
def test_kernel_against_the_host_scorer(n, L):
    dc, refs, vocab = scorer()
    ids, sc = case(n, L)
    wide = torch.full((B, n, L + 9), 7, dtype=torch.int64)
    wide[:, :, 3:3 + L] = ids
    view = wide.to(DEV)[:, :, 3:3 + L]                                # rows of a wider buffer
    assert not view.is_contiguous()
    U = None
    for rows, scores, temp in ((ids.to(DEV), None, 1.0), (view, sc.to(DEV), 0.5), (view, sc.to(DEV), 2.0)):
        order, expected, util = dc.consensus_device(rows, scores, temp, return_utility=True)
        U, E, O = host_consensus(dc, ids, None if scores is None else sc, temp)
        got_u, got_e, got_o = util.cpu().numpy(), expected.cpu().numpy(), order.cpu().numpy()
        assert np.isfinite(got_u).all()
        assert np.allclose(got_u, U, **TOL), np.abs(got_u - U).max()
        assert np.array_equal(np.isneginf(got_e), np.isneginf(E))
        fin = np.isfinite(E)
        assert np.allclose(got_e[fin], E[fin], **TOL), np.abs(got_e[fin] - E[fin]).max()
        check_order(got_e, got_o)                                     # against the device's own expected
        if scores is not None and n >= 2:
            assert got_o[2, -1] == 1 and np.isneginf(got_e[2, 1])
        plain = dc.consensus_device(rows, scores, temp)
        assert torch.equal(plain[0], order) and torch.equal(plain[1], expected)
    assert positive_share(U) > 0.5, positive_share(U)
    if n >= 5:
        assert np.array_equal(got_u[0, 0], got_u[0, 1]) and (got_u[0, 2] == 0).all() and (got_u[0, :, 2] == 0).all()
        assert (ids[0, 3] != dc.end_id).all()
        assert ((ids[1] < 0) | (ids[1] >= len(vocab))).sum() >= 5
        assert '<out-of-range-id>' in ' '.join(host_words(vocab, r, dc.end_id) for r in ids[1].tolist())


def test_empty_batch_and_refusals():
    dc, refs, vocab = scorer()
    order, expected, util = dc.consensus_device(torch.zeros(0, 4, 26, dtype=torch.int64, device=DEV), return_utility=True)
    assert order.shape == (0, 4) and expected.shape == (0, 4) and util.shape == (0, 4, 4)
    for n, L in ((33, 26), (4, 65)):
        ids = torch.zeros(2, n, L, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError):
            dc.consensus_device(ids)
        expected = torch.full((2, n), -7.0, dtype=torch.float64, device=DEV)
        order = torch.full((2, n), -7, dtype=torch.int64, device=DEV)
        with pytest.raises(RuntimeError):                             # the entry point itself refuses and launches nothing
            dc._ops().cider_consensus(ids, dc.end_id, dc, None, 1.0, None, expected, order)
        torch.cuda.synchronize()
        assert (expected == -7.0).all() and (order == -7).all()


def test_relaunch_and_graph_replay_are_bit_identical():
    dc, refs, vocab = scorer()
    ids, sc = case(8, 26)
    ids, sc = ids.to(DEV), sc.to(DEV)
    first = dc.consensus_device(ids, sc, 0.7, return_utility=True)
    again = dc.consensus_device(ids, sc, 0.7, return_utility=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    order, expected, util = (torch.empty_like(x) for x in first)
    ops = dc._ops()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.cider_consensus(ids, dc.end_id, dc, sc, 0.7, util, expected, order)            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.cider_consensus(ids, dc.end_id, dc, sc, 0.7, util, expected, order)
    for _ in range(3):
        for x in (order, expected, util):
            x.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(order, first[0]) and torch.equal(expected, first[1]) and torch.equal(util, first[2])


OPTS = dict(beam_size=6, num_groups=3, diversity_penalty=0.5)


def check_against_host(reward, want, got):
    """got = the rerank of the beam search `want`, against CiderD.consensus on the decoded strings"""
    ids, scores, lens = want
    U, E, O = host_consensus(reward, ids)
    order = got[3].cpu().numpy()
    assert np.allclose(got[1].cpu().numpy(), np.take_along_axis(E, order, 1), **TOL)
    for b in range(ids.shape[0]):
        top = np.sort(E[b])[::-1]
        if top[0] - top[1] > 1e-9:
            assert order[b, 0] == O[b, 0] and torch.equal(got[0][b, 0], ids[b, O[b, 0]])
        assert torch.equal(got[0][b], ids[b][got[3][b]]) and torch.equal(got[2][b], lens[b][got[3][b]])


def test_consensus_search_end_to_end():
    net, sd, args, vocab, frames, regions, _, _ = gpu_net()
    reward = S.CiderD(scst_corpus(vocab)).to_device(vocab)
    want = net.beam_search(frames, regions, **OPTS)
    got = dlsg_amd.consensus_search(net, frames, regions, reward, n_best=6, **OPTS)
    ref = dlsg_amd.consensus_rerank(reward, *want)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    check_against_host(reward, want, got)
    # captured: a replay equals the eager call
    graph = dlsg_amd.ConsensusBeamGraph(net, frames, regions, reward, n_best=6, **OPTS)
    assert graph.valid_for(frames, regions) and not graph.valid_for(frames[:2], regions[:2])
    for _ in range(2):
        out = graph(frames, regions)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, got))
    # no host synchronisation
    with no_host_sync():
        again = dlsg_amd.consensus_search(net, frames, regions, reward, n_best=6, **OPTS)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    net.ops.check_persistent()


def test_consensus_search_with_an_ensemble_of_two():
    net, sd, args, vocab, frames, regions, _, _ = gpu_net()
    other = gpu_net(seed=8)[0]
    ens = dlsg_amd.Ensemble([net, other])
    reward = S.CiderD(scst_corpus(vocab)).to_device(vocab)
    want = ens.beam_search(frames, regions, **OPTS)
    got = dlsg_amd.consensus_search(ens, frames, regions, reward, n_best=6, weights='posterior', temperature=2.0, **OPTS)
    ref = dlsg_amd.consensus_rerank(reward, *want, weights='posterior', temperature=2.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    o, e = reward.consensus_device(want[0], want[1], 2.0)
    assert torch.equal(got[3], o)
    graph = dlsg_amd.ConsensusBeamGraph(ens, frames, regions, reward, n_best=6, weights='posterior', temperature=2.0, **OPTS)
    assert graph.valid_for(frames, regions)
    out = graph(frames, regions)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, got))
    other.train()                                                     # the graph holds every member's mode
    assert not graph.valid_for(frames, regions)

"""GPU (-m gpu): the lexically constrained beam step (dlsg_beam_select_cons) against its emulation (tests/emul_constrained.py) on the
step cases of tests/test_constrained_host.py, its reduction to dlsg_beam_select_hist without constraints, launch behaviour, and
`constrained_beam_search` / `ConstrainedBeamGraph` / `gather_results(decode=dict(constraints=...))` on the HIP kernels against the
restated search of that file.  The tests without the mark run on the CPU: they check the cap on near-ties."""
import functools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from test_beam_nbest_host import close, oracle_stepper, reference_rank, synth_pair
from test_constrained_host import (DIMS, END, GAP, build_cons_case, check_search_properties, check_step_rules, close_lp, count_met,
                                   emulated_step, fresh, reference_constrained_search, run_cons, step_keys)

gpu = pytest.mark.gpu
INTS = ('pred', 'back', 'rows', 'hout', 'met')


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


@gpu
@pytest.mark.parametrize('L', [26, 64])
@pytest.mark.parametrize('dims', DIMS)
def test_beam_select_cons_matches_the_emulation(hip, dims, L):
    """clips with a gap of GAP or more: the integer outputs are equal and new_lp agrees to 1e-5; ended_count where every clip of the
    case qualifies; the other clips keep the step's rules"""
    B, k, V = dims
    for key in step_keys([dims], [L]):
        c, want, gap, _, _ = emulated_step(key)
        got = fresh(c, cuda=True)
        run_cons(hip, got, key)
        got = {o: v.cpu() for o, v in got.items()}
        kept = [b for b in range(B) if gap[b] >= GAP]
        assert 10 * len(kept) >= 9 * B, key
        for b in kept:
            s = slice(b * k, (b + 1) * k)
            for o in INTS:
                assert torch.equal(got[o][s], want[o][s]), (key, b, o)
            close_lp(got['nlp'][s].numpy(), want['nlp'][s].numpy())
        if len(kept) == B:
            assert torch.equal(got['cnt'], want['cnt']), key
        check_step_rules(c, got, key)


@gpu
@pytest.mark.parametrize('L', [26, 64])
@pytest.mark.parametrize('dims', DIMS)
def test_without_constraints_the_launch_is_beam_select_hist_bit_for_bit(hip, dims, L):
    B, k, V = dims
    for key in step_keys([dims], [L]):
        _, _, g, t, m, cw = key
        if cw != (8, 8):
            continue
        c = build_cons_case(dims, L, t, g, cw, 100 * g + t)
        want = fresh(c, cuda=True)
        hip.beam_select_hist(want['lg'][:, 1:V + 1], want['last'], want['lp'], want['pred'], want['nlp'], want['back'], want['rows'], k, END,
                             want['hist'], want['hout'], t, g, m, ended_count=want['cnt'])
        for cons in (None, torch.zeros(B, 0, 1, dtype=torch.int64), torch.full((B, 8, 8), -1, dtype=torch.int64)):
            got = fresh(c, cuda=True)
            got['met'].fill_(7)
            run_cons(hip, got, key, None if cons is None else cons.cuda())
            for o in ('pred', 'back', 'rows', 'hout', 'cnt'):
                assert torch.equal(got[o], want[o]), (key, o)
            assert torch.equal(got['nlp'].view(torch.int32), want['nlp'].view(torch.int32)), key
            assert not bool(got['met'].any())


@gpu
def test_two_launches_give_equal_bits_and_bad_arguments_raise(hip):
    key = ((7, 6, 1000), 26, 2, 2, 0, (8, 8))
    c = emulated_step(key)[0]
    a, b = fresh(c, cuda=True), fresh(c, cuda=True)
    run_cons(hip, a, key)
    run_cons(hip, b, key)
    for o in INTS + ('cnt',):
        assert torch.equal(a[o], b[o]), o
    assert torch.equal(a['nlp'].view(torch.int32), b['nlp'].view(torch.int32))
    B, k, V = key[0]
    bad = fresh(c, cuda=True)
    for cons in (torch.full((B, 9, 1), -1, dtype=torch.int64), torch.full((B, 1, 9), -1, dtype=torch.int64)):
        with pytest.raises(RuntimeError):
            run_cons(hip, bad, key, cons.cuda())
    with pytest.raises(RuntimeError):                                   # what dlsg_beam_select_hist refuses: t outside the history
        hip.beam_select_cons(bad['lg'][:, 1:V + 1], bad['last'], bad['lp'], bad['pred'], bad['nlp'], bad['back'], bad['rows'], k, END,
                             bad['hist'], bad['hout'], 26, bad['cons'])
    with pytest.raises(RuntimeError):                                   # and one buffer for both histories
        hip.beam_select_cons(bad['lg'][:, 1:V + 1], bad['last'], bad['lp'], bad['pred'], bad['nlp'], bad['back'], bad['rows'], k, END,
                             bad['hist'], bad['hist'], 2, bad['cons'])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- model level
NEAR_TIE = 2e-3                                                        # as tests/test_gpu_beam_nbest.py: the two sides' logits differ by up to 1e-3
MODEL_SEED, MODEL_BIAS = 147, 2.0                                     # chosen by the restatement alone (the test below)
OPTS = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=2, min_len=4)


def eight_constraints(batch=8, seed=5):
    """clip b: b % 4 constraints of 1 to 3 alternative word ids of the 50-word vocabulary"""
    rng = np.random.RandomState(seed)
    return [[[int(v) for v in rng.choice(np.arange(4, 50), size=1 + (b + c) % 3, replace=False)] for c in range(b % 4)]
            for b in range(batch)]


@functools.lru_cache(maxsize=None)
def restated_case():
    """g = 2, min_len = 4, alpha = 0.7, up to 3 constraints on eight clips, by the restatement alone: what it returns, and per clip the
    smallest gap its choices and its ranking rest on"""
    net, orc, frames, regions = synth_pair(MODEL_SEED, 8, end_bias=MODEL_BIAS)
    per_clip = eight_constraints()
    step_fn, start, state, end, L = oracle_stepper(orc, frames, regions)
    toks, lps, gap = reference_constrained_search(step_fn, start, state, end, L, 5, 2, 4, per_clip)
    ids, sc, ln, rank_gap = reference_rank(toks, lps, end, 0.7, 5)
    out = [], [], [], []
    for b in range(8):
        met = [count_met(row, per_clip[b], end) for row in ids[b]]
        order = sorted(range(5), key=lambda i: (-met[i], i))
        for dst, src in zip(out, (ids[b], sc[b], ln[b], met)):
            dst.append([src[i] for i in order])
    return (net, frames, regions, per_clip) + out + ([min(a, b) for a, b in zip(gap, rank_gap)],)


def test_restated_case_stays_inside_the_cap():
    """at most one clip in eight has a near-tie in the restatement itself"""
    gap = restated_case()[-1]
    print('smallest gaps', ['%.1e' % x for x in gap])
    assert sum(g >= NEAR_TIE for g in gap) >= 7


@gpu
def test_constrained_search_matches_the_restated_search():
    net, frames, regions, per_clip, want_ids, want_sc, want_len, want_met, gap = restated_case()
    net = net.cuda()
    ids, scores, lens, met = [x.cpu() for x in net.constrained_beam_search(frames.cuda(), regions.cuda(), per_clip, return_met=True, **OPTS)]
    keep = [b for b in range(8) if gap[b] >= NEAR_TIE]
    assert len(keep) >= 7
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b] and met[b].tolist() == want_met[b], b
        close(scores[b].numpy(), want_sc[b], 1e-4)
    check_search_properties(ids, scores, lens, met, per_clip, END, 2, 4)


@gpu
def test_graph_replays_equal_eager_on_two_batches_and_two_constraint_tensors():
    net, orc, frames, regions = synth_pair(36, 8, end_bias=1.0)
    net = net.cuda()
    vocab = net.decoder.vocab
    opts = dict(beam_size=3, length_penalty=0.7, no_repeat_ngram=2, min_len=4, return_met=True)
    f1, r1 = frames.cuda(), regions.cuda()
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    c1 = dlsg_amd.pack_constraints([[[10 + b, 20 + b], 30 + b] for b in range(8)], vocab, 'cuda')
    c2 = dlsg_amd.pack_constraints([[[40 - b, 12], [] if b % 2 else 25] for b in range(8)], vocab, 'cuda', skip_unknown=True)
    assert c1.shape == c2.shape == (8, 2, 2)
    graph = dlsg_amd.ConstrainedBeamGraph(net, f1, r1, c1, **opts)
    for f, r, c in ((f2, r2, c2), (f1, r1, c1), (f1, r1, c2)):
        got = [x.clone() for x in graph(f, r, c)]
        want = net.constrained_beam_search(f, r, c, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(net.constrained_beam_search(f1, r1, c1, **opts)[0], net.constrained_beam_search(f1, r1, c2, **opts)[0])
    with pytest.raises(ValueError):
        graph(f1, r1, torch.full((8, 3, 2), -1, dtype=torch.int64, device='cuda'))
    assert net.decoder.beam_size == 5


@gpu
def test_batch16_beam5_three_constraints_keep_the_properties():
    net, orc, frames, regions = synth_pair(7, 16, end_bias=0.5)
    net = net.cuda()
    rng = np.random.RandomState(3)
    per_clip = [[[int(v) for v in rng.choice(np.arange(4, 50), size=1 + c, replace=False)] for c in range(3)] for _ in range(16)]
    out = net.constrained_beam_search(frames.cuda(), regions.cuda(), per_clip, beam_size=5, no_repeat_ngram=3, min_len=4,
                                      length_penalty=0.7, return_met=True)
    assert out[0].shape == (16, 5, net.decoder.max_words)
    check_search_properties(*out, per_clip, END, 3, 4)
    free = net.beam_search(frames.cuda(), regions.cuda(), beam_size=5, n_best=1)[0][:, 0].cpu()
    assert sum(count_met(free[b].tolist(), per_clip[b], END) == 3 for b in range(16)) < 8        # the constraints are not idle


@gpu
def test_gather_results_returns_captions_with_the_required_words():
    net, _, frames, regions = synth_pair(11, 3)
    net = net.cuda()
    vocab = net.decoder.vocab
    need = {'v0': [vocab.idx2word[20]], 'v1': [[vocab.idx2word[21], vocab.idx2word[22]], vocab.idx2word[23]], 'v2': []}
    loader = [(frames.cuda(), regions.cuda(), None, ['v0', 'v1', 'v2'])]
    got = S.gather_results(net, loader, decode=dict(beam_size=3, constraints=lambda vids: [need[v] for v in vids]))
    assert got['v2'] == S.gather_results(net, loader, decode=dict(beam_size=3))['v2']
    for vid, cons in need.items():
        for con in cons:
            assert set(con if isinstance(con, list) else [con]) & set(got[vid].split()), (vid, got[vid])

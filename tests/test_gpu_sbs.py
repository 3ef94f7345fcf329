"""GPU (-m gpu): the stochastic beam step (dlsg_beam_select_gumbel) against its emulation (tests/emul_sbs.py) on the step cases of
tests/test_sbs_host.py, with one beam against dlsg_sample_embed, launch for launch and captured; and `sample_without_replacement` /
`StochasticBeamGraph` / `consensus_search(stochastic=...)` on the HIP kernels against the restated search of that file."""
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.engine import SITE_SAMPLE, SITE_WORD
from test_beam_nbest_host import close, synth_pair
from test_cider_device_host import corpus_for
from test_sbs_host import (DIMS, END, GAP, INF, OUTPUTS, RESTATED, RESTATED_CLIPS, RESTATED_MODEL, STEP_SEED, TEMPERATURES, build_case,
                           check_against_restated, check_rows, check_sbs_rules, emulated_step, fresh, run_gumbel, step_keys)

gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


@gpu
@pytest.mark.parametrize('L', [26, 64])
@pytest.mark.parametrize('dims', DIMS)
def test_beam_select_gumbel_matches_the_emulation(hip, dims, L):
    """clips whose gap is GAP or more: pred, back, rows, hist_out equal, new_lp to 1e-5, G_out to 1e-5 absolute (float64 arithmetic
    on a float32 log-sum-exp; the largest difference seen is printed), ended_count when every clip qualifies; the other clips:
    the step rules, and the sorted new_lp to 1e-4"""
    B, k, V = dims
    worst = 0.0
    for key in [x for x in step_keys() if x[0] == dims and x[1] == L]:
        c, want, gap, _ = emulated_step(key)
        tg = fresh(c, cuda=True)
        run_gumbel(hip, tg, key)
        got = {o: tg[o].cpu() for o in OUTPUTS}
        keep = gap >= GAP
        assert 10 * int(keep.sum()) >= 9 * B, key
        check_sbs_rules(c, got, key)
        for b in range(B):
            s = slice(b * k, (b + 1) * k)
            if bool(keep[b]):
                for o in ('pred', 'back', 'rows', 'hout'):
                    assert torch.equal(got[o][s], want[o][s]), (key, b, o)
                close(got['nlp'][s].numpy(), want['nlp'][s].numpy(), 1e-5)
                fin = want['gout'][s] > -INF
                assert torch.equal(got['gout'][s][~fin], want['gout'][s][~fin]), (key, b)
                if bool(fin.any()):
                    err = float((got['gout'][s][fin] - want['gout'][s][fin]).abs().max())
                    worst = max(worst, err)
                    assert err <= 1e-5, (key, b, err)
            else:
                close(got['nlp'][s].sort()[0].numpy(), want['nlp'][s].sort()[0].numpy(), 1e-4)
        if bool(keep.all()):
            assert torch.equal(got['cnt'], want['cnt']), key
    print('largest |G_out - emulation| on %s, L = %d: %.3g' % (dims, L, worst))


@gpu
@pytest.mark.parametrize('temperature', TEMPERATURES)
@pytest.mark.parametrize('V', [40, 50, 10007])
def test_one_beam_is_sample_embed_bit_for_bit(hip, V, temperature):
    """k = 1 on the same logits and seed, row0 = (t + 1) * B: pred are the ids dlsg_sample_embed writes, new_lp - last_lp its logp to
    1e-6 (last_lp = 0, so the difference is the child's term itself)"""
    B, W, L = 9, 8, 26
    gen = torch.Generator().manual_seed(V)
    E = torch.randn(V, W, generator=gen).cuda()
    for t, seed in ((0, 5), (3, 2 ** 41 + 17), (L - 1, 99)):
        lg = (torch.randn(B, V + 3, generator=gen) * 3.0).cuda()[:, 1:V + 1]
        ids, out = torch.zeros(B, dtype=torch.int64, device='cuda'), torch.zeros(B, W, device='cuda')
        logp, lens = torch.zeros(B, device='cuda'), torch.full((B,), L, dtype=torch.int64, device='cuda')
        hip.sample_embed(lg, E, ids, out, logp, lens, t, END, temperature=temperature, p=0.0, seed=seed, site=SITE_WORD,
                         site_sample=SITE_SAMPLE, row0=(t + 1) * B)
        c = fresh(build_case((B, 1, V), L, t, 0, 7), cuda=True)
        c['last'].fill_(1)                                              # every row live
        c['lp'].zero_()
        hip.beam_select_gumbel(lg, c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'], 1, END, c['hist'], c['hout'], t,
                               c['gin'], c['gout'], temperature=temperature, seed=seed, site_sample=SITE_SAMPLE)
        assert torch.equal(c['pred'], ids), (t, seed)
        print('V %d, t %d: largest |new_lp - logp| %.3g' % (V, t, float((c['nlp'] - logp).abs().max())))
        close(c['nlp'].cpu().numpy(), logp.cpu().numpy(), 1e-6)
        if t:
            assert torch.equal(c['gout'], c['gin'])                     # one child: it takes the parent's value


@gpu
def test_two_launches_give_equal_bits_and_the_seed_word_is_the_seed(hip):
    key = ((7, 6, 1000), 26, 2, 2, 3, 0.7)
    c = emulated_step(key)[0]
    a, b, d, e = (fresh(c, cuda=True) for _ in range(4))
    run_gumbel(hip, a, key)
    run_gumbel(hip, b, key)
    run_gumbel(hip, d, key, seed=torch.tensor([STEP_SEED], dtype=torch.int64, device='cuda'))
    run_gumbel(hip, e, key, seed=STEP_SEED + 1)
    for o in OUTPUTS:
        assert torch.equal(a[o], b[o]) and torch.equal(a[o], d[o]), o
    assert not torch.equal(a['pred'], e['pred'])


@gpu
def test_step_refuses_what_it_cannot_run(hip):
    key = ((3, 4, 50), 26, 0, 1, 0, 1.0)
    c = fresh(emulated_step(key)[0], cuda=True)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(RuntimeError):
            run_gumbel(hip, c, key[:5] + (bad,))
    with pytest.raises(RuntimeError):
        run_gumbel(hip, dict(c, gout=c['gin']), key)


# ---------------------------------------------------------------------------------------------- model level
@gpu
def test_search_on_the_kernels_matches_the_restated_search_and_the_graph_replays_it():
    net, orc, frames, regions = synth_pair(RESTATED_MODEL, RESTATED_CLIPS, end_bias=1.0)
    net = net.cuda()
    f1, r1 = frames.cuda(), regions.cuda()
    want = net.sample_without_replacement(f1, r1, **RESTATED)
    check_against_restated(*[x.cpu() for x in want])
    opts = {o: v for o, v in RESTATED.items() if o != 'seed'}
    graph = dlsg_amd.StochasticBeamGraph(net, f1, r1, **opts)
    got = [x.clone() for x in graph(f1, r1, RESTATED['seed'])]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    other = [x.clone() for x in graph(f1, r1, RESTATED['seed'] + 1)]
    assert not torch.equal(other[0], want[0])
    eager = net.sample_without_replacement(f1, r1, **dict(RESTATED, seed=RESTATED['seed'] + 1))
    assert all(torch.equal(a, b) for a, b in zip(other, eager))
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    again = graph(f2, r2, RESTATED['seed'])
    assert all(torch.equal(a, b) for a, b in zip(again, net.sample_without_replacement(f2, r2, **RESTATED)))


@gpu
@pytest.mark.parametrize('temperature, seed', [(1.0, 7), (0.7, 123456789)])
def test_one_beam_draws_what_sample_draws(temperature, seed):
    net, orc, frames, regions = synth_pair(11, 6, end_bias=1.0)
    net = net.cuda()
    fc, rc = frames.cuda(), regions.cuda()
    ids, logp, lens = [x.cpu() for x in net.sample_without_replacement(fc, rc, n=1, temperature=temperature, seed=seed)]
    want, want_lp, want_len = [x.cpu() for x in net.sample(fc, rc, n=1, temperature=temperature, seed=seed)]
    end = net.decoder.vocab('<end>')
    for b in range(6):
        n = int(want_len[b])
        assert int(lens[b, 0]) == n and ids[b, 0, :n].tolist() == want[b, :n].tolist() and bool((ids[b, 0, n:] == end).all()), b
        close([float(logp[b, 0])], [float(want_lp[b, :n].double().sum())], 1e-5)


@gpu
def test_threshold_rows_and_consensus_on_the_kernels():
    net, orc, frames, regions = synth_pair(11, 6, end_bias=1.0)
    net = net.cuda()
    fc, rc = frames.cuda(), regions.cuda()
    end = net.decoder.vocab('<end>')
    ids, logp, lens, gumbel, kappa = net.sample_without_replacement(fc, rc, n=5, seed=3, return_threshold=True)
    check_rows(ids.cpu(), lens.cpu(), end)
    assert bool((gumbel[:, :-1] >= gumbel[:, 1:]).all()) and bool((kappa <= gumbel[:, -1]).all())
    six = net.sample_without_replacement(fc, rc, n=6, seed=3)
    assert torch.equal(six[0][:, :5], ids) and torch.equal(six[1][:, :5], logp)
    w = dlsg_amd.importance_weights(logp, kappa)
    assert w.is_cuda and w.dtype == torch.float64 and bool((w >= logp.double().exp()).all())
    reward = S.CiderD(corpus_for(net.decoder.vocab, 6)).to_device(net.decoder.vocab)
    opts = dict(n=5, temperature=0.9, seed=21)
    want = dlsg_amd.consensus_rerank(reward, *net.sample_without_replacement(fc, rc, **opts), n_best=3)
    got = dlsg_amd.consensus_search(net, fc, rc, reward, n_best=3, stochastic=opts)
    assert all(torch.equal(a, b) for a, b in zip(got, want))

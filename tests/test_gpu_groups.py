"""GPU (-m gpu): the diverse beam step (dlsg_beam_select_groups) against dlsg_beam_select_ens -- with one group, and group by group
without a penalty --, against its emulation (tests/emul_groups.py) on the step cases of tests/test_groups_host.py, and the grouped
`beam_search` / `NBestBeamGraph` / `EnsembleBeamGraph` on the HIP kernels against the restated search of that file."""
import pytest
import torch

import dlsg_amd
from test_beam_nbest_host import close, synth_pair
from test_ensemble_host import SETTINGS
from test_gpu_beam_nbest import END, check_properties, fresh
from test_groups_host import (CASES, ENSEMBLES, GAP, INF, OUTPUTS, PENALTIES, SEEDS, base_case, build_seeded, check_against_restated,
                              check_step_rules, emulated_steps, member_logits, run_groups, search_opts, step_keys)

gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def run_ens(ops, c, lgs, weights, mode, key, k=None):
    dims, G, L, g, t, m = key
    V = dims[2]
    ops.beam_select_ens([x[:, 1:V + 1] for x in lgs], weights, mode, c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'],
                        dims[1] if k is None else k, END, c['hist'], c['hout'], t, g, m, ended_count=c['cnt'])


def cases_without_groups():
    """one key per (dims, L, g, t, min_len): the step cases whatever their G"""
    seen, out = set(), []
    for key in step_keys():
        if key[:1] + key[2:] not in seen:
            seen.add(key[:1] + key[2:])
            out.append(key)
    return out


@gpu
@pytest.mark.parametrize('M', list(ENSEMBLES))
@pytest.mark.parametrize('mode', [0, 1])
def test_one_group_is_beam_select_ens_bit_for_bit(hip, mode, M):
    for key in cases_without_groups():
        lgs = [x.cuda() for x in member_logits(key, M)]
        a, b = fresh(base_case(key), cuda=True), fresh(base_case(key), cuda=True)
        run_ens(hip, a, lgs, ENSEMBLES[M], mode, key)
        run_groups(hip, b, lgs, ENSEMBLES[M], mode, key, 0.0, G=1)
        for o in OUTPUTS:
            assert torch.equal(a[o], b[o]), (key, o)


@gpu
@pytest.mark.parametrize('M', list(ENSEMBLES))
@pytest.mark.parametrize('mode', [0, 1])
def test_without_a_penalty_every_group_is_the_smaller_search(hip, mode, M):
    """penalty 0: the outputs of group y are, bit for bit, those of dlsg_beam_select_ens run with k' beams on y's rows alone (rows
    and back after the group offset); at step 0 every group is the k'-beam step 0 of the clip"""
    for key in step_keys():
        dims, G, L, g, t, m = key
        B, k, V = dims
        kg = k // G
        lgs = [x.cuda() for x in member_logits(key, M)]
        whole = fresh(base_case(key), cuda=True)
        run_groups(hip, whole, lgs, ENSEMBLES[M], mode, key, 0.0)
        n_end = 0
        for y in range(G):
            src = y if t else 0                                    # step 0 reads the clip's first row only
            idx = (torch.arange(B).view(B, 1) * k + src * kg + torch.arange(kg).view(1, kg)).reshape(-1).cuda()
            out = (torch.arange(B).view(B, 1) * k + y * kg + torch.arange(kg).view(1, kg)).reshape(-1).cuda()
            part = {o: v[idx].contiguous() if v.shape[0] == B * k else v.clone() for o, v in fresh(base_case(key), cuda=True).items()}
            run_ens(hip, part, [x[idx].contiguous() for x in lgs], ENSEMBLES[M], mode, key, k=kg)
            for o in ('pred', 'nlp', 'hout'):
                assert torch.equal(whole[o][out], part[o]), (key, y, o)
            assert torch.equal(whole['back'][out], part['back'] + y * kg), (key, y)
            clip = (torch.arange(B).view(B, 1) * k).expand(B, kg).reshape(-1).cuda()
            assert torch.equal(whole['rows'][out], clip + y * kg + part['back']), (key, y)
            assert torch.equal(part['rows'], (torch.arange(B).view(B, 1) * kg).expand(B, kg).reshape(-1).cuda() + part['back'])
            n_end += int(part['cnt'])
        assert int(whole['cnt']) == n_end, key


@gpu
@pytest.mark.parametrize('penalty', PENALTIES)
@pytest.mark.parametrize('M', list(ENSEMBLES))
@pytest.mark.parametrize('mode', [0, 1])
def test_beam_select_groups_matches_the_emulation(hip, mode, M, penalty):
    want_all = emulated_steps(mode, M, penalty)
    for key in step_keys():
        dims, G, L, g, t, m = key
        B, k, V = dims
        c = base_case(key)
        tg = fresh(c, cuda=True)
        run_groups(hip, tg, [x.cuda() for x in member_logits(key, M)], ENSEMBLES[M], mode, key, penalty)
        got = {o: tg[o].cpu() for o in OUTPUTS}
        want, gap, _ = want_all[key]
        keep = gap >= GAP
        check_step_rules(c, got, key, exclusive=False)              # parents inside their group, nothing banned chosen: every clip
        for b in range(B):
            s = slice(b * k, (b + 1) * k)
            if bool(keep[b]):
                for o in ('pred', 'back', 'rows', 'hout'):
                    assert torch.equal(got[o][s], want[o][s]), (key, b, o)
                close(got['nlp'][s].numpy(), want['nlp'][s].numpy(), 1e-5)
            else:
                close(got['nlp'][s].sort()[0].numpy(), want['nlp'][s].sort()[0].numpy(), 1e-4)
        if bool(keep.all()):
            assert torch.equal(got['cnt'], want['cnt']), key


@gpu
@pytest.mark.parametrize('mode, M', [(0, 1), (1, 3)])
def test_an_infinite_penalty_excludes(hip, mode, M):
    """no word chosen from a live parent in a group was chosen from a live parent in an earlier group at that step, and every finite
    new_lp belongs to such a pick or to an ended beam's <end>"""
    for key in step_keys():
        c = base_case(key)
        tg = fresh(c, cuda=True)
        run_groups(hip, tg, [x.cuda() for x in member_logits(key, M)], ENSEMBLES[M], mode, key, INF)
        check_step_rules(c, {o: tg[o].cpu() for o in OUTPUTS}, key, exclusive=True)


# ---------------------------------------------------------------------------------------------- model level
@gpu
@pytest.mark.parametrize('name, setting', CASES)
def test_grouped_search_on_the_kernels_matches_the_restated_search(name, setting):
    """the cases of tests/test_groups_host.py on the HIP kernels; and the captured form replays to the eager bits, on the batch it was
    captured on and on another"""
    nets, frames, regions = build_seeded(SEEDS[name, setting])
    ens = dlsg_amd.Ensemble([n.cuda() for n in nets], SETTINGS[setting], setting)
    opts = search_opts(name)
    f1, r1 = frames.cuda(), regions.cuda()
    check_against_restated(name, setting, *[x.cpu() for x in ens.beam_search(f1, r1, **opts)])
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    graph = dlsg_amd.EnsembleBeamGraph(ens, f1, r1, **opts)
    for f, r in ((f2, r2), (f1, r1)):
        got = [x.clone() for x in graph(f, r)]
        want = ens.beam_search(f, r, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(ens.beam_search(f1, r1, **opts)[0], ens.beam_search(f2, r2, **opts)[0])


@gpu
def test_graph_replays_equal_eager_on_two_batches():
    net, orc, frames, regions = synth_pair(36, 8, end_bias=1.0)
    net = net.cuda()
    opts = search_opts('k6g3')
    f1, r1 = frames.cuda(), regions.cuda()
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    graph = dlsg_amd.NBestBeamGraph(net, f1, r1, **opts)
    for f, r in ((f2, r2), (f1, r1)):
        got = [x.clone() for x in graph(f, r)]
        want = net.beam_search(f, r, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(net.beam_search(f1, r1, **opts)[0], net.beam_search(f2, r2, **opts)[0])
    plain = net.beam_search(f1, r1, **dict(opts, num_groups=1, diversity_penalty=0.0))
    assert not torch.equal(plain[0], net.beam_search(f1, r1, **opts)[0])
    assert net.decoder.beam_size == 5


@gpu
def test_batch128_beam6_three_groups_graph_equals_eager_and_keeps_the_properties():
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(1000)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), 3))
    net = net.cuda()
    frames, regions, _, _ = synth_batch(args, 1000, 128, 5)
    fc, rc = frames.cuda(), regions.cuda()
    opts = dict(beam_size=6, num_groups=3, diversity_penalty=0.5, length_penalty=0.7, no_repeat_ngram=3, min_len=4)
    want = net.beam_search(fc, rc, **opts)
    got = dlsg_amd.NBestBeamGraph(net, fc, rc, **opts)(fc, rc)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[0].shape == (128, 6, args.max_words)
    check_properties(got[0].cpu(), vocab('<end>'), 3, 4)

"""GPU (-m gpu): the ensemble beam step (dlsg_beam_select_ens) against dlsg_beam_select_hist with one member and against its
emulation (tests/emul_ensemble.py) with several, and `Ensemble.beam_search` / `EnsembleBeamGraph` on the HIP kernels against the
restated ensemble search of tests/test_ensemble_host.py and the members' own searches.  The first test runs without a GPU: it
checks that the step cases leave at most a tenth of their clips out as near-ties."""
import functools

import pytest
import torch

import dlsg_amd
from emul_beam import banned_classes
from emul_ensemble import EnsembleEmul
from test_beam_nbest_host import close, synth_pair
from test_ensemble_host import OPTS, SETTINGS, build_members, check_against_restated
from test_gpu_beam_nbest import DIMS, END, check_properties, fresh, golden_net, run_step, step_case, steps_of

gpu = pytest.mark.gpu
GAP = 1e-4          # ten times the float32 evaluation error of a combined value of magnitude <= 20 (a few steps of 1.9e-6)
ENSEMBLES = [(1, [1.0]), (2, [0.7, 0.3]), (3, [1.0, 1.0, 1.0]), (8, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])]
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt')


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def step_keys():
    """(dims, L, g, t, min_len) of every step case"""
    return [(dims, L, g, t, m) for dims in DIMS for L in (26, 64) for g in (0, 2, 3) for t in steps_of(L, g) for m in (0, t + 1)]


def member_logits(key, M):
    """member m's logits: those of the step case with seed 100 g + t + 1000 m"""
    dims, L, g, t, _ = key
    return [step_case(dims, L, t, g, 100 * g + t + 1000 * m)['lg'] for m in range(M)]


def base_case(key):
    dims, L, g, t, _ = key
    return step_case(dims, L, t, g, 100 * g + t)


def run_ens(ops, c, lgs, weights, mode, key):
    dims, L, g, t, m = key
    V = dims[2]
    ops.beam_select_ens([x[:, 1:V + 1] for x in lgs], weights, mode, c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'],
                        dims[1], END, c['hist'], c['hout'], t, g, m, ended_count=c['cnt'])


@functools.lru_cache(maxsize=None)
def emulated_steps(mode, M):
    """the emulator on every step case of one (mode, M), computed once and never modified: {key: (outputs, gap (B,))}"""
    emul, out = EnsembleEmul(), {}
    for key in step_keys():
        c = base_case(key)
        run_ens(emul, c, member_logits(key, M), dict(ENSEMBLES)[M], mode, key)
        out[key] = ({o: c[o] for o in OUTPUTS}, emul.gap)
    return out


@pytest.mark.parametrize('M', [m for m, _ in ENSEMBLES])
@pytest.mark.parametrize('mode', [0, 1])
def test_step_cases_leave_few_clips_out(mode, M):
    """on the emulator alone: over all step cases of a (mode, M), at most 10 % of the clips have a gap below 1e-4"""
    gaps = torch.cat([gap for _, gap in emulated_steps(mode, M).values()])
    out = int((gaps < GAP).sum())
    print('mode %d M %d: %d of %d clips below %g' % (mode, M, out, gaps.numel(), GAP))
    assert gaps.numel() >= 384 and 10 * out <= gaps.numel()


@gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_one_member_is_beam_select_hist_bit_for_bit(hip, mode):
    for key in step_keys():
        dims, L, g, t, m = key
        a, b = fresh(base_case(key), cuda=True), fresh(base_case(key), cuda=True)
        run_step(hip, a, dims, t, g, m)
        run_ens(hip, b, [b['lg']], [1.0], mode, key)
        for o in OUTPUTS:
            assert torch.equal(a[o], b[o]), (key, o)


def chosen_are_not_banned(c, got, key, b):
    dims, L, g, t, m = key
    k = dims[1]
    for j in range(k):
        parent = int(got['rows'][b * k + j])
        assert b * k <= parent < (b + 1) * k
        if t == 0 or int(c['last'][parent]) != END:
            assert int(got['pred'][b * k + j]) not in banned_classes(c['hist'][parent, :t].tolist(), t, g, m, END), (key, b, j)


@gpu
@pytest.mark.parametrize('M, weights', ENSEMBLES)
@pytest.mark.parametrize('mode', [0, 1])
def test_beam_select_ens_matches_the_emulation(hip, mode, M, weights):
    want_all = emulated_steps(mode, M)
    for key in step_keys():
        dims, L, g, t, m = key
        B, k, V = dims
        c = base_case(key)
        tg = fresh(c, cuda=True)
        run_ens(hip, tg, [x.cuda() for x in member_logits(key, M)], weights, mode, key)
        got = {o: tg[o].cpu() for o in OUTPUTS}
        want, gap = want_all[key]
        keep = gap >= GAP
        for b in range(B):
            s = slice(b * k, (b + 1) * k)
            if bool(keep[b]):
                for o in ('pred', 'back', 'rows', 'hout'):
                    assert torch.equal(got[o][s], want[o][s]), (key, b, o)
                close(got['nlp'][s].numpy(), want['nlp'][s].numpy(), 1e-5)
            else:
                close(got['nlp'][s].sort()[0].numpy(), want['nlp'][s].sort()[0].numpy(), 1e-4)
                chosen_are_not_banned(c, got, key, b)
        if bool(keep.all()):
            assert torch.equal(got['cnt'], want['cnt']), key


@gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_the_same_member_three_times_is_that_member(hip, mode):
    """weights 0.5 : 0.3 : 0.2 on one logits tensor: both modes give back the member's log-probs (to 1e-5), and its choices where
    the emulator saw no near-tie"""
    emul, weights = EnsembleEmul(), [0.5, 0.3, 0.2]
    for key in [key for key in step_keys() if key[1] == 26 and key[2] == 2]:
        dims, L, g, t, m = key
        B, k, V = dims
        c = base_case(key)
        one, three, ec = fresh(c, cuda=True), fresh(c, cuda=True), fresh(c)
        run_ens(hip, one, [one['lg']], [1.0], mode, key)
        run_ens(hip, three, [three['lg']] * 3, weights, mode, key)
        run_ens(emul, ec, [ec['lg']] * 3, weights, mode, key)
        close(three['nlp'].cpu().numpy(), one['nlp'].cpu().numpy(), 1e-5)
        for b in range(B):
            if float(emul.gap[b]) >= GAP:
                assert torch.equal(three['pred'][b * k:(b + 1) * k], one['pred'][b * k:(b + 1) * k]), (key, b)


# ---------------------------------------------------------------------------------------------- model level
@gpu
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_ensemble_on_the_kernels_matches_the_restated_search(setting):
    """the three-member case of tests/test_ensemble_host.py on the HIP kernels; and its captured form replays to the eager bits,
    on the batch it was captured on and on another"""
    nets, frames, regions = build_members()
    ens = dlsg_amd.Ensemble([n.cuda() for n in nets], SETTINGS[setting], setting)
    f1, r1 = frames.cuda(), regions.cuda()
    check_against_restated(setting, *[x.cpu() for x in ens.beam_search(f1, r1, **OPTS)])
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    graph = dlsg_amd.EnsembleBeamGraph(ens, f1, r1, **OPTS)
    for f, r in ((f2, r2), (f1, r1)):
        got = [x.clone() for x in graph(f, r)]
        want = ens.beam_search(f, r, **OPTS)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(ens.beam_search(f1, r1, **OPTS)[0], ens.beam_search(f2, r2, **OPTS)[0])
    assert [n.decoder.beam_size for n in nets] == [5, 5, 5]


@gpu
@pytest.mark.parametrize('opts', [dict(), dict(length_penalty=0.7, no_repeat_ngram=2, min_len=4)])
@pytest.mark.parametrize('tag', ['small_msvd', 'small_baselinemodel', 'end_bias'])
def test_one_member_is_the_models_own_search(tag, opts):
    if tag == 'end_bias':
        net, orc, frames, regions = synth_pair(13, 4, end_bias=2.0)
        net = net.cuda()
    else:
        net, orc, frames, regions = golden_net(tag)
    fc, rc = frames.cuda(), regions.cuda()
    want = net.beam_search(fc, rc, **opts)
    for mode in ('prob', 'logprob'):
        got = dlsg_amd.Ensemble([net], mode=mode).beam_search(fc, rc, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), mode


@gpu
def test_batch128_beam5_two_members_graph_equals_eager():
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(1000)
    nets = []
    for seed in (3, 4):
        torch.manual_seed(0)
        net = dlsg_amd.CapGnnModel(args, vocab).eval()
        net.load_state_dict(synth_state_dict(net.state_dict(), seed))
        nets.append(net.cuda())
    ens = dlsg_amd.Ensemble(nets)
    frames, regions, _, _ = synth_batch(args, 1000, 128, 5)
    fc, rc = frames.cuda(), regions.cuda()
    opts = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=3, min_len=4)
    want = ens.beam_search(fc, rc, **opts)
    graph = dlsg_amd.EnsembleBeamGraph(ens, fc, rc, **opts)
    got = graph(fc, rc)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[0].shape == (128, 5, args.max_words)
    check_properties(got[0].cpu(), vocab('<end>'), 3, 4)
    # the second member moves to a new arena (what load_state_dict into a copy leads to): the graph refuses to replay
    assert graph.valid_for(fc, rc)
    old = nets[1]._flat
    nets[1]._flat = None
    nets[1].flatten_parameters_()
    assert nets[1]._flat is not old and not graph.valid_for(fc, rc)
    with pytest.raises(RuntimeError, match='arena'):
        graph(fc, rc)

"""GPU (-m gpu): the beam step with exclusions (dlsg_beam_select_excl) against its emulation (tests/emul_excl.py) on the step cases of
tests/test_excl_host.py, its exact reductions to dlsg_beam_select_ens and dlsg_beam_select_hist, and `beam_search(exclude=...)` of a
model, an `Ensemble`, `NBestBeamGraph` and `gather_results` on the HIP kernels against the restated search of that file."""
import functools

import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.beam import Exclusions, exclusions_hit, pack_exclusions
from test_beam_nbest_host import close, synth_pair
from test_constrained_host import GAP, close_lp
from test_excl_host import (GPU_CASE, OUTPUTS, WEIGHTS, check_excluded, restated_search, run_excl, step_case, step_keys)
from test_gpu_beam_nbest import NEAR_TIE
from test_sbs_host import END, fresh

gpu = pytest.mark.gpu
SEARCH = (5, 2, 4, 0.7)                                               # beam 5, no repeated bigram, four words at least, alpha 0.7
OPTS = dict(beam_size=5, no_repeat_ngram=2, min_len=4, length_penalty=0.7)


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def on_device(x):
    return None if x is None else x.cuda()


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same_bits(a, b, what):
    for o in OUTPUTS:
        assert torch.equal(bits(a[o]), bits(b[o])), (what, o)


def run_ens(ops, c, lgs, key, min_len=None):
    dims, L, g, t, m, tab, M, mode = key
    V = dims[2]
    ops.beam_select_ens([x[:, 1:V + 1] for x in lgs], WEIGHTS[M], mode, c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'],
                        dims[1], END, c['hist'], c['hout'], t, g, m if min_len is None else min_len, ended_count=c['cnt'])


# ---------------------------------------------------------------------------------------------- the step
@gpu
def test_beam_select_excl_matches_the_emulation(hip):
    """pred, back, rows, hist_out equal and new_lp to 1e-5 on the clips whose deciding gap in the restatement is GAP or more
    (tests/test_excl_host.py keeps nine tenths of every case's clips); ended_count where every clip of the case qualifies"""
    compared = 0
    for key in step_keys():
        c, lgs, shared, per_clip, want, _, restated, _ = step_case(key)
        B, k, V = key[0]
        tg = fresh(c, cuda=True)
        run_excl(hip, tg, [x.cuda() for x in lgs], on_device(shared), on_device(per_clip), key)
        got = {o: tg[o].cpu() for o in OUTPUTS}
        keep = [x >= GAP for x in restated['gap']]
        for b in range(B):
            if keep[b]:
                s = slice(b * k, (b + 1) * k)
                for o in ('pred', 'back', 'rows', 'hout'):
                    assert torch.equal(got[o][s], want[o][s]), (key, b, o)
                close_lp(got['nlp'][s].numpy(), want['nlp'][s].numpy())
                compared += 1
        if all(keep):
            assert torch.equal(got['cnt'], want['cnt']), key
    assert compared > 1500


@gpu
def test_empty_tables_are_beam_select_ens_bit_for_bit(hip):
    for key in [key for key in step_keys() if key[5] == 'mixed']:
        c, lgs, shared, per_clip = step_case(key)[:4]
        B = key[0][0]
        lg = [x.cuda() for x in lgs]
        a = fresh(c, cuda=True)
        run_ens(hip, a, lg, key)
        for sh, pc in ((None, None), (shared[:0].cuda(), per_clip[:, :0].cuda()), (torch.full_like(shared, -1).cuda(), None),
                       (None, torch.full_like(per_clip, key[0][2]).cuda())):
            b = fresh(c, cuda=True)
            run_excl(hip, b, lg, sh, pc, key)
            same_bits(a, b, key)


@gpu
def test_one_member_with_empty_tables_is_beam_select_hist_bit_for_bit(hip):
    seen = 0
    for key in [key for key in step_keys() if key[6] == 1 and key[5] in ('empty', 'mixed')]:
        dims, L, g, t, m, tab, M, mode = key
        c, lgs = step_case(key)[:2]
        V = dims[2]
        a, b = fresh(c, cuda=True), fresh(c, cuda=True)
        lg = lgs[0].cuda()
        hip.beam_select_hist(lg[:, 1:V + 1], a['last'], a['lp'], a['pred'], a['nlp'], a['back'], a['rows'], dims[1], END, a['hist'],
                             a['hout'], t, g, m, ended_count=a['cnt'])
        for md in (0, 1):
            b = fresh(c, cuda=True)
            run_excl(hip, b, [lg], None, None, key[:7] + (md,))
            same_bits(a, b, key)
        seen += 1
    assert seen >= 40


@gpu
def test_excluding_end_is_a_minimum_length_bit_for_bit(hip):
    """the one-word shared entry (<end>,) with min_len = 0 against beam_select_ens with min_len = t + 1, at t in {0, 2}"""
    seen = 0
    for key in [key for key in step_keys() if key[3] in (0, 2) and key[4] == 0 and key[5] == 'one']:
        dims, L, g, t, m, tab, M, mode = key
        c, lgs = step_case(key)[:2]
        lg = [x.cuda() for x in lgs]
        a, b = fresh(c, cuda=True), fresh(c, cuda=True)
        run_ens(hip, a, lg, key, min_len=t + 1)
        run_excl(hip, b, lg, torch.tensor([[END]]).cuda(), None, key)
        same_bits(a, b, key)
        seen += 1
    assert seen >= 12


@gpu
def test_two_launches_give_equal_bits(hip):
    for key in [key for key in step_keys() if key[5] in ('mixed', 'full') and key[1] == 64]:
        c, lgs, shared, per_clip = step_case(key)[:4]
        lg, sh, pc = [x.cuda() for x in lgs], shared.cuda(), per_clip.cuda()
        a, b = fresh(c, cuda=True), fresh(c, cuda=True)
        run_excl(hip, a, lg, sh, pc, key)
        run_excl(hip, b, lg, sh, pc, key)
        same_bits(a, b, key)


@gpu
def test_bad_arguments_raise(hip):
    key = [key for key in step_keys() if key[0] == (3, 3, 70) and key[3] == 2 and key[5] == 'mixed'][0]
    c, lgs, shared, per_clip = step_case(key)[:4]
    lg, sh, pc = [x.cuda() for x in lgs], shared.cuda(), per_clip.cuda()
    tg = fresh(c, cuda=True)
    run_excl(hip, tg, lg, sh, pc, key)
    for bad_sh, bad_pc in ((sh.int(), pc), (sh, pc[:2]), (sh.cpu(), pc), (sh[:, :2], pc), (sh.t(), pc), (sh, pc.cpu()), (sh[0], pc),
                           (torch.zeros(65, 4, dtype=torch.int64).cuda(), pc), (sh, torch.zeros(3, 33, 4, dtype=torch.int64).cuda()),
                           (torch.zeros(2, 5, dtype=torch.int64).cuda(), None)):
        with pytest.raises(AssertionError):
            run_excl(hip, fresh(c, cuda=True), lg, bad_sh, bad_pc, key)
    # the library's own refusals, behind the binding's checks: counts and P outside their limits, a count with a NULL table
    import ctypes as C
    from dlsg_amd.hip import _p
    dims, L, g, t, m, tab, M, mode = key
    V = dims[2]
    R_, V_, members = hip._beam_members([x[:, 1:V + 1] for x in lg], WEIGHTS[M], tg['hout'].device)
    a, hist = hip._hist_step(R_, V_, tg['last'], tg['lp'], tg['pred'], tg['nlp'], tg['back'], tg['rows'], dims[1], END, tg['hist'], tg['hout'],
                             t, g, m, tg['cnt'])
    call = lambda *tables: hip.lib.dlsg_beam_select_excl(C.byref(a), *members, mode, *hist, *tables, hip._stream())      # noqa: E731
    assert call(_p(sh), sh.shape[0], _p(pc), pc.shape[1], 4) == 0
    for tables in ((_p(sh), 65, _p(pc), 1, 4), (_p(sh), -1, _p(pc), 1, 4), (_p(sh), 1, _p(pc), 33, 4), (_p(sh), 1, _p(pc), -1, 4),
                   (None, 1, _p(pc), 1, 4), (_p(sh), 1, None, 1, 4), (_p(sh), 1, _p(pc), 1, 0), (_p(sh), 1, _p(pc), 1, 5),
                   (None, 0, _p(pc), 1, 9)):
        assert call(*tables) != 0, tables[1::2]
    assert call(None, 0, None, 0, 0) == 0                                        # (no table: P is not looked at)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- model level
@functools.lru_cache(maxsize=None)
def restated_case():
    """the 8-clip case by the restatement alone: exclusions from the clips' own unrestricted captions, the search under them, and
    per clip the smallest gap it saw"""
    ex, ids, sc, ln, gap = restated_search(*SEARCH, **GPU_CASE)[:5]
    return ex, ids, sc, ln, gap


def test_restated_case_stays_inside_the_cap():
    ex, _, _, want_len, gap = restated_case()
    print('smallest gaps', ['%.1e' % x for x in gap])
    assert len([b for b in range(8) if gap[b] >= NEAR_TIE]) >= 7
    assert ex.shared.shape[0] >= 4 and ex.per_clip.shape == (8, 1, 2)


def gpu_net():
    net, _, frames, regions = synth_pair(GPU_CASE['seed'], GPU_CASE['batch'], end_bias=GPU_CASE['bias'])
    return net.cuda(), frames.cuda(), regions.cuda()


@gpu
def test_beam_search_with_exclusions_matches_the_restated_search():
    """ids in ranking order, lens, and scores to 1e-4, on the clips without a near-tie below 2e-3 in the restatement (the rule of
    tests/test_gpu_beam_nbest.py); no caption of finite score holds an excluded entry or a listed ending"""
    ex, want_ids, want_sc, want_len, gap = restated_case()
    endings = restated_search(*SEARCH, **GPU_CASE)[7]
    net, fc, rc = gpu_net()
    dev = Exclusions(ex.shared.cuda(), ex.per_clip.cuda())
    ids, scores, lens = [x.cpu() for x in net.beam_search(fc, rc, exclude=dev, **OPTS)]
    keep = [b for b in range(8) if gap[b] >= NEAR_TIE]
    assert len(keep) >= 7
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b], b
        close(scores[b].numpy(), want_sc[b], 1e-4)
    check_excluded(ids, scores, lens, ex, endings, END)
    free = net.beam_search(fc, rc, **OPTS)
    assert 2 * int((exclusions_hit(free[0], free[2], dev)[:, 0] > 0).sum()) > 8
    empty = net.beam_search(fc, rc, exclude=Exclusions(None, None), **OPTS)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(empty, free))


@gpu
def test_an_ensemble_of_two_members_with_exclusions():
    """the model twice, weights 0.6 : 0.4, in both modes: the model's own captions under the same exclusions; and two different
    members: nothing excluded in any caption, and the captions differ from the search without"""
    ex = restated_case()[0]
    endings = restated_search(*SEARCH, **GPU_CASE)[7]
    net, fc, rc = gpu_net()
    dev = Exclusions(ex.shared.cuda(), ex.per_clip.cuda())
    want = net.beam_search(fc, rc, exclude=dev, **OPTS)
    gap = restated_case()[4]
    keep = [b for b in range(8) if gap[b] >= NEAR_TIE]
    for mode in ('prob', 'logprob'):
        got = dlsg_amd.Ensemble([net, net], weights=[0.6, 0.4], mode=mode).beam_search(fc, rc, exclude=dev, **OPTS)
        assert torch.equal(got[0][keep], want[0][keep]) and torch.equal(got[2][keep], want[2][keep])
        close(got[1][keep].cpu().numpy(), want[1][keep].cpu().numpy(), 1e-4)
    other = synth_pair(GPU_CASE['seed'] + 1, GPU_CASE['batch'], end_bias=GPU_CASE['bias'])[0].cuda()
    ens = dlsg_amd.Ensemble([net, other], weights=[0.5, 0.5])
    ids, scores, lens = [x.cpu() for x in ens.beam_search(fc, rc, exclude=dev, **OPTS)]
    check_excluded(ids, scores, lens, ex, endings, END)
    assert not torch.equal(ids, ens.beam_search(fc, rc, **OPTS)[0].cpu())
    graph = dlsg_amd.EnsembleBeamGraph(ens, fc, rc, exclude=dev, **OPTS)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(graph(fc, rc), ens.beam_search(fc, rc, exclude=dev, **OPTS)))


@gpu
def test_graph_replay_equals_eager_and_follows_its_tables():
    """NBestBeamGraph(..., exclude=ex): a replay gives the eager call's bits, on the batch it was captured on and on another, and
    again after new per-clip entries were copied into `graph.exclude.per_clip` in place"""
    ex = restated_case()[0]
    net, f1, r1 = gpu_net()
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    dev = Exclusions(ex.shared.cuda(), ex.per_clip.cuda())
    graph = dlsg_amd.NBestBeamGraph(net, f1, r1, exclude=dev, **OPTS)
    assert graph.exclude.per_clip.data_ptr() != dev.per_clip.data_ptr() and graph.options == OPTS
    for f, r in ((f2, r2), (f1, r1)):
        got = [x.clone() for x in graph(f, r)]
        want = net.beam_search(f, r, exclude=dev, **OPTS)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
    before = [x.clone() for x in graph(f1, r1)]
    # new per-clip entries: the first two words of the best caption the graph has just returned
    new = before[0][:, 0, :2].reshape(8, 1, 2).contiguous()
    graph.exclude.per_clip.copy_(new)
    got = [x.clone() for x in graph(f1, r1)]
    want = net.beam_search(f1, r1, exclude=Exclusions(dev.shared, new), **OPTS)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
    assert not torch.equal(got[0], before[0])
    assert not bool(exclusions_hit(got[0], got[2], Exclusions(None, new))[got[1] > -float('inf')].any())
    plain = dlsg_amd.NBestBeamGraph(net, f1, r1, **OPTS)
    assert plain.exclude is None
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plain(f1, r1), net.beam_search(f1, r1, **OPTS)))


@gpu
def test_gather_results_with_exclusions():
    ex = restated_case()[0]
    net, fc, rc = gpu_net()
    vocab = net.decoder.vocab
    vids = ['v%d' % i for i in range(8)]
    loader = [(fc[:4], rc[:4], None, vids[:4]), (fc[4:], rc[4:], None, vids[4:])]
    own = {v: ex.per_clip[i:i + 1] for i, v in enumerate(vids)}
    fn = lambda batch: Exclusions(ex.shared, torch.cat([own[v] for v in batch]))                      # noqa: E731
    got = S.gather_results(net, loader, decode=dict(exclude=fn, **OPTS))
    want = {}
    for frames, regions, _, batch in loader:                               # the same batches, searched directly
        dev = Exclusions(ex.shared.cuda(), torch.cat([own[v] for v in batch]).cuda())
        ids = net.beam_search(frames, regions, exclude=dev, n_best=1, **OPTS)[0][:, 0].cpu()
        want.update({v: net.decoder.decode_tokens(ids[i]) for i, v in enumerate(batch)})
    assert got == want and list(got) == vids
    words = {vocab.idx2word[int(w)] for w in ex.shared[ex.shared[:, 1] < 0, 0]}
    assert words and all(not words & set(sent.split()) for sent in got.values())
    assert got != S.gather_results(net, loader, decode=dict(OPTS))

"""GPU (-m gpu): dlsg_seq_logprob against its float64 restatement (tests/emul_seqscore.py), bit for bit against the beam steps whose
log-probs it reproduces, and `score` / `rescore_search` / `ScoreGraph` / `RescoreBeamGraph` / `perplexity` on the HIP kernels:
a model that rescores its own search gets that search's scores back.  Cases, bounds and helpers are those of
tests/test_rescore_host.py.  The first test runs without a GPU: it checks how many rank positions the cases leave out."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from emul_seqscore import seq_logprob_f64
from test_ensemble_host import SETTINGS, build_members, member_specs
from test_rescore_host import (ALPHA, END, K, KERNEL_CASES, OPTS, WEIGHTS, caption_loader, check_perplexity, check_round_trip,
                               kernel_case)

gpu = pytest.mark.gpu
INF, NAN = float('inf'), float('nan')
GAP = 1e-4                                        # a combined value's float32 evaluation error is a few 1e-6 at magnitude <= 40


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


@functools.lru_cache(maxsize=None)
def emulated(case, mode):
    """the float64 restatement of a kernel case (computed once, never modified)"""
    views, ids = kernel_case(*case)
    return seq_logprob_f64(views, WEIGHTS[case[3]], mode, ids, None, ALPHA, END)


def on_device(case):
    """the case's views rebuilt over device copies of their buffers: same layout, same strides"""
    V, L, R, M, layout, pad = case
    views, ids = kernel_case(*case)
    out = []
    for x in views:
        buf = (x if layout == 'tm' else x.transpose(0, 1))
        whole = torch.empty(buf.shape[0], buf.shape[1], V + pad).copy_(torch.as_strided(buf, (buf.shape[0], buf.shape[1], V + pad), buf.stride()))
        dev = whole.cuda()[:, :, :V]
        out.append(dev if layout == 'tm' else dev.transpose(0, 1))
        assert out[-1].stride() == x.stride()
    return out, ids.cuda()


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('case', KERNEL_CASES)
def test_cases_leave_few_rank_positions_out(case, mode):
    """on the restatement alone: at most 10 % of a case's positions have another class within 1e-4 of the target's value"""
    out = emulated(case, mode)
    live = out['tok_rank'] >= 0
    near = int((out['margin'][live] < GAP).sum())
    print('V %d L %d R %d M %d mode %d: %d of %d positions within %g' % (case[:4] + (mode, near, int(live.sum()), GAP)))
    assert 10 * near <= int(live.sum())


@gpu
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('case', KERNEL_CASES)
def test_kernel_matches_the_restatement(hip, case, mode):
    V, L, R, M = case[:4]
    views, ids = on_device(case)
    want = emulated(case, mode)
    scores, lens, lp, tok, rank = hip.seq_logprob(views, WEIGHTS[M], mode, ids, None, ALPHA, True, True, end=END)
    again = hip.seq_logprob(views, WEIGHTS[M], mode, ids, None, ALPHA, True, True, end=END)
    for a, b in zip((scores, lens, lp, tok, rank), again):                  # two launches: equal bits
        assert torch.equal(a, b)
    plain = hip.seq_logprob(views, WEIGHTS[M], mode, ids, None, ALPHA, end=END)
    assert plain[3] is None and plain[4] is None and all(torch.equal(a, b) for a, b in zip(plain[:3], (scores, lens, lp)))
    assert torch.equal(lens.cpu(), want['lens'])
    ln = want['lens'].double()
    err = (tok.cpu().double() - want['tok_lp']).abs()
    print('max |tok_lp - restated| %.3g, max |lp - restated| / len %.3g' % (float(err.max()), float(((lp.cpu().double() - want['lp']).abs() / ln).max())))
    assert float(err.max()) <= 1e-5
    assert bool(((lp.cpu().double() - want['lp']).abs() <= 1e-5 * ln).all())
    assert bool(((scores.cpu().double() - lp.cpu().double() / ln ** ALPHA).abs() <= 1e-6 * (1 + want['scores'].abs())).all())
    rank = rank.cpu().long()
    if M == 1:
        assert torch.equal(rank, want['tok_rank'])
    else:
        keep = want['margin'] >= GAP
        live = want['tok_rank'] >= 0
        assert 10 * int((live & ~keep).sum()) <= int(live.sum())
        assert torch.equal(rank[keep], want['tok_rank'][keep])
        assert bool((rank[live] >= 0).all())
    # given lens, clamped: the first row counts nothing, the last more than there is
    given = torch.arange(R, dtype=torch.int64) * 7 - int(R > 1)
    got = hip.seq_logprob(views, WEIGHTS[M], mode, ids, given.cuda(), 0.0, True, end=END)
    host_views, host_ids = kernel_case(*case)
    ref = seq_logprob_f64(host_views, WEIGHTS[M], mode, host_ids, given, 0.0, END)
    assert torch.equal(got[1].cpu(), ref['lens']) and float((got[3].cpu().double() - ref['tok_lp']).abs().max()) <= 1e-5
    assert float(got[0][0]) == 0.0 and float(got[2][0]) == 0.0


@gpu
@pytest.mark.parametrize('V', [50, 65, 1000, 4099])
def test_word_log_probs_are_the_search_steps_bits(hip, V):
    """targets = the row's best class: tok_lp is the new_lp of beam_select_hist (one member) and of beam_select_ens (three, both
    modes) on the same rows with k = 1 at step 0, with torch.equal"""
    R, L = 17, 5
    g = torch.Generator().manual_seed(V)
    xs = [(torch.randn(L, R, V + 3, generator=g) * 4.0).cuda()[:, :, :V] for _ in range(3)]

    def step(t, run):
        o = dict(pred=torch.empty(R, dtype=torch.int64, device='cuda'), nlp=torch.empty(R, dtype=torch.float32, device='cuda'),
                 back=torch.empty(R, dtype=torch.int64, device='cuda'), rows=torch.empty(R, dtype=torch.int64, device='cuda'))
        last, lp0 = torch.zeros(R, dtype=torch.int64, device='cuda'), torch.zeros(R, dtype=torch.float32, device='cuda')
        hist = torch.empty(2, R, L, dtype=torch.int64, device='cuda')
        run(last, lp0, o['pred'], o['nlp'], o['back'], o['rows'], 1, V + 7, hist[0], hist[1], 0)
        return o['pred'], o['nlp']
    for M, mode in ((1, 0), (3, 0), (3, 1)):
        weights = WEIGHTS[M]
        preds, nlps = [], []
        for t in range(L):
            if M == 1:
                p, v = step(t, lambda *a: hip.beam_select_hist(xs[0][t], *a))
            else:
                p, v = step(t, lambda *a: hip.beam_select_ens([x[t] for x in xs], weights, mode, *a))
            preds.append(p); nlps.append(v)
        ids = torch.stack(preds, 1).contiguous()
        got = hip.seq_logprob(xs[:M], weights, mode, ids, None, 0.0, True, True, end=V + 7)
        assert torch.equal(got[3], torch.stack(nlps, 1)), (M, mode)
        assert torch.equal(got[1], torch.full((R,), L, device='cuda')) and bool((got[4] == 0).all())


@gpu
def test_einval_cases(hip):
    x = torch.randn(4, 2, 10, device='cuda')
    ids = torch.zeros(2, 4, dtype=torch.int64, device='cuda')
    lp = torch.zeros(2, device='cuda')

    def call(M=1, mode=0, L=4, V=10, alpha=0.0, R=2):
        n = max(M, 1)
        return hip.lib.dlsg_seq_logprob((C.c_void_p * n)(*[x.data_ptr()] * n), (C.c_int64 * n)(*[20] * n), (C.c_int64 * n)(*[10] * n),
                                        (C.c_float * n)(*[1.0 / n] * n), (C.c_float * n)(*[math.log(1.0 / n)] * n), M, mode,
                                        C.c_void_p(ids.data_ptr()), 4, None, R, L, V, C.c_int64(3), C.c_double(alpha), None, None,
                                        C.c_void_p(lp.data_ptr()), None, None, hip._stream())
    from dlsg_amd.hip import ENS_MAX
    EINVAL = dlsg_amd.abi.defines['DLSG_EINVAL']
    for bad in (dict(M=0), dict(M=ENS_MAX + 1), dict(mode=2), dict(mode=-1), dict(L=0), dict(L=65), dict(V=0), dict(alpha=-0.5),
                dict(alpha=NAN)):
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((lp == 0).all())                                         # nothing was launched
    assert call(R=0) == 0 and call() == 0 and call(M=2, mode=1) == 0
    torch.cuda.synchronize()
    assert bool((lp != 0).all())
    with pytest.raises(ValueError):
        hip.seq_logprob([x], [0.0], 0, ids)


@gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_special_rows(hip, mode):
    """designated rows only: a target outside the vocabulary, a -inf target, a member row of -inf, a NaN -- against the restatement,
    which tests/test_rescore_host.py pins to the stated values"""
    V, L, R = 70, 3, 6
    g = torch.Generator().manual_seed(31)
    xs = [torch.randn(L, R, V, generator=g) * 4.0 for _ in range(3)]
    ids = torch.randint(4, V, (R, L), generator=g)
    ids[0, 1] = V                                                 # row 0: target above the vocabulary
    ids[1, 0] = -5                                                # row 1: below
    for x in xs:
        x[2, 2, int(ids[2, 2])] = -INF                            # row 2: a -inf target in every member
    xs[1][0, 3] = -INF                                            # row 3: member 1 all -inf at t = 0
    xs[2][1, 4, 9] = NAN                                          # row 4: a NaN in member 2 at t = 1
    for M in (1, 3):
        members = xs[1:2] if M == 1 else xs
        want = seq_logprob_f64(members, WEIGHTS[M], mode, ids, None, 0.5, END)
        got = hip.seq_logprob([x.cuda() for x in members], WEIGHTS[M], mode, ids.cuda(), None, 0.5, True, True, end=END)
        tok, w = got[3].cpu().double(), want['tok_lp']
        assert torch.equal(tok.isnan(), w.isnan()) and torch.equal(tok == -INF, w == -INF), (M, tok, w)
        fin = w.isfinite()
        assert float((tok[fin] - w[fin]).abs().max()) <= 1e-5
        assert torch.equal(got[4].cpu().long()[~fin], want['tok_rank'][~fin])
        assert torch.equal(got[2].cpu().isnan(), want['lp'].isnan()) and torch.equal(got[0].cpu().isnan(), want['scores'].isnan())
        assert math.isnan(float(got[2][0])) and math.isnan(float(got[0][1])) and float(got[2][2]) == -INF
        assert bool(got[3][5].isfinite().all()) and bool(got[2][5].isfinite())


# ---------------------------------------------------------------------------------------------- model level
@gpu
def test_reference_parity_on_the_teacher_forced_fixture():
    """model.score of the fixture's captions against log_softmax(golden logits).gather, summed over the counted positions, within
    2e-3 * len"""
    from test_gpu_parity import build
    for tag in ('small_msvd', 'small_baseline1'):
        net, g, frames, regions, caps, lens, kind = build(tag)
        golden = torch.from_numpy(np.asarray(g['logits'])).double()
        assert golden.shape[:2] == caps.shape
        L = caps.shape[1]
        lens = torch.as_tensor(lens, dtype=torch.int64).clamp(max=L)
        logp = torch.log_softmax(golden, 2).gather(2, caps.cpu().unsqueeze(2)).squeeze(2)
        live = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
        want = torch.where(live, logp, torch.zeros_like(logp)).sum(1)
        scores, got_len, tok = net.score(frames, regions, caps, lens=lens.cuda(), return_tokens=True)
        assert torch.equal(got_len.cpu(), lens)
        err = (scores.cpu().double() - want).abs()
        print(tag, 'max |score - golden| %.3g over lens %s' % (float(err.max()), lens.tolist()))
        assert bool((err <= 2e-3 * lens.double()).all())
        assert float((tok.cpu().double() - logp)[live].abs().max()) <= 2e-3


@gpu
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_round_trip_and_graphs(setting):
    """the eight-clip, beam-3 case of the host test on the kernels: a member and the ensemble each get their own search's scores and
    lens back; n candidates on one encoder pass equal n separate calls; the captured forms replay to the eager bits on two batches"""
    nets, frames, regions = build_members()
    nets = [n.cuda() for n in nets]
    ens = dlsg_amd.Ensemble(nets, SETTINGS[setting], setting)
    f1, r1 = frames.cuda(), regions.cuda()
    for scorer in (nets[0], ens):
        search = scorer.beam_search(f1, r1, **OPTS)
        score = scorer.score(f1, r1, search[0], length_penalty=ALPHA, return_tokens=True, return_ranks=True)
        check_round_trip([x.cpu() for x in search], [x.cpu() for x in score])
    ids = ens.beam_search(f1, r1, **OPTS)[0]
    whole = ens.score(f1, r1, ids, return_tokens=True)
    for j in range(K):
        part = ens.score(f1, r1, ids[:, j].contiguous(), return_tokens=True)
        assert torch.equal(part[1], whole[1][:, j]) and float((part[2] - whole[2][:, j]).abs().max()) <= 1e-5
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    ids2 = ids.flip(0).contiguous()
    sg = dlsg_amd.ScoreGraph(ens, f1, r1, ids, length_penalty=ALPHA, return_tokens=True, return_ranks=True)
    rg = dlsg_amd.RescoreBeamGraph(nets[0], ens, f1, r1, n_best=2, mix=0.75, **OPTS)
    for f, r, i in ((f2, r2, ids2), (f1, r1, ids)):
        got = [x.clone() for x in sg(f, r, i)]
        want = ens.score(f, r, i, length_penalty=ALPHA, return_tokens=True, return_ranks=True)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
        got = [x.clone() for x in rg(f, r)]
        want = dlsg_amd.rescore_search(nets[0], ens, f, r, n_best=2, mix=0.75, **OPTS)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert len(rg.held) == 3 and rg.valid_for(f1, r1)
    with pytest.raises(ValueError):
        sg(f1, r1, ids[:, :2])


@gpu
def test_loader_paths(tmp_path):
    nets, frames, regions = build_members()
    nets = [n.cuda() for n in nets]
    args = member_specs()[0][1]
    loader = caption_loader(tmp_path, args, 50, 4, 2, 2, 2, 'cuda')
    batches = list(loader)
    assert len(batches) == 2
    check_perplexity(S.perplexity(nets[0], loader), nets, batches)
    both = S.perplexity(dlsg_amd.Ensemble(nets[:2]), loader)
    assert both['words'] == sum(int(torch.as_tensor(b[5]).clamp(max=args.max_words).sum()) for b in batches)
    ens = dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob')
    f, r = frames[:4].cuda(), regions[:4].cuda()
    vids = ['v%d' % i for i in range(4)]
    got = S.gather_results(nets[0], [(f, r, None, vids)], decode=dict(beam_size=3, rescore=ens))
    ids = dlsg_amd.rescore_search(nets[0], ens, f, r, n_best=1, beam_size=3)[0][:, 0].cpu()
    assert got == {v: nets[0].decoder.decode_tokens(ids[i]) for i, v in enumerate(vids)}

"""GPU (-m gpu): the constrained beam step with phrases (dlsg_beam_select_phrases) against its emulation (tests/emul_phrases.py) on
the step cases of tests/test_phrases_host.py, its reductions to dlsg_beam_select_cons and dlsg_beam_select_hist, padding, launch
behaviour, and `constrained_beam_search` / `ConstrainedBeamGraph` / `gather_results` with phrases on the HIP kernels against the
restated search of that file.  The test without the mark runs on the CPU: it checks the cap on near-ties."""
import functools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from test_beam_nbest_host import close, oracle_stepper, synth_pair
from test_constrained_host import build_cons_case, close_lp, run_cons
from test_phrases_host import (DIMS, END, GAP, check_search_properties, clip_phrases, contains, count_met, emulated_step, fresh,
                               ranked_by_met, reference_phrase_search, run_phrases, step_keys, tensors, widened)

gpu = pytest.mark.gpu
INTS = ('pred', 'back', 'rows', 'hout', 'met', 'bank')


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


@gpu
@pytest.mark.parametrize('L', [26, 64])
@pytest.mark.parametrize('dims', DIMS)
def test_beam_select_phrases_matches_the_emulation(hip, dims, L):
    """clips with a gap of GAP or more: the integer outputs are equal and new_lp agrees to 1e-5; ended_count where every clip of the
    case qualifies"""
    B, k, V = dims
    for key in step_keys([dims], [L]):
        c, want, gap, _, _ = emulated_step(key)
        got = fresh(tensors(c), cuda=True)
        run_phrases(hip, got, key)
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


def same_bits(a, b, outputs, where):
    for o in outputs:
        assert torch.equal(a[o], b[o]), (where, o)
    assert torch.equal(a['nlp'].view(torch.int32), b['nlp'].view(torch.int32)), where


@gpu
@pytest.mark.parametrize('dims', DIMS)
def test_the_reductions_are_bit_for_bit(hip, dims):
    """one-word phrases against hip.beam_select_cons, no constraints against hip.beam_select_hist, padded against unpadded tensors"""
    B, k, V = dims
    for key in step_keys([dims], [26]):
        _, L, g, t, m, cwp = key
        if cwp == (3, 2, 3):
            for cw in ((3, 2), (8, 8)):
                c = build_cons_case(dims, L, t, g, cw, 100 * g + t)
                want, got = fresh(c, cuda=True), fresh(c, cuda=True)
                run_cons(hip, want, (dims, L, g, t, m, cw))
                got['phr'], got['bank'] = got.pop('cons').unsqueeze(3).contiguous(), torch.zeros_like(got['met'])
                run_phrases(hip, got, key)
                same_bits(got, want, ('pred', 'back', 'rows', 'hout', 'cnt', 'met'), (key, cw))
            c = emulated_step(key)[0]
            want, got = fresh(tensors(c), cuda=True), fresh(tensors(c), cuda=True)
            run_phrases(hip, want, key)
            run_phrases(hip, got, key, widened(c['phr'], 8, 8, 4).cuda())
            same_bits(got, want, INTS + ('cnt',), key)
        if cwp == (8, 8, 4):
            c = tensors(emulated_step(key)[0])
            want = fresh(c, cuda=True)
            hip.beam_select_hist(want['lg'][:, 1:V + 1], want['last'], want['lp'], want['pred'], want['nlp'], want['back'], want['rows'], k,
                                 END, want['hist'], want['hout'], t, g, m, ended_count=want['cnt'])
            for phr in (None, torch.zeros(B, 0, 1, 1, dtype=torch.int64), torch.full((B, 8, 8, 4), -1, dtype=torch.int64)):
                got = fresh(c, cuda=True)
                got['met'].fill_(7)
                got['bank'].fill_(7)
                run_phrases(hip, got, key, None if phr is None else phr.cuda())
                same_bits(got, want, ('pred', 'back', 'rows', 'hout', 'cnt'), key)
                assert not bool(got['met'].any()) and not bool(got['bank'].any())


@gpu
def test_two_launches_give_equal_bits_and_bad_arguments_raise(hip):
    key = ((7, 6, 1000), 26, 2, 25, 0, (8, 8, 4))
    c = tensors(emulated_step(key)[0])
    a, b = fresh(c, cuda=True), fresh(c, cuda=True)
    run_phrases(hip, a, key)
    run_phrases(hip, b, key)
    same_bits(a, b, INTS + ('cnt',), key)
    B, k, V = key[0]
    bad = fresh(c, cuda=True)
    for shape in ((B, 1, 1, 5), (B, 9, 1, 1), (B, 1, 9, 1)):            # P = 5, C = 9, W = 9
        with pytest.raises(RuntimeError):
            run_phrases(hip, bad, key, torch.full(shape, -1, dtype=torch.int64).cuda())
    args = (bad['lg'][:, 1:V + 1], bad['last'], bad['lp'], bad['pred'], bad['nlp'], bad['back'], bad['rows'], k, END)
    with pytest.raises(RuntimeError):                                   # t outside the history
        hip.beam_select_phrases(*args, bad['hist'], bad['hout'], 26, bad['phr'])
    with pytest.raises(RuntimeError):                                   # one buffer for both histories
        hip.beam_select_phrases(*args, bad['hist'], bad['hist'], 2, bad['phr'])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- model level
NEAR_TIE = 2e-3                                                        # as tests/test_gpu_beam_nbest.py: the two sides' logits differ by up to 1e-3
MODEL_SEED, MODEL_BIAS = 160, 2.0                                     # chosen by the restatement alone (the test below)
OPTS = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=2, min_len=4)


@functools.lru_cache(maxsize=None)
def restated_case():
    """g = 2, min_len = 4, alpha = 0.7, up to 3 phrase constraints on eight clips of the 50-word model, by the restatement alone: what
    it returns, and per clip the smallest gap its choices and its ranking rest on"""
    net, orc, frames, regions = synth_pair(MODEL_SEED, 8, end_bias=MODEL_BIAS)
    per_clip = clip_phrases(3, batch=8)
    step_fn, start, state, end, L = oracle_stepper(orc, frames, regions)
    toks, lps, gap = reference_phrase_search(step_fn, start, state, end, L, 5, 2, 4, per_clip)
    return (net, frames, regions, per_clip) + tuple(ranked_by_met(toks, lps, gap, per_clip, end, 0.7, 5))


def test_restated_case_stays_inside_the_cap():
    """at most one clip in eight has a near-tie in the restatement itself"""
    gap = restated_case()[-1]
    print('smallest gaps', ['%.1e' % x for x in gap])
    assert sum(g >= NEAR_TIE for g in gap) >= 7


@gpu
def test_phrase_search_matches_the_restated_search():
    net, frames, regions, per_clip, want_ids, want_sc, want_len, want_met, gap = restated_case()
    net = net.cuda()
    phr = dlsg_amd.pack_phrases(per_clip, net.decoder.vocab, 'cuda')
    ids, scores, lens, met = [x.cpu() for x in net.constrained_beam_search(frames.cuda(), regions.cuda(), phr, return_met=True, **OPTS)]
    keep = [b for b in range(8) if gap[b] >= NEAR_TIE]
    assert len(keep) >= 7
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b] and met[b].tolist() == want_met[b], b
        close(scores[b].numpy(), want_sc[b], 1e-4)
    check_search_properties(ids, scores, lens, met, per_clip, END, 2, 4, complete=False)


@gpu
def test_graph_replays_equal_eager_on_two_batches_and_two_phrase_tensors():
    net, orc, frames, regions = synth_pair(36, 8, end_bias=1.0)
    net = net.cuda()
    vocab = net.decoder.vocab
    opts = dict(beam_size=3, length_penalty=0.7, no_repeat_ngram=2, min_len=4, return_met=True)
    f1, r1 = frames.cuda(), regions.cuda()
    f2, r2 = f1.flip(0).contiguous() * 0.5, r1.flip(0).contiguous()
    p1 = dlsg_amd.pack_phrases([[[(10 + b, 20 + b), 25 + b], (30 + b, 31 + b, 32 + b)] for b in range(8)], vocab, 'cuda')
    p2 = dlsg_amd.pack_phrases([[[(40 - b, 12), (41, 42, 43)], [] if b % 2 else 25] for b in range(8)], vocab, 'cuda')
    assert p1.shape == p2.shape == (8, 2, 2, 3)
    graph = dlsg_amd.ConstrainedBeamGraph(net, f1, r1, p1, **opts)
    for f, r, p in ((f2, r2, p2), (f1, r1, p1), (f1, r1, p2)):
        got = [x.clone() for x in graph(f, r, p)]
        want = net.constrained_beam_search(f, r, p, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    lists = [[(10 + b, 20 + b)] for b in range(8)]                      # lists are packed and padded to the captured shape
    got = [x.clone() for x in graph(f1, r1, lists)]
    assert all(torch.equal(a, b) for a, b in zip(got, net.constrained_beam_search(f1, r1, dlsg_amd.pack_phrases(lists, vocab, 'cuda'), **opts)))
    assert not torch.equal(net.constrained_beam_search(f1, r1, p1, **opts)[0], net.constrained_beam_search(f1, r1, p2, **opts)[0])
    for bad in (torch.full((8, 3, 2, 3), -1, dtype=torch.int64, device='cuda'), torch.full((8, 2, 2), -1, dtype=torch.int64, device='cuda')):
        with pytest.raises(ValueError):
            graph(f1, r1, bad)
    assert net.decoder.beam_size == 5


@gpu
def test_batch16_beam5_three_two_word_phrases_are_all_met():
    net, orc, frames, regions = synth_pair(7, 16, end_bias=0.5)
    net = net.cuda()
    rng = np.random.RandomState(3)
    per_clip = [[tuple(int(v) for v in rng.choice(np.arange(4, 50), size=2, replace=False)) for c in range(3)] for _ in range(16)]
    out = net.constrained_beam_search(frames.cuda(), regions.cuda(), dlsg_amd.pack_phrases(per_clip, net.decoder.vocab, 'cuda'),
                                      beam_size=5, no_repeat_ngram=0, min_len=4, length_penalty=0.7, return_met=True)
    assert out[0].shape == (16, 5, net.decoder.max_words)
    clips = [[[list(a)] for a in clip] for clip in per_clip]
    check_search_properties(*out, clips, END, 0, 4)
    ids = out[0].cpu()
    assert all(contains(ids[b, 0].tolist(), a) for b in range(16) for a in per_clip[b])
    assert torch.equal(dlsg_amd.phrases_met(out[0], dlsg_amd.pack_phrases(per_clip, net.decoder.vocab, 'cuda')), out[3])
    free = net.beam_search(frames.cuda(), regions.cuda(), beam_size=5, n_best=1)[0][:, 0].cpu()
    assert sum(count_met(free[b].tolist(), clips[b], END) == 3 for b in range(16)) < 8        # the constraints are not idle


@gpu
def test_gather_results_returns_captions_with_the_required_phrases():
    net, _, frames, regions = synth_pair(11, 3)
    net = net.cuda()
    w = net.decoder.vocab.idx2word
    need = {'v0': ['%s %s' % (w[20], w[21])], 'v1': [['%s %s %s' % (w[22], w[23], w[24]), w[25]], w[26]], 'v2': []}
    loader = [(frames.cuda(), regions.cuda(), None, ['v0', 'v1', 'v2'])]
    got = S.gather_results(net, loader, decode=dict(beam_size=3, constraints=lambda vids: [need[v] for v in vids]))
    assert got['v2'] == S.gather_results(net, loader, decode=dict(beam_size=3))['v2']
    for vid, cons in need.items():
        for con in cons:
            assert any(' %s ' % a in ' %s ' % got[vid] for a in (con if isinstance(con, list) else [con])), (vid, got[vid])

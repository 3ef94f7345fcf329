"""CPU: scoring given captions (`dlsg_amd.rescore`, `scoring.perplexity`, `gather_results(decode=dict(rescore=...))`) through the
emulated kernels: tests/emul_seqscore.py restates dlsg_seq_logprob in float64.  The kernel-level cases, the three-member round
trip and the loader are shared with the GPU side, tests/test_gpu_rescore.py, which imports them from here."""
import functools
import importlib
import math
import pickle

import pytest
import torch

import dlsg_amd
from dlsg_amd import data as D
from dlsg_amd import scoring as S
from dlsg_amd.hip import normalised_weights
from dlsg_amd.synth import synth_batch
from emul_seqscore import SeqScoreEmul, seq_logprob_f64
from test_ensemble_host import CLIPS, SETTINGS, build_members

INF, NAN = float('inf'), float('nan')
END = 3
K, ALPHA = 3, 0.7
WEIGHTS = {1: [1.0], 3: [0.5, 0.3, 0.2], 8: [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]}
# every V, L, R and M of the list is used, both layouts and a padded row stride with each M: (V, L, R, M, layout, pad)
KERNEL_CASES = [(50, 1, 1, 1, 'tm', 0), (64, 5, 3, 3, 'bm', 0), (65, 26, 17, 8, 'tm', 7), (1000, 64, 3, 1, 'bm', 24),
                (4099, 5, 17, 3, 'tm', 1), (4099, 26, 3, 8, 'bm', 0), (1000, 26, 17, 3, 'bm', 9), (65, 64, 1, 1, 'tm', 3),
                (50, 5, 3, 8, 'tm', 0), (64, 1, 17, 3, 'tm', 5), (4099, 64, 1, 1, 'bm', 0), (1000, 5, 1, 8, 'bm', 40)]


@functools.lru_cache(maxsize=None)
def kernel_case(V, L, R, M, layout, pad):
    """The members' logits, 4 x standard normal, as (L, R, V) views of the layout's buffers with rows V + pad apart; ids with
    half the targets the row's argmax under the first member and half random, <end> = 3 at a random place in two rows of three
    (the third has none); never modified"""
    g = torch.Generator().manual_seed(V * 131 + L * 17 + R * 5 + M)
    views = []
    for _ in range(M):
        buf = torch.randn((L, R, V + pad) if layout == 'tm' else (R, L, V + pad), generator=g) * 4.0
        views.append(buf[:, :, :V] if layout == 'tm' else buf.transpose(0, 1)[:, :, :V])
    ids = torch.randint(0, V, (R, L), generator=g)
    ids[ids == END] = END + 1
    top = views[0].argmax(2).t()
    ids = torch.where(torch.rand(R, L, generator=g) < 0.5, top, ids)
    for r in range(R):
        if r % 3 != 2:
            ids[r, int(torch.randint(0, L, (1,), generator=g))] = END
    return views, ids.contiguous()


def plain_logprob(views, weights, mode, ids):
    """log_softmax(...).gather in float64, combined over the members: (R, L), every position"""
    w = normalised_weights(weights)
    lp = [torch.log_softmax(x.double(), 2).gather(2, ids.t().unsqueeze(2)).squeeze(2).t() for x in views]
    if mode == 0:
        return torch.logsumexp(torch.stack([l + math.log(wm) for l, wm in zip(lp, w)]), 0)
    return sum(wm * l for l, wm in zip(lp, w))


# ---------------------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('case', KERNEL_CASES)
def test_emulation_is_log_softmax_gather(case, mode):
    V, L, R, M = case[:4]
    views, ids = kernel_case(*case)
    out = seq_logprob_f64(views, WEIGHTS[M], mode, ids, None, ALPHA, END)
    want = plain_logprob(views, WEIGHTS[M], mode, ids)
    is_end = ids == END
    lens = torch.where(is_end.any(1), is_end.int().argmax(1) + 1, torch.full((R,), L))
    assert torch.equal(out['lens'], lens)
    live = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    assert float((out['tok_lp'] - want)[live].abs().max()) <= 1e-12
    assert bool((out['tok_lp'][~live] == 0).all()) and bool((out['tok_rank'][~live] == -1).all())
    lp = torch.where(live, want, torch.zeros_like(want)).sum(1)
    assert float((out['lp'] - lp).abs().max()) <= 1e-10
    assert float((out['scores'] - lp / lens.double() ** ALPHA).abs().max()) <= 1e-10
    # a target that is the first member's argmax has rank 0 with one member
    if M == 1:
        top = views[0].argmax(2).t()
        assert bool((out['tok_rank'][live & (ids == top)] == 0).all())
        assert bool((out['tok_rank'][live & (ids != top)] > 0).all())


def test_length_and_token_rules():
    V, L = 9, 6
    g = torch.Generator().manual_seed(5)
    x = torch.randn(L, 7, V, generator=g) * 4.0
    x[1, 5, 4] = -INF                                            # row 5 aims at a -inf logit at t = 1
    ids = torch.tensor([[END, 1, 2, 4, 5, 6],                    # <end> at position 0: one word
                        [1, 2, 4, 5, 6, 7],                      # no <end>: L words
                        [1, 2, END, 4, END, 5],                  # the first <end> counts
                        [1, V, 2, END, 1, 1],                    # a target above the vocabulary
                        [-1, 2, END, 1, 1, 1],                   # and one below
                        [1, 4, END, 1, 1, 1],                    # the -inf target
                        [1, 2, 4, 5, 6, END]])
    out = seq_logprob_f64([x], [1.0], 0, ids, None, 1.0, END)
    assert out['lens'].tolist() == [1, 6, 3, 4, 3, 3, 6]
    logp = torch.log_softmax(x.double(), 2)
    assert abs(float(out['lp'][0]) - float(logp[0, 0, END])) <= 1e-12
    assert abs(float(out['scores'][2]) - float(logp[0, 2, 1] + logp[1, 2, 2] + logp[2, 2, END]) / 3.0) <= 1e-12
    for r, t in ((3, 1), (4, 0)):
        assert math.isnan(float(out['tok_lp'][r, t])) and int(out['tok_rank'][r, t]) == -1
        assert math.isnan(float(out['lp'][r])) and math.isnan(float(out['scores'][r]))
        other = [u for u in range(int(out['lens'][r])) if u != t]
        assert bool(out['tok_lp'][r, other].isfinite().all()) and bool((out['tok_rank'][r, other] >= 0).all())
    assert float(out['tok_lp'][5, 1]) == -INF and float(out['lp'][5]) == -INF and float(out['scores'][5]) == -INF
    assert int(out['tok_rank'][5, 1]) == V - 1
    # given lens: 0, inside, L, above L and negative; <end> is then a word like any other
    lens = torch.tensor([0, 2, 6, 9, -3, 1, 4])
    out = seq_logprob_f64([x], [1.0], 0, ids, lens, 0.5, END)
    assert out['lens'].tolist() == [0, 2, 6, 6, 0, 1, 4]
    assert float(out['lp'][0]) == 0.0 and float(out['scores'][0]) == 0.0 and float(out['scores'][4]) == 0.0
    assert bool((out['tok_rank'][0] == -1).all()) and bool((out['tok_lp'][4] == 0).all())
    assert abs(float(out['lp'][2]) - float(sum(logp[t, 2, ids[2, t]] for t in range(6)))) <= 1e-12
    assert abs(float(out['scores'][6]) - float(sum(logp[t, 6, ids[6, t]] for t in range(4))) / 2.0) <= 1e-12


@pytest.mark.parametrize('mode', [0, 1])
def test_special_member_rows(mode):
    """a member row that is all -inf or holds a NaN has a NaN log-sum-exp: NaN with one member and in mode 1; in mode 0 NaN where
    another member gives the class a value above -inf, -inf where none does"""
    V, L, R = 12, 2, 4
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(L, R, V, generator=g) * 4.0 for _ in range(3)]
    xs[1][0, 0] = -INF                                           # (t 0, r 0): member 1 all -inf
    xs[2][0, 1, 5] = NAN                                         # (t 0, r 1): member 2 holds a NaN
    xs[0][0, 2, 7] = -INF; xs[1][0, 2] = NAN; xs[2][0, 2, 7] = -INF    # (t 0, r 2): class 7 has no finite member
    ids = torch.tensor([[4, END], [5, END], [7, END], [4, END]])
    out = seq_logprob_f64(xs, WEIGHTS[3], mode, ids, None, 0.0, END)
    for r in (0, 1):
        assert math.isnan(float(out['tok_lp'][r, 0])) and int(out['tok_rank'][r, 0]) == 0
    if mode == 0:
        assert float(out['tok_lp'][2, 0]) == -INF and int(out['tok_rank'][2, 0]) == 0     # the only -inf among NaNs
    else:
        assert math.isnan(float(out['tok_lp'][2, 0]))
    assert bool(out['tok_lp'][3].isfinite().all()) and bool(out['tok_lp'][:, 1].isfinite().all())
    one = seq_logprob_f64([xs[1]], [1.0], mode, ids, None, 0.0, END)
    assert math.isnan(float(one['tok_lp'][0, 0])) and math.isnan(float(one['tok_lp'][2, 0])) and math.isfinite(float(one['tok_lp'][1, 0]))


# ---------------------------------------------------------------------------------------------- rescore
def test_rescore_orders_mixes_and_cuts(monkeypatch):
    RS = importlib.import_module('dlsg_amd.rescore')          # (the package exports the function `rescore` under that name)
    new = torch.tensor([[-1.0, -0.5, -0.5, -2.0], [-3.0, -1.0, -2.0, -0.1]])
    monkeypatch.setattr(RS, 'score_captions', lambda scorer, f, r, ids, lens=None, length_penalty=0.0: (
        new.clone(), torch.full(new.shape, 2, dtype=torch.int64) if lens is None else lens))
    ids = torch.arange(2 * 4 * 5).view(2, 4, 5)
    out_ids, sc, lens, order = RS.rescore(None, None, None, ids)
    assert order.tolist() == [[1, 2, 0, 3], [3, 1, 2, 0]]                    # the tie keeps the input order
    assert torch.equal(sc, torch.tensor([[-0.5, -0.5, -1.0, -2.0], [-0.1, -1.0, -2.0, -3.0]]))
    assert torch.equal(out_ids, torch.gather(ids, 1, order.unsqueeze(2).expand(-1, -1, 5))) and lens.shape == (2, 4)
    old = torch.tensor([[-0.1, -4.0, -INF, -0.2], [NAN, -1.0, -1.0, -9.0]])
    given = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]])
    out_ids, sc, lens, order = RS.rescore(None, None, None, ids, old, given)
    assert order.tolist() == [[1, 0, 3, 2], [3, 1, 2, 0]]                    # invalid candidates last, their score -inf
    assert float(sc[0, 3]) == -INF and float(sc[1, 3]) == -INF and torch.equal(lens, torch.gather(given, 1, order))
    out_ids, sc, lens, order = RS.rescore(None, None, None, ids, old, given, mix=0.25, n_best=2)
    mixed = 0.25 * new + 0.75 * old
    assert order.tolist() == [[0, 3], [1, 2]] and sc.shape == (2, 2) and out_ids.shape == (2, 2, 5)
    assert torch.allclose(sc, torch.gather(mixed, 1, order))
    assert RS.rescore(None, None, None, ids, old, mix=0.0)[3].tolist() == [[0, 3, 1, 2], [1, 2, 3, 0]]   # the incoming order
    for bad in (dict(mix=0.5), dict(scores=old, mix=1.5), dict(scores=old, mix=-0.1), dict(n_best=0), dict(n_best=5),
                dict(scores=old[:, :3]), dict(scores=old.double())):
        with pytest.raises(ValueError):
            RS.rescore(None, None, None, ids, **bad)
    with pytest.raises(ValueError):
        RS.rescore(None, None, None, ids[0])


# ---------------------------------------------------------------------------------------------- the whole path
OPTS = dict(beam_size=K, length_penalty=ALPHA, no_repeat_ngram=2, min_len=4)


@functools.lru_cache(maxsize=None)
def searched(setting):
    """the three-member case's own beam search through the emulated ops (never modified): (ids, scores, lens)"""
    nets, frames, regions = build_members(ops=SeqScoreEmul())
    return dlsg_amd.Ensemble(nets, SETTINGS[setting], setting).beam_search(frames, regions, **OPTS)


def check_round_trip(search, score):
    """`score` = scorer.score(frames, regions, ids, length_penalty=ALPHA, return_tokens=True, return_ranks=True) on the
    scorer's own `search`: the search's lens exactly and its scores within 2e-3 * len / len^alpha (the logits parity bound, 1e-3
    per logit, once on x and once on lse, per word)"""
    ids, scores, lens = search
    got_sc, got_len, tok, rank = score
    assert got_sc.shape == scores.shape and got_len.shape == lens.shape and tok.shape == ids.shape and rank.shape == ids.shape
    assert torch.equal(got_len, lens)
    tol = 2e-3 * lens.double() / lens.double() ** ALPHA
    err = (got_sc.double() - scores.double()).abs()
    print('round trip: max |score difference| %.3g, smallest bound %.3g' % (float(err.max()), float(tol.min())))
    assert bool((err <= tol).all())
    live = torch.arange(ids.shape[-1]).view(1, 1, -1) < lens.unsqueeze(2)
    assert bool((tok[~live] == 0).all()) and bool((rank[~live] == -1).all()) and bool((rank[live] >= 0).all())
    # a beam of K keeps words among a row's K best that are not banned: min_len bans <end>, the bigram ban at most len words
    assert bool((rank[live] < K + 1 + ids.shape[-1]).all()) and bool((rank[live] < K).any())


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_ensemble_scores_its_own_search(setting):
    nets, frames, regions = build_members(ops=SeqScoreEmul())
    ens = dlsg_amd.Ensemble(nets, SETTINGS[setting], setting)
    ids = searched(setting)[0]
    check_round_trip(searched(setting), ens.score(frames, regions, ids, length_penalty=ALPHA, return_tokens=True, return_ranks=True))
    # the encoder once per clip: (B, n, L) equals n calls of (B, L)
    whole = ens.score(frames, regions, ids, return_tokens=True)
    for j in range(K):
        part = ens.score(frames, regions, ids[:, j].contiguous(), return_tokens=True)
        assert torch.equal(part[1], whole[1][:, j]) and float((part[2] - whole[2][:, j]).abs().max()) <= 1e-5
    # a model scores like the ensemble of itself, and the module-level form is the method
    one = nets[0].score(frames, regions, ids, length_penalty=ALPHA)
    same = dlsg_amd.score_captions(dlsg_amd.Ensemble([nets[0]]), frames, regions, ids, length_penalty=ALPHA)
    assert torch.equal(one[0], same[0]) and torch.equal(one[1], same[1]) and not torch.equal(one[0], whole[0])


def test_rescore_search_and_value_errors():
    nets, frames, regions = build_members(ops=SeqScoreEmul())
    ens = dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob')
    ids, scores, lens = nets[0].beam_search(frames, regions, **OPTS)
    got = dlsg_amd.rescore_search(nets[0], ens, frames, regions, n_best=2, **OPTS)
    want = dlsg_amd.rescore(ens, frames, regions, ids, scores, lens, length_penalty=ALPHA, n_best=2)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[0].shape == (CLIPS, 2, ids.shape[2])
    new = ens.score(frames, regions, ids, length_penalty=ALPHA)[0]
    assert torch.equal(got[3], new.sort(dim=1, descending=True, stable=True)[1][:, :2])
    assert bool((got[3][:, 0] != 0).any())                       # the ensemble does not agree with the member everywhere
    own = dlsg_amd.rescore_search(nets[0], nets[0], frames, regions, n_best=K, mix=0.5, **OPTS)
    assert torch.equal(own[0], ids)                              # a model's own ranking survives its own rescoring
    L = nets[0].decoder.max_words
    long_ids = torch.full((CLIPS, L + 1), END, dtype=torch.int64)
    for bad in (lambda: ens.score(frames, regions, long_ids), lambda: ens.score(frames, regions, ids.int()),
                lambda: ens.score(frames, regions, ids[0, 0]), lambda: ens.score(frames, regions, ids.unsqueeze(0)),
                lambda: ens.score(frames, regions, ids, lens=lens[:, :2]), lambda: ens.score(frames, regions, ids, length_penalty=-1.0),
                lambda: ens.score(frames, regions, ids, length_penalty=NAN), lambda: ens.score(frames[:3], regions[:3], ids)):
        with pytest.raises(ValueError):
            bad()
    from helpers import small_args
    stranger = dlsg_amd.CapGnnModel(small_args(dropout=0.0), dlsg_amd.make_vocab(51)).eval()
    with pytest.raises(ValueError, match='vocabulary'):
        dlsg_amd.Ensemble([nets[0], stranger]).score(frames, regions, ids)


# ---------------------------------------------------------------------------------------------- loaders
def caption_loader(tmp_path, args, V, clips, sentences, batch, n, device, seed=21):
    """a real TrainLoader over `clips` synthetic clips with `sentences` captions each: captions U{4..V-1} of lengths 3 .. max_words,
    padded with 0"""
    g = torch.Generator().manual_seed(seed)
    frames, regions, _, _ = synth_batch(args, V, clips, seed)
    L = args.max_words
    vids = [v for v in range(clips) for _ in range(sentences)]
    lens = torch.randint(3, L + 1, (len(vids),), generator=g).tolist()
    caps = []
    for ln in lens:
        row = torch.zeros(L, dtype=torch.int64)
        row[:ln] = torch.randint(4, V, (ln,), generator=g)
        caps.append(row)
    path = str(tmp_path / 'caps.pkl')
    with open(path, 'wb') as f:
        pickle.dump((caps, [torch.zeros(L, dtype=torch.int64) for _ in caps], lens, vids), f)
    store = D.ResidentFeatures.from_arrays(frames, regions, args.num_obj, device)
    return D.TrainLoader(D.CaptionSet(path), store, batch, shuffle=False, seed=3, captions_per_clip=n)


def check_perplexity(got, nets, batches):
    """against the `ce_ragged` loss of every batch's eval-mode teacher-forced logits (what the train step reports), to 1e-4
    relative: a float32 sum over a few hundred rows against float64"""
    ops = nets[0].ops
    total, words = 0.0, 0
    for frames, regions, _, caps, _, cap_lens, _ in batches:
        n = caps.shape[0] // frames.shape[0]
        lg = dlsg_amd.Ensemble([nets[0]]).teacher_logits(frames, regions, caps, seq_per_clip=n)[0]
        lens = torch.as_tensor(cap_lens, dtype=torch.int64, device=caps.device)
        loss = torch.empty(1, dtype=torch.float32, device=caps.device)
        ops.ce_ragged(lg, caps, lens, torch.empty_like(lg), torch.empty(lg.shape[0] * lg.shape[1], dtype=torch.float32, device=caps.device),
                      loss, time_major=True)
        cnt = int(lens.clamp(max=caps.shape[1]).sum())
        total, words = total + float(loss) * cnt, words + cnt
    print('perplexity: nll %.6f against ce_ragged %.6f over %d words' % (got['nll'], total / words, words))
    assert got['words'] == words and abs(got['nll'] - total / words) <= 1e-4 * total / words
    assert abs(got['ppl'] - math.exp(got['nll'])) <= 1e-9 * got['ppl'] and 0.0 <= got['top1'] <= got['top5'] <= 1.0


@pytest.mark.parametrize('n', [1, 2])
def test_perplexity_is_the_train_steps_loss(tmp_path, n):
    nets, _, _ = build_members(ops=SeqScoreEmul())
    from test_ensemble_host import member_specs
    args = member_specs()[0][1]
    loader = caption_loader(tmp_path, args, 50, 4, 3, 4, n, 'cpu')
    batches = list(loader)
    assert len(batches) == (3 if n == 1 else 1)
    got = S.perplexity(nets[0], loader)
    check_perplexity(got, nets, batches)
    # random captions: the model ranks about 1 word in V first
    assert got['top1'] < 0.5
    ens = S.perplexity(dlsg_amd.Ensemble(nets[:2]), loader)
    assert ens['words'] == got['words'] and ens['nll'] != got['nll']
    with pytest.raises(ValueError):
        S.perplexity(nets[0], [])


def test_gather_results_rescored():
    nets, frames, regions = build_members(ops=SeqScoreEmul())
    ens = dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob')
    f, r = frames[:4], regions[:4]
    vids = ['v%d' % i for i in range(4)]
    loader = [(f, r, None, vids)]
    got = S.gather_results(nets[0], loader, decode=dict(OPTS, rescore=ens))
    ids = dlsg_amd.rescore_search(nets[0], ens, f, r, n_best=1, **OPTS)[0][:, 0]
    assert got == {v: nets[0].decoder.decode_tokens(ids[i]) for i, v in enumerate(vids)}
    mixed = S.gather_results(nets[0], loader, decode=dict(OPTS, rescore=ens, rescore_mix=0.0))
    assert mixed == S.gather_results(nets[0], loader, decode=OPTS)           # mix 0: the search's own best beam
    for other in (dict(consensus=object()), dict(constraints=lambda v: [])):
        with pytest.raises(ValueError, match='rescore'):
            S.gather_results(nets[0], loader, decode=dict(OPTS, rescore=ens, **other))

"""CPU: stochastic beam search (sampling without replacement) -- the emulated step (tests/emul_sbs.py) against the rules it restates
on the step cases that tests/test_gpu_sbs.py runs on the kernel; its distribution on a toy tree whose 40 sequences can be
enumerated, against the exact probabilities of sampling without replacement, and the importance weights of the threshold; and
`beam.stochastic_nbest` / `sample_without_replacement` / `consensus_search(stochastic=...)` through the emulated ops on a small
host model."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.beam import check_stochastic_options
from dlsg_amd.engine import SITE_SAMPLE
from emul_beam import banned_classes
from emul_sbs import INF, SbsEmul, gumbel_step, root_values
from test_beam_nbest_host import close, has_repeat, synth_pair, words_of
from test_cider_device_host import corpus_for

END = 2
DIMS = [(3, 4, 50), (7, 6, 1000), (4, 8, 10007), (2, 2, 40), (5, 1, 50), (2, 8, 8)]
# Ten times the float32 error of a key or a perturbed value: both stay below about 40 in magnitude, where one float32 step is 3.8e-6
GAP = 1e-4
TEMPERATURES = (1.0, 0.7)
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt', 'gout')
STEP_SEED = 0x5B5


# ---------------------------------------------------------------------------------------------- step cases (shared with the GPU tests)
def steps_of(L, g):
    return sorted({t for t in (0, 1, g - 1, g, L - 1) if 0 <= t < L})


def step_keys():
    """(dims, L, g, t, min_len, temperature) of every step case"""
    return [(dims, L, g, t, m, temp) for dims in DIMS for L in (26, 64) for g in (0, 2) for t in steps_of(L, g) for m in (0, t + 1)
            for temp in TEMPERATURES]


def build_case(dims, L, t, g, seed):
    """One step's inputs, in the manner of `step_case` of tests/test_gpu_beam_nbest.py: logits behind a strided view with a few -inf
    and NaN entries, ~40 % ended beams and clip 0 ended altogether, <end> lifted in a third of the rows (so a minimum length bites),
    the last clip live and without the lift, histories that start with a token of the row's own (so the rows of a clip differ,
    where the vocabulary has room) and whose last g - 1 tokens repeat their first g - 1, which the row's best class follows (so the
    n-gram ban hits the top of every live row); log-probs in (-5, 0] and perturbed values a Gumbel away from them."""
    B, k, V = dims
    R_ = B * k
    gen = torch.Generator().manual_seed(seed)
    lg = torch.randn(R_, V + 3, generator=gen) * 3.0
    lift = torch.rand(R_, generator=gen) < 0.33
    lift[-k:] = False
    lg[lift, 1 + END] = 15.0
    nb = min(k + 2, V)
    best = lg[:, 1:V + 1].topk(nb)[1]
    if V >= 40:                                                        # two classes per row that can never be chosen
        off = torch.randint(3, V, (R_, 2), generator=gen)
        lg[torch.arange(R_), 1 + off[:, 0]] = -INF
        lg[torch.arange(R_), 1 + off[:, 1]] = float('nan')
        best = torch.where(torch.isnan(lg[:, 1:V + 1]), torch.full((), -INF), lg[:, 1:V + 1]).topk(nb)[1]
    hist = torch.full((R_, L), END, dtype=torch.int64)
    if t:
        hist[:, :t] = best.gather(1, torch.randint(0, nb, (R_, t), generator=gen))
        hist[:, :t][hist[:, :t] == END] = 3
        if V >= k + 4:
            hist[:, 0] = 3 + torch.arange(R_) % k
        if g and t >= g:
            top = torch.where(best[:, 0] == END, best[:, 1], best[:, 0])
            if t <= 2 * g - 2:
                hist[:, :t] = top.unsqueeze(1)
            else:
                hist[:, t - g + 1:t] = hist[:, :g - 1]
                hist[:, g - 1] = top
        last = hist[:, t - 1].clone()
        last[torch.rand(R_, generator=gen) < 0.4] = END
        last[:k] = END
        last[-k:] = hist[-k:, t - 1]
    else:
        last = torch.full((R_,), 1, dtype=torch.int64)
    lp = -torch.rand(R_, generator=gen) * 5
    u = torch.rand(R_, generator=gen, dtype=torch.float64).clamp_(1e-9, 1 - 1e-9)
    return dict(lg=lg, last=last, lp=lp, gin=lp.double() - torch.log(-torch.log(u)), hist=hist, hout=torch.zeros(R_, L, dtype=torch.int64),
                pred=torch.zeros(R_, dtype=torch.int64), nlp=torch.zeros(R_), back=torch.zeros(R_, dtype=torch.int64),
                rows=torch.zeros(R_, dtype=torch.int64), cnt=torch.zeros(1, dtype=torch.int32), gout=torch.zeros(R_, dtype=torch.float64))


def run_gumbel(ops, c, key, seed=STEP_SEED):
    dims, L, g, t, m, temp = key
    V = dims[2]
    ops.beam_select_gumbel(c['lg'][:, 1:V + 1], c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'], dims[1], END, c['hist'],
                           c['hout'], t, c['gin'], c['gout'], temperature=temp, seed=seed, site_sample=SITE_SAMPLE, no_repeat_ngram=g,
                           min_len=m, ended_count=c['cnt'])


def fresh(c, cuda=False):
    return {k: (v.cuda() if cuda else v.clone()) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def emulated_step(key):
    """(inputs, emulated outputs, gap (B,), input seeds tried) of a step case, computed once and never modified.  The inputs are
    seeded 100 g + t, then + 1000, + 2000 ... until at least 90 % of the clips have a gap of GAP or more in the emulation: a
    condition on the inputs, which the kernel is never asked about."""
    dims, L, g, t, m, temp = key
    emul = SbsEmul()
    for tries in itertools.count(1):
        c = build_case(dims, L, t, g, 100 * g + t + 1000 * (tries - 1))
        e = fresh(c)
        run_gumbel(emul, e, key)
        if 10 * int((emul.gap >= GAP).sum()) >= 9 * dims[0]:
            return c, {o: e[o] for o in OUTPUTS}, emul.gap, tries


def test_step_cases_leave_few_clips_out():
    keys = step_keys()
    assert len(keys) == 6 * 2 * 7 * 2 * 2
    tries, out, clips = 0, 0, 0
    for key in keys:
        c, _, gap, n = emulated_step(key)
        assert 10 * int((gap >= GAP).sum()) >= 9 * key[0][0], key
        tries, out, clips = max(tries, n), out + int((gap < GAP).sum()), clips + gap.numel()
    print('%d of %d clips below %g; at most %d input seeds tried' % (out, clips, GAP, tries))
    assert tries <= 3


def check_sbs_rules(c, out, key):
    """what a step owes its inputs whatever the rounding: parents inside the clip, nothing banned or dead chosen, G descending and at
    most the parent's T (at step 0 the root's own Gumbel value) with equality for exactly the parent's first child, an ended beam
    goes on with <end> at its phi and its T, and distinct histories stay distinct"""
    dims, L, g, t, m, temp = key
    B, k, V = dims
    x = c['lg'][:, 1:V + 1]
    root = root_values(STEP_SEED, SITE_SAMPLE, B * k, V)               # step 0: the perturbed value of the empty prefix
    for b in range(B):
        s = slice(b * k, (b + 1) * k)
        G = out['gout'][s]
        assert bool((G[:-1] >= G[1:]).all()), (key, b)
        eq = {}
        for q in range(k):
            o = b * k + q
            parent, cls, lp, Gq = int(out['rows'][o]), int(out['pred'][o]), float(out['nlp'][o]), float(G[q])
            assert parent == b * k + int(out['back'][o]) and b * k <= parent < (b + 1) * k and (t or parent == b * k), (key, o)
            assert 0 <= cls < V and (lp > -INF) == (Gq > -INF), (key, o)
            assert out['hout'][o].tolist() == c['hist'][parent, :t].tolist() + [cls] + [END] * (L - t - 1), (key, o)
            if Gq == -INF:
                continue
            T = float(c['gin'][parent]) if t else float(root[parent])
            assert Gq <= T, (key, o)
            if t and int(c['last'][parent]) == END:
                assert cls == END and lp == float(c['lp'][parent]) and Gq == T, (key, o)
                continue
            assert cls not in banned_classes(c['hist'][parent, :t].tolist(), t, g, m, END) and float(x[parent, cls]) > -INF, (key, o)
            eq.setdefault(parent, []).append(Gq == T)
        for parent, flags in eq.items():                              # the children of a parent come in G order: the first one has T
            assert flags[0] and not any(flags[1:]), (key, b, parent)
        before = {tuple(r) for r in c['hist'][s, :t].tolist()}
        if t == 0 or len(before) == k:
            assert len({tuple(r) for r in out['hout'][s].tolist()}) == k, (key, b)
    return sum(1 for b in range(B) if t == 0 or len({tuple(r) for r in c['hist'][b * k:(b + 1) * k, :t].tolist()}) == k)


def test_the_emulated_step_keeps_the_rules():
    distinct, clips, bans, short = 0, 0, 0, 0
    for key in step_keys():
        c, out, gap, _ = emulated_step(key)
        distinct += check_sbs_rules(c, out, key)
        clips += key[0][0]
        short += int((out['gout'] == -INF).sum())
        if key[2] and key[3] >= key[2]:                                # the n-gram ban changes what is chosen
            off = fresh(c)
            run_gumbel(SbsEmul(), off, key[:2] + (0,) + key[3:])
            bans += not torch.equal(off['pred'], out['pred'])
    print('%d of %d clips had distinct histories; the ban changed %d cases; %d slots left empty' % (distinct, clips, bans, short))
    assert 2 * distinct >= clips and bans > 20 and short > 0


def test_the_step_renormalises_and_tempers():
    """written out on one row: phi of a child is log softmax(x / temperature) over the classes that are left"""
    x = torch.tensor([[0.0, 1.0, 2.0, 3.0, -INF, float('nan')]])
    out = gumbel_step(x.numpy(), np.array([1]), np.zeros(1), np.zeros((1, 4), dtype=np.int64), 1, END, 0, np.zeros(1), 0.5, 9,
                      SITE_SAMPLE, 0, 1)
    z = np.array([0.0, 2.0, 6.0])                                      # <end> = 2 is banned by min_len, 4 and 5 are dead
    want = z - np.log(np.exp(z).sum())
    cls = int(out['pred'][0])
    assert cls in (0, 1, 3) and abs(out['new_lp'][0] - want[[0, 1, 3].index(cls)]) <= 1e-12
    assert out['G'][0] == root_values(9, SITE_SAMPLE, 1, 6)[0]        # the one child takes the root's value


# ---------------------------------------------------------------------------------------------- the distribution, on a toy tree
TOY_V, TOY_L, TOY_N = 4, 3, 20000


@functools.lru_cache(maxsize=None)
def toy_tree(seed=5):
    """vocabulary 4 with <end> = 2, 3 words: the conditional logits of every prefix, and the probability and the length of each of
    the 64 codes h0 * 16 + h1 * 4 + h2 (40 of them are end-padded sequences, the others have probability 0)"""
    rng = np.random.RandomState(seed)
    tabs = [(rng.randn(TOY_V ** t, TOY_V) * 1.5).astype(np.float32) for t in range(TOY_L)]
    logp = [t.astype(np.float64) - np.log(np.exp(t.astype(np.float64)).sum(1, keepdims=True)) for t in tabs]
    p, ln = np.zeros(64), np.zeros(64)
    for h0, h1, h2 in itertools.product(range(TOY_V), repeat=3):
        if (h0 == END and (h1, h2) != (END, END)) or (h1 == END and h2 != END):
            continue
        lp = logp[0][0, h0] + (0.0 if h0 == END else logp[1][h0, h1]) + (0.0 if END in (h0, h1) else logp[2][h0 * 4 + h1, h2])
        p[h0 * 16 + h1 * 4 + h2] = math.exp(lp)
        ln[h0 * 16 + h1 * 4 + h2] = 1 if h0 == END else 2 if h1 == END else 3
    assert int((p > 0).sum()) == 40 and abs(p.sum() - 1.0) <= 1e-12
    return tabs, p, ln


@functools.lru_cache(maxsize=None)
def toy_search(k):
    """the emulated search with k beams on TOY_N seeds, every seed a clip of one batch: (codes (N, k) in sampling order, phi, G)"""
    tabs, _, _ = toy_tree()
    seeds = (np.arange(TOY_N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)) & np.uint64(0xFFFFFFFFFFFF)
    R_ = TOY_N * k
    last, lp, G = np.ones(R_, dtype=np.int64), np.zeros(R_), np.zeros(R_)
    hist = np.full((R_, TOY_L), END, dtype=np.int64)
    for t in range(TOY_L):
        code = np.zeros(R_, dtype=np.int64) if t == 0 else hist[:, 0] if t == 1 else hist[:, 0] * 4 + hist[:, 1]
        out = gumbel_step(tabs[t][code], last, lp, hist, k, END, t, G, 1.0, seeds, SITE_SAMPLE)
        hist = hist[out['rows']]
        hist[:, t] = out['pred']
        last, lp, G = out['pred'], out['new_lp'], out['G']
    code = (hist[:, 0] * 16 + hist[:, 1] * 4 + hist[:, 2]).reshape(TOY_N, k)
    return code, lp.reshape(TOY_N, k), G.reshape(TOY_N, k)


def test_toy_tree_inclusion_and_first_pick_frequencies():
    """k = 3: every sequence's inclusion frequency against the exact inclusion probability of 3-fold sampling without replacement,
    and the frequency with which it comes first against its probability; statistics with an expected count of 50 or more, each
    within 4.5 binomial standard deviations (at most 80 statistics: a false alarm has probability below 1e-3)"""
    _, p, _ = toy_tree()
    code, phi, G = toy_search(3)
    assert all(len(set(r)) == 3 for r in code[:2000].tolist()) and bool((p[code] > 0).all())
    assert np.allclose(phi, np.log(p[code]), rtol=0, atol=1e-9) and bool((G[:, :-1] >= G[:, 1:]).all())
    a, b, c = np.meshgrid(p, p, p, indexing='ij')
    i = np.arange(64)
    with np.errstate(divide='ignore', invalid='ignore'):
        P = a * b / (1 - a) * c / (1 - a - b)
    P[i, i, :] = 0
    P[i, :, i] = 0
    P[:, i, i] = 0
    P = np.where(a * b * c > 0, P, 0.0)
    incl = P.sum((1, 2)) + P.sum((0, 2)) + P.sum((0, 1))
    assert abs(P.sum() - 1.0) <= 1e-9 and abs(incl.sum() - 3.0) <= 1e-9
    worst, used = {}, 0
    for name, q, count in (('inclusion', incl, np.bincount(code.reshape(-1), minlength=64)),
                           ('first pick', p, np.bincount(code[:, 0], minlength=64))):
        use = TOY_N * q >= 50
        dev = np.abs(count[use] - TOY_N * q[use]) / np.sqrt(TOY_N * q[use] * (1 - q[use]))
        worst[name], used = float(dev.max()), used + int(use.sum())
        assert int(count[q == 0].sum()) == 0
    print('standard deviations off, at most:', worst, 'over', used, 'statistics')
    assert 20 <= used <= 80 and max(worst.values()) <= 4.5


def test_toy_tree_threshold_gives_unbiased_importance_weights():
    """4 beams, 3 returned, kappa = the fourth's G: the means over the seeds of sum_i w_i len(y_i) and of sum_i w_i against the
    exact E[len] and 1, each within 4.5 of its standard errors"""
    _, p, ln = toy_tree()
    code, phi, G = toy_search(4)
    w = dlsg_amd.importance_weights(torch.from_numpy(phi[:, :3]).float(), torch.from_numpy(G[:, 3])).numpy()
    assert w.dtype == np.float64 and w.shape == (TOY_N, 3) and bool((w >= np.exp(phi[:, :3]) - 1e-7).all())
    worst = {}
    for name, est, exact in (('E[len]', (w * ln[code[:, :3]]).sum(1), float((p * ln).sum())), ('1', w.sum(1), 1.0)):
        se = est.std(ddof=1) / math.sqrt(TOY_N)
        worst[name] = abs(est.mean() - exact) / se
        print('%s: mean %.5f, exact %.5f, standard error %.5f' % (name, est.mean(), exact, se))
    assert max(worst.values()) <= 4.5
    # the plain mean over the three rows is biased towards likely captions: the weights are not idle
    assert abs(ln[code[:, :3]].mean() - float((p * ln).sum())) > 10 * (ln[code[:, :3]].mean(1).std() / math.sqrt(TOY_N))


# ---------------------------------------------------------------------------------------------- the host search
CLIPS = 3


@functools.lru_cache(maxsize=None)
def host_net():
    return synth_pair(11, CLIPS, end_bias=1.0, ops=SbsEmul())


@pytest.mark.parametrize('temperature, seed', [(1.0, 7), (0.7, 123456789), (1.3, 2 ** 40 + 5)])
def test_one_beam_draws_what_sample_draws(temperature, seed):
    net, orc, frames, regions = host_net()
    ids, logp, lens = net.sample_without_replacement(frames, regions, n=1, temperature=temperature, seed=seed)
    want, want_lp, want_len = net.sample(frames, regions, n=1, temperature=temperature, seed=seed)
    L = net.decoder.max_words
    assert ids.shape == (CLIPS, 1, L) and logp.shape == (CLIPS, 1) and lens.shape == (CLIPS, 1)
    assert ids.dtype == torch.int64 and logp.dtype == torch.float32 and lens.dtype == torch.int64
    end = net.decoder.vocab('<end>')
    for b in range(CLIPS):
        n = int(want_len[b])
        assert int(lens[b, 0]) == n and ids[b, 0, :n].tolist() == want[b, :n].tolist() and bool((ids[b, 0, n:] == end).all()), b
        close([float(logp[b, 0])], [float(want_lp[b, :n].double().sum())], 1e-5)


def check_rows(ids, lens, end, g=0, min_len=0):
    for clip, clip_lens in zip(ids.tolist(), lens.tolist()):
        assert len({tuple(r) for r in clip}) == len(clip)
        for row, n in zip(clip, clip_lens):
            words = words_of(row, end)
            assert n == min(len(words) + 1, len(row)) and all(w == end for w in row[len(words):])
            assert (g == 0 or not has_repeat(words, g)) and len(words) >= min_len


def test_rows_are_distinct_padded_and_reproducible():
    net, orc, frames, regions = host_net()
    end = net.decoder.vocab('<end>')
    a = net.sample_without_replacement(frames, regions, n=5, seed=3)
    check_rows(a[0], a[2], end)
    assert len({int(x) for x in a[2].view(-1)}) > 2
    b = net.sample_without_replacement(frames, regions, n=5, seed=3)
    c = dlsg_amd.sample_without_replacement(net, frames, regions, n=5, seed=4)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], c[0])
    d, e = net.sample_without_replacement(frames, regions, n=5), net.sample_without_replacement(frames, regions, n=5)
    assert not torch.equal(d[0], e[0])                                  # seed None: the model's next seed
    opt = net.sample_without_replacement(frames, regions, n=8, temperature=0.8, seed=3, min_len=4, no_repeat_ngram=2)
    check_rows(opt[0], opt[2], end, 2, 4)


def test_threshold_lies_below_the_rows():
    net, orc, frames, regions = host_net()
    ids, logp, lens, gumbel, kappa = net.sample_without_replacement(frames, regions, n=4, seed=3, return_threshold=True)
    assert ids.shape[:2] == (CLIPS, 4) and gumbel.shape == (CLIPS, 4) and kappa.shape == (CLIPS,)
    assert gumbel.dtype == kappa.dtype == torch.float64
    assert bool((gumbel[:, :-1] >= gumbel[:, 1:]).all()) and bool((kappa <= gumbel[:, -1]).all()) and bool(torch.isfinite(kappa).all())
    five = net.sample_without_replacement(frames, regions, n=5, seed=3)
    assert torch.equal(five[0][:, :4], ids) and torch.equal(five[1][:, :4], logp)
    w = dlsg_amd.importance_weights(logp, kappa)
    assert w.dtype == torch.float64 and w.shape == (CLIPS, 4) and bool((w >= logp.double().exp()).all())
    q = -torch.expm1(-(logp.double() - kappa.unsqueeze(1)).exp())
    assert torch.allclose(w * q, logp.double().exp(), rtol=1e-12, atol=0)


def test_value_errors():
    net, orc, frames, regions = host_net()
    L = net.decoder.max_words
    for bad in (dict(n=0), dict(n=9), dict(n=-1), dict(n=8, return_threshold=True), dict(temperature=0.0), dict(temperature=-1.0),
                dict(temperature=float('nan')), dict(min_len=L), dict(min_len=-1), dict(no_repeat_ngram=-2)):
        with pytest.raises(ValueError):
            net.sample_without_replacement(frames, regions, **bad)
    with pytest.raises(ValueError):
        check_stochastic_options(5, 26, 4, 1.0)                         # vocabulary smaller than the beams
    with pytest.raises(ValueError):
        check_stochastic_options(4, 26, 4, 1.0, return_threshold=True)
    with pytest.raises(ValueError):
        check_stochastic_options(5, 65, 50, 1.0)                        # max_words above the history
    assert check_stochastic_options(7, 64, 8, 0.5, 63, 3, True) == 8 and check_stochastic_options(8, 26, 50, 1.0) == 8
    assert net.sample_without_replacement(frames, regions, n=7, return_threshold=True)[0].shape[1] == 7


def test_consensus_search_takes_its_candidates_from_the_stochastic_search():
    net, orc, frames, regions = host_net()
    reward = S.CiderD(corpus_for(net.decoder.vocab, 5)).to_device(net.decoder.vocab, device='cpu')
    reward.ops = net.ops
    opts = dict(n=5, temperature=0.9, seed=21)
    want = dlsg_amd.consensus_rerank(reward, *net.sample_without_replacement(frames, regions, **opts), n_best=3)
    got = dlsg_amd.consensus_search(net, frames, regions, reward, n_best=3, stochastic=opts)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[0].shape[:2] == (CLIPS, 3)
    for bad in (dict(beam_size=5), dict(length_penalty=0.7), dict(num_groups=1)):
        with pytest.raises(ValueError):
            dlsg_amd.consensus_search(net, frames, regions, reward, stochastic=opts, **bad)
    with pytest.raises(ValueError):
        dlsg_amd.consensus_search(dlsg_amd.Ensemble([net]), frames, regions, reward, stochastic=opts)
    plain = dlsg_amd.consensus_search(net, frames, regions, reward, n_best=3, beam_size=5)
    ref = dlsg_amd.consensus_rerank(reward, *net.beam_search(frames, regions, beam_size=5), n_best=3)
    assert all(torch.equal(a, b) for a, b in zip(plain, ref))


def test_library_exports_the_step():
    from dlsg_amd import abi
    assert 'dlsg_beam_select_gumbel' in abi.functions and len(abi.functions['dlsg_beam_select_gumbel'][1]) == 14


# ---------------------------------------------------------------------------------------------- the whole search, restated
# The case of the end-to-end comparison (tests/test_gpu_sbs.py): eight clips, n = 5, the bans on.  The restatement steps the ORACLE
# and selects with `gumbel_step`; the kernels step their own decoder, whose logits differ from the oracle's by up to 1e-3, and a
# perturbed value moves about as far as the log-probs under it.  What decides a search is the order of each clip's k + 1 best
# perturbed values at every step (a near-tie of two keys inside a row shows there, or concerns children nobody takes), so a clip whose
# smallest such gap over all steps is below NEAR_TIE is compared for its form only.  On the restatement alone the model seeds 0 .. 39
# keep six to eight clips of eight; seed 3 keeps seven, so both kinds of clip occur.
RESTATED = dict(n=5, temperature=0.9, seed=77, min_len=3, no_repeat_ngram=2)
RESTATED_CLIPS, RESTATED_MODEL, NEAR_TIE = 8, 3, 1e-2


@functools.lru_cache(maxsize=None)
def restated(model_seed=RESTATED_MODEL):
    """(ids [B][n][L], phi (B, n), lens [B][n], gap (B,), end, L) of the restated search, computed once and never modified"""
    from test_beam_nbest_host import oracle_stepper
    net, orc, frames, regions = synth_pair(model_seed, RESTATED_CLIPS, end_bias=1.0)
    step_fn, start, state, end, L = oracle_stepper(orc, frames, regions)
    k, B = RESTATED['n'], RESTATED_CLIPS
    R_ = B * k
    last = start.repeat_interleave(k)
    state = {key: v.repeat_interleave(k, 0) for key, v in state.items()}
    lp, G, hist, gap = np.zeros(R_), np.zeros(R_), np.full((R_, L), end, dtype=np.int64), np.full(B, INF)
    for t in range(L):
        logp, state = step_fn(last, state)
        out = gumbel_step(logp.numpy(), last.numpy(), lp, hist, k, end, t, G, RESTATED['temperature'], RESTATED['seed'], SITE_SAMPLE,
                          RESTATED['no_repeat_ngram'], RESTATED['min_len'])
        idx = torch.from_numpy(out['rows'])
        state = {key: v[idx] for key, v in state.items()}
        hist = hist[out['rows']]
        hist[:, t] = out['pred']
        last, lp, G, gap = torch.from_numpy(out['pred']), out['new_lp'], out['G'], np.minimum(gap, out['clip_gap'])
    ids = hist.reshape(B, k, L).tolist()
    lens = [[min(len(words_of(r, end)) + 1, L) for r in clip] for clip in ids]
    return ids, lp.reshape(B, k), lens, gap, end, L


def restated_kept():
    return [b for b in range(RESTATED_CLIPS) if restated()[3][b] >= NEAR_TIE]


def check_against_restated(ids, logp, lens):
    """what both the emulated and the HIP search owe the restatement: kept clips exact (log-probs to 1e-4), every clip well-formed"""
    want_ids, want_lp, want_len, gap, end, L = restated()
    assert ids.shape == (RESTATED_CLIPS, RESTATED['n'], L) and logp.shape == lens.shape == (RESTATED_CLIPS, RESTATED['n'])
    for b in restated_kept():
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b], b
        close(logp[b].numpy(), want_lp[b], 1e-4)
    check_rows(ids, lens, end, RESTATED['no_repeat_ngram'], RESTATED['min_len'])


def test_restated_case_is_decisive():
    ids, lp, lens, gap, end, L = restated()
    print('smallest gaps', ['%.1e' % x for x in gap], 'lengths', sorted({n for clip in lens for n in clip}))
    assert len(restated_kept()) >= RESTATED_CLIPS - 1 and len({n for clip in lens for n in clip}) > 2


def test_host_search_matches_the_restated_search():
    net, orc, frames, regions = synth_pair(RESTATED_MODEL, RESTATED_CLIPS, end_bias=1.0, ops=SbsEmul())
    check_against_restated(*net.sample_without_replacement(frames, regions, **RESTATED))

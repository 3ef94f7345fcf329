"""GPU (-m gpu): the two force launches of a decode under a forced prefix, dlsg_beam_force_prefix and dlsg_sample_force_prefix, called
directly -- behind a real select launch / a real sampled step, against those launches' own bits, `seq_logprob`'s bits and the float64
restatement (tests/emul_prefix.py) -- and `prefix=` through the searches, the samplers, `score`, the four graph classes and
`gather_results` on the small models of tests/test_gpu_rescore.py.  The CPU side is tests/test_prefix_host.py."""
import ctypes as C
import math

import pytest
import torch

import dlsg_amd
from dlsg_amd import engine as E
from dlsg_amd import scoring as S
from dlsg_amd.beam import exclusions_hit, pack_exclusions
from emul_prefix import PrefixEmul, forced_value
from test_ensemble_host import SETTINGS, build_members
from test_rescore_host import ALPHA, K as K3, check_round_trip

gpu = pytest.mark.gpu
INF, NAN = float('inf'), float('nan')
WEIGHTS = {1: [1.0], 3: [0.5, 0.3, 0.2]}
B = 3


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


# ---------------------------------------------------------------------------------------------- the beam launch
def beam_step(V, K, L, M, t, seed, end):
    """the inputs of one history step on B = 3 clips (logit rows V + 3 floats apart, words and histories in [4, V), running
    log-probs in [-8, 0]: one float32 step of a sum below 64 is 3.8e-6, inside the 1e-5 the word values are held to) and fresh
    outputs, on the device"""
    g = torch.Generator().manual_seed(seed)
    R = B * K
    xs = [(torch.randn(R, V + 3, generator=g) * 4.0).cuda()[:, :V] for _ in range(M)]
    c = dict(last=torch.randint(4, V, (R,), generator=g), lp=-8.0 * torch.rand(R, generator=g),
             hist=torch.randint(4, V, (R, L), generator=g))
    c = {key: v.cuda() for key, v in c.items()}
    out = dict(pred=torch.full((R,), -7), nlp=torch.full((R,), 7.0), back=torch.full((R,), -7), rows=torch.full((R,), -7),
               hout=torch.full((R, L), -7))
    out = {key: v.cuda() for key, v in out.items()}
    step = (c['last'], c['lp'], out['pred'], out['nlp'], out['back'], out['rows'], K, end, c['hist'], out['hout'], t)
    return xs, c, out, step


def table(V, L, P, lens, seed):
    """a (B, P) prefix table whose clip b has lens[b] words in [4, V), -1 behind them"""
    px = torch.randint(4, V, (B, P), generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        px[b, n:] = -1
    return px


def select(hip, xs, M, mode, step):
    if M == 1:
        hip.beam_select_hist(xs[0], *step)
    else:
        hip.beam_select_ens(xs, WEIGHTS[M], mode, *step)


@gpu
@pytest.mark.parametrize('L', [5, 64])
@pytest.mark.parametrize('M,mode', [(1, 0), (3, 0), (3, 1)])
@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('V', [50, 65, 1000, 4099])
def test_beam_launch_behind_a_select_launch(hip, V, K, L, M, mode):
    """clips with prefixes of 0, 1 and P = L - 1 words at t = 0, p_b - 1 and p_b.  The sum: new_lp[slot 0] == tok_lp + last_lp with
    torch.equal, tok_lp `seq_logprob`'s for that row and word (at t = 0 new_lp == tok_lp): the float32 sum the kernel stores, which
    a float32 subtraction would not undo; and new_lp - last_lp, in float64, within 1e-5 of the float64 restatement."""
    P, end = L - 1, 2
    plen = [0, 1, P]
    px = table(V, L, P, plen, V + K)
    for t in sorted({0, 1, P - 1, P}):
        xs, c, out, step = beam_step(V, K, L, M, t, 100 * V + 10 * K + t, end)
        select(hip, xs, M, mode, step)
        kept = {key: v.clone() for key, v in out.items()}
        hip.beam_force_prefix(xs, WEIGHTS[M], mode, *step, px.cuda())
        torch.cuda.synchronize()
        emul = {key: v.cpu().clone() for key, v in kept.items()}
        PrefixEmul().beam_force_prefix([x.cpu() for x in xs], WEIGHTS[M], mode, None, c['lp'].cpu(), emul['pred'], emul['nlp'],
                                       emul['back'], emul['rows'], K, end, c['hist'].cpu(), emul['hout'], t, px)
        for b in range(B):
            s = slice(b * K, (b + 1) * K)
            if t >= plen[b]:                                           # the select launch's own bits
                assert all(torch.equal(out[key][s], kept[key][s]) for key in out), (t, b)
                continue
            for key in ('pred', 'back', 'rows', 'hout'):
                assert torch.equal(out[key][s].cpu(), emul[key][s]), (t, b, key)
            assert out['pred'][s].tolist() == [int(px[b, t])] * K and out['rows'][s].tolist() == [b * K] * K
            assert out['nlp'][s][1:].tolist() == [-INF] * (K - 1)
            word = torch.zeros(B * K, 1, dtype=torch.int64, device='cuda')
            word[b * K] = int(px[b, t])
            tok = hip.seq_logprob([x.unsqueeze(0) for x in xs], WEIGHTS[M], mode, word, None, 0.0, True)[3][b * K, 0]
            base = c['lp'][b * K] if t else torch.zeros((), device='cuda')
            assert torch.equal(out['nlp'][b * K], tok + base), (t, b)
            want = forced_value([x.cpu() for x in xs], WEIGHTS[M], mode, b * K, int(px[b, t]))
            assert abs((float(out['nlp'][b * K].double() - base.double())) - want) <= 1e-5, (t, b)


@gpu
@pytest.mark.parametrize('M,mode', [(1, 0), (3, 0), (3, 1)])
@pytest.mark.parametrize('V', [50, 65, 1000, 4099])
def test_forcing_the_word_the_step_chose_leaves_every_buffer(hip, V, M, mode):
    """K = 1: the select launch's word as the prefix's word at t -- pred, new_lp, back, rows and hist_out keep their bits"""
    L = 5
    for t in (0, 2):
        xs, c, out, step = beam_step(V, 1, L, M, t, 7 * V + t, V + 7)
        select(hip, xs, M, mode, step)
        kept = {key: v.clone() for key, v in out.items()}
        px = torch.cat([c['hist'][:, :t], out['pred'].view(B, 1), torch.full((B, L - 2 - t), -1, device='cuda')], 1).contiguous()
        for key in out:
            out[key].fill_(-3)
        hip.beam_force_prefix(xs, WEIGHTS[M], mode, *step, px)
        assert all(torch.equal(out[key], kept[key]) for key in out), t


@gpu
def test_beam_launch_special_values(hip):
    """a -inf forced logit gives the clip -inf, a NaN in the row NaN, as the restatement says"""
    V, K, L, t = 70, 3, 5, 1
    xs, c, out, step = beam_step(V, K, L, 1, t, 5, 2)
    px = table(V, L, 4, [2, 2, 2], 9)
    xs[0][0, int(px[0, t])] = -INF
    xs[0][K, 11] = NAN
    select(hip, xs, 1, 0, step)
    hip.beam_force_prefix(xs, [1.0], 0, *step, px.cuda())
    nlp = out['nlp'].cpu()
    want = [forced_value([xs[0].cpu()], [1.0], 0, b * K, int(px[b, t])) + float(c['lp'][b * K]) for b in range(B)]
    assert want[0] == -INF and math.isnan(want[1]) and math.isfinite(want[2])
    assert float(nlp[0]) == -INF and math.isnan(float(nlp[K])) and abs(float(nlp[2 * K]) - want[2]) <= 1e-5
    assert nlp[1:K].tolist() == [-INF] * (K - 1) and nlp[K + 1:2 * K].tolist() == [-INF] * (K - 1)


@gpu
def test_beam_launch_einval_cases(hip):
    V, K, L, t = 50, 3, 5, 1
    xs, c, out, step = beam_step(V, K, L, 3, t, 3, 2)
    px = table(V, L, 3, [3, 3, 3], 1).cuda()
    kept = {key: v.clone() for key, v in out.items()}

    def call(K=K, L=L, t=t, P=3, M=3, mode=0, table=px, clips=B, hist_out=out['hout']):
        R, _, members = hip._beam_members(xs[:max(1, min(M, 3))], WEIGHTS[3][:max(1, min(M, 3))], px.device)
        a = hip._beam_args(B * 3, V, *step[:6], 3, 2, t == 0, None)
        a.k, a.B = K, clips
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())       # noqa: E731
        return hip.lib.dlsg_beam_force_prefix(C.byref(a), *members[:4], M, mode, ptr(c['hist']), ptr(hist_out), L, t, ptr(table), P,
                                              hip._stream())
    EINVAL = dlsg_amd.abi.defines['DLSG_EINVAL']
    from dlsg_amd.hip import ENS_MAX
    for bad in (dict(K=0), dict(K=9), dict(L=0), dict(L=65), dict(t=-1), dict(t=L), dict(P=L), dict(P=-1), dict(M=0), dict(M=ENS_MAX + 1),
                dict(mode=2), dict(mode=-1), dict(table=None), dict(hist_out=None)):
        assert call(**bad) == EINVAL, bad
    assert call(P=0) == 0 and call(P=0, table=None) == 0 and call(clips=0) == 0 and call(t=3) == 0        # nothing to force
    torch.cuda.synchronize()
    assert all(torch.equal(out[key], kept[key]) for key in out)        # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(out['pred'], kept['pred'])
    with pytest.raises(ValueError, match='holds 2 clips, the step 3'):
        hip.beam_force_prefix(xs, WEIGHTS[3], 0, *step, px[:2].contiguous())
    with pytest.raises(ValueError, match='contiguous int64 tensor'):
        hip.beam_force_prefix(xs, WEIGHTS[3], 0, *step, px.int())
    with pytest.raises(ValueError, match='contiguous int64 tensor'):
        hip.beam_force_prefix(xs, WEIGHTS[3], 0, *step, px.t().contiguous().t())
    with pytest.raises(ValueError, match='the prefix on cpu'):
        hip.beam_force_prefix(xs, WEIGHTS[3], 0, *step, px.cpu())


# ---------------------------------------------------------------------------------------------- the sampler launch
def sampled_step(V, rows, seed, W=20):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, V + 3, generator=g) * 3.0).cuda()[:, :V]
    emb = torch.randn(V, W, generator=g).cuda()
    return x, emb


def sample_outputs(rows, L, W=20):
    return dict(ids=torch.full((rows,), -7, device='cuda'), out=torch.full((rows, W), 7.0, device='cuda'),
                logp=torch.full((rows,), 7.0, device='cuda'), lens=torch.full((rows,), L, device='cuda'))


@gpu
@pytest.mark.parametrize('seed_word', [False, True])
@pytest.mark.parametrize('tau', [0.0, 0.7])
@pytest.mark.parametrize('V', [50, 65, 1000, 4099])
def test_forcing_the_word_sample_embed_drew_leaves_its_bits(hip, V, tau, seed_word):
    rows, L, t, p = 7, 5, 2, 0.3
    x, emb = sampled_step(V, rows, V + 1)
    seed = torch.tensor([0x5B5], dtype=torch.int64, device='cuda') if seed_word else 0x5B5
    kw = dict(temperature=tau, p=p, seed=seed, site=E.SITE_WORD, row0=(t + 1) * rows)
    o = sample_outputs(rows, L)
    hip.sample_embed(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, V + 7, site_sample=E.SITE_SAMPLE, **kw)
    kept = {key: v.clone() for key, v in o.items()}
    assert bool((kept['out'] == 0).any()) and bool((kept['lens'] == L).all())          # the dropout bites; no row ended
    px = torch.cat([torch.full((rows, t), 4, device='cuda'), kept['ids'].view(rows, 1), torch.full((rows, 1), -1, device='cuda')], 1)
    px[3, 0] = -1                                                      # row 3 is free: it keeps whatever stands there
    for key in o:
        o[key].fill_(-3)
    flags = torch.full((rows,), 7, dtype=torch.int32, device='cuda')
    hip.sample_force_prefix(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, px.contiguous(), L, kept=flags, **kw)
    forced = torch.tensor([r != 3 for r in range(rows)], device='cuda')
    for key in o:
        assert torch.equal(o[key][forced], kept[key][forced]), key
        assert bool((o[key][3] == -3).all()), key
    assert flags.tolist() == [1, 1, 1, 7, 1, 1, 1]


@gpu
@pytest.mark.parametrize('tau', [0.0, 0.7])
@pytest.mark.parametrize('V', [50, 4099])
def test_sampler_launch_against_the_restatement(hip, V, tau):
    """two rows per clip, prefixes of 0, 1 and L - 1 words, at t = 0, p_b - 1 and p_b, behind a real sampled step: free rows keep
    its bits; forced rows get the clip's word, its log-probability within 1e-5 of log_softmax in float64, `embed_fwd`'s row,
    lens = L -- also where the step drew <end> -- and kept = 1"""
    n, L, p, seed = 2, 5, 0.3, 77
    rows, P = B * n, L - 1
    plen = [0, 1, P]
    px = table(V, L, P, plen, V + 2)
    for t in sorted({0, 1, P - 1, P}):
        x, emb = sampled_step(V, rows, 10 * V + t)
        o = sample_outputs(rows, L)
        kw = dict(temperature=tau, p=p, seed=seed, site=E.SITE_WORD, row0=(t + 1) * rows)
        hip.sample_embed(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, 2, site_sample=E.SITE_SAMPLE, **kw)
        end = int(o['ids'][rows - 1])                                  # once more, with the last row's word as <end>: it ends there
        o = sample_outputs(rows, L)
        hip.sample_embed(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, end, site_sample=E.SITE_SAMPLE, **kw)
        assert int(o['lens'][rows - 1]) == t + 1
        kept = {key: v.clone() for key, v in o.items()}
        flags = torch.full((rows,), 7, dtype=torch.int32, device='cuda')
        hip.sample_force_prefix(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, px.cuda(), L, rows_per_clip=n, kept=flags, **kw)
        lp = torch.log_softmax(x.cpu().double() / tau if tau > 0 else x.cpu().double(), 1)
        want_out = torch.empty_like(o['out'])
        words = torch.tensor([int(px[r // n, min(t, P - 1)]) if t < plen[r // n] else 4 for r in range(rows)], device='cuda')
        hip.embed_fwd(emb, words, want_out, p=p, seed=seed, site=E.SITE_WORD, row0=(t + 1) * rows)
        for r in range(rows):
            if t >= plen[r // n]:
                assert all(torch.equal(o[key][r], kept[key][r]) for key in o) and int(flags[r]) == 7, (t, r)
                continue
            w = int(px[r // n, t])
            assert int(o['ids'][r]) == w and int(o['lens'][r]) == L and int(flags[r]) == 1, (t, r)
            assert abs(float(o['logp'][r]) - float(lp[r, w])) <= 1e-5, (t, r)
            assert torch.equal(o['out'][r], want_out[r]), (t, r)


@gpu
def test_sampler_launch_special_values_and_einval(hip):
    V, rows, L, t = 70, 4, 5, 0
    x, emb = sampled_step(V, rows, 3)
    px = torch.tensor([[9], [10], [11], [-1]], device='cuda')
    x[0, 9] = -INF
    x[1, 10] = NAN
    o = sample_outputs(rows, L)
    hip.sample_embed(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, 2, temperature=1.0, seed=5, site_sample=E.SITE_SAMPLE)
    kept = {key: v.clone() for key, v in o.items()}
    hip.sample_force_prefix(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, px, L, temperature=1.0, seed=5)
    lp = torch.log_softmax(x[:, :].cpu().double(), 1)
    assert float(o['logp'][0]) == -INF and float(lp[0, 9]) == -INF and math.isnan(float(o['logp'][1])) and math.isnan(float(lp[1, 10]))
    assert abs(float(o['logp'][2]) - float(lp[2, 11])) <= 1e-5 and o['ids'].tolist()[:3] == [9, 10, 11]
    assert all(torch.equal(o[key][3], kept[key][3]) for key in o)

    def call(V=V, W=20, tau=1.0, L=L, t=t, P=1, table=px, rows=rows, rpc=1):
        ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())       # noqa: E731
        return hip.lib.dlsg_sample_force_prefix(ptr(x), C.c_int64(x.stride(0)), V, C.c_float(tau), ptr(emb), ptr(o['ids']), ptr(o['out']),
                                                C.c_int64(20), W, ptr(o['logp']), ptr(o['lens']), t, rows, C.c_float(0.0), C.c_uint64(5),
                                                C.c_uint32(0), C.c_int64(0), None, ptr(table), P, rpc, L, None, hip._stream())
    for key in o:
        o[key].fill_(-3)
    EINVAL = dlsg_amd.abi.defines['DLSG_EINVAL']
    for bad in (dict(V=0), dict(W=-1), dict(tau=-1.0), dict(L=0), dict(t=-1), dict(t=L), dict(P=L), dict(P=-1), dict(table=None),
                dict(rpc=0), dict(rpc=3)):
        assert call(**bad) == EINVAL, bad
    assert call(P=0) == 0 and call(rows=0) == 0 and call(t=1) == 0
    torch.cuda.synchronize()
    assert all(bool((o[key] == -3).all()) for key in o)                # nothing was launched
    assert call() == 0 and o['ids'].tolist() == [9, 10, 11, -3]
    with pytest.raises(ValueError, match='holds 4 clips, the step 2'):
        hip.sample_force_prefix(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, px, L, rows_per_clip=2)
    with pytest.raises(ValueError, match='rows_per_clip = 3'):
        hip.sample_force_prefix(x, emb, o['ids'], o['out'], o['logp'], o['lens'], t, px, L, rows_per_clip=3)


# ---------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope='module')
def members():
    nets, frames, regions = build_members()
    return [n.cuda() for n in nets], frames.cuda(), regions.cuda()


def prefix_of(rows, plen):
    """(B, max plen) int64: clip b's first plen[b] words of rows[b] (a row of ids), -1 behind them"""
    px = torch.full((rows.shape[0], max(plen)), -1, dtype=torch.int64, device=rows.device)
    for b, n in enumerate(plen):
        px[b, :n] = rows[b, :n]
    return px


PLEN = [0, 1, 2, 3, 0, 4, 2, 1]
OPTS = dict(beam_size=K3, length_penalty=ALPHA, no_repeat_ngram=2, min_len=5)


@gpu
@pytest.mark.parametrize('setting', [None] + list(SETTINGS))
def test_prefixed_search_and_round_trip(members, setting):
    """a model and the three-member ensemble: the prefix is each clip's last beam's beginning (words a beam chose, so `check_round_trip`'s
    rank rule holds for them too); every row begins with it, the clips without one keep their bits, `score` returns the scores"""
    nets, frames, regions = members
    scorer = nets[0] if setting is None else dlsg_amd.Ensemble(nets, SETTINGS[setting], setting)
    plain = scorer.beam_search(frames, regions, **OPTS)
    px = prefix_of(plain[0][:, -1], PLEN)
    got = scorer.beam_search(frames, regions, prefix=px, **OPTS)
    L = got[0].shape[2]
    for b, n in enumerate(PLEN):
        assert torch.equal(got[0][b, :, :n], px[b, :n].expand(K3, n)), b
        if n == 0:
            assert all(torch.equal(a[b], c[b]) for a, c in zip(got, plain)), b
    assert not torch.equal(got[0], plain[0]) and bool(torch.isfinite(got[1]).all()) and bool((got[2] > 5).all())
    score = scorer.score(frames, regions, got[0], length_penalty=ALPHA, return_tokens=True, return_ranks=True)
    check_round_trip([x.cpu() for x in got], [x.cpu() for x in score])
    assert got[0].shape == (len(PLEN), K3, L)


@gpu
def test_forcing_what_beam_one_chose_changes_nothing(members):
    nets, frames, regions = members
    L = nets[0].decoder.max_words
    opts = dict(beam_size=1, length_penalty=ALPHA, min_len=L - 1)
    want = nets[0].beam_search(frames, regions, **opts)
    px = prefix_of(want[0][:, 0], [(1, 3, L - 1)[b % 3] for b in range(frames.shape[0])])
    assert not bool((px == nets[0].decoder.vocab('<end>')).any())
    got = nets[0].beam_search(frames, regions, prefix=px, **opts)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    ens = dlsg_amd.Ensemble(nets, SETTINGS['logprob'], 'logprob')
    want = ens.beam_search(frames, regions, **opts)
    got = ens.beam_search(frames, regions, prefix=prefix_of(want[0][:, 0], [(1, 3, L - 1)[b % 3] for b in range(frames.shape[0])]), **opts)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@gpu
def test_forcing_what_the_samplers_drew(members):
    nets, frames, regions = members
    net = nets[0]
    for kw, exact in ((dict(), True), (dict(top_k=5, no_repeat_ngram=2), False)):
        ids, logp, lens = net.sample(frames, regions, n=1, temperature=0.8, seed=11, **kw)
        plen = [min(p, int(l) - 1) for p, l in zip(PLEN, lens.tolist())]
        px = prefix_of(ids, plen)
        got = net.sample(frames, regions, n=1, temperature=0.8, seed=11, prefix=px, **kw)
        assert torch.equal(got[0], ids) and torch.equal(got[2], lens) and max(plen) >= 1
        for b, n in enumerate(plen):
            assert torch.equal(got[1][b, n:], logp[b, n:]), b
            if exact:
                assert torch.equal(got[1][b], logp[b]), b
    # two rows per clip, a table for the clips: both rows begin with it, the filtered sampler reports kept = 1 there
    px = prefix_of(ids, plen)
    for share in (False, True):
        ids2, logp2, lens2, kept2 = net.sample(frames, regions, n=2, temperature=0.8, seed=11, top_k=5, return_kept=True, prefix=px,
                                               share_encoder=share)
        for b, n in enumerate(plen):
            assert torch.equal(ids2[2 * b:2 * b + 2, :n], px[b, :n].expand(2, n)) and bool((kept2[2 * b:2 * b + 2, :n] == 1).all())
            assert bool((lens2[2 * b:2 * b + 2] > n).all())


@gpu
def test_exclusions_and_constraints_see_the_prefix(members):
    nets, frames, regions = members
    net = nets[0]
    vocab = net.decoder.vocab
    plain = net.beam_search(frames, regions, **OPTS)
    px = prefix_of(plain[0][:, -1], PLEN)
    px = torch.where((px >= 0) & (px < 4), torch.full_like(px, 17), px)          # (no <pad>, <start>, <unk>: they go into tables below)
    inside = set(px[px >= 0].tolist())
    best = [w for w in plain[0][:, 0].flatten().tolist() if w >= 4 and w not in inside]
    words = sorted(set(best), key=lambda w: -best.count(w))[:2]
    # entries that cross the boundary: (a clip's last prefix word, the word the prefixed search puts behind it)
    free = net.beam_search(frames, regions, prefix=px, **OPTS)[0]
    pairs = [[(int(px[b, n - 1]), int(free[b, 0, n]))] if n and int(free[b, 0, n]) >= 4 else [] for b, n in enumerate(PLEN)]
    ex = pack_exclusions(vocab, words=words, per_clip=pairs, device='cuda')
    ids, scores, lens = net.beam_search(frames, regions, prefix=px, exclude=ex, **OPTS)
    assert sum(bool(p) for p in pairs) >= 1 and not torch.equal(ids, free)
    assert int(exclusions_hit(ids, lens, ex)[scores > -INF].sum()) == 0 and bool(torch.isfinite(scores[:, 0]).all())
    for b, n in enumerate(PLEN):
        assert torch.equal(ids[b, :, :n], px[b, :n].expand(K3, n))
    # a constraint a prefix word meets is counted; one the search has to meet itself is met behind the prefix
    other = [w for w in range(4, 50) if w not in inside][:len(PLEN)]
    cons = [[[int(px[b, 0])], [other[b]]] if n else [[other[b]]] for b, n in enumerate(PLEN)]
    ids, scores, lens, met = net.constrained_beam_search(frames, regions, cons, prefix=px, return_met=True, **OPTS)
    assert met[:, 0].tolist() == [2 if n else 1 for n in PLEN]
    for b, n in enumerate(PLEN):
        assert torch.equal(ids[b, :, :n], px[b, :n].expand(K3, n)) and other[b] in ids[b, 0, n:].tolist()


@gpu
def test_the_graphs_replay_to_the_eager_bits(members):
    nets, frames, regions = members
    net = nets[0]
    ens = dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob')
    plain = net.beam_search(frames, regions, **OPTS)
    px = prefix_of(plain[0][:, -1], PLEN)
    new = prefix_of(plain[0][:, 1].flip(0), PLEN)
    assert new.shape == px.shape and not torch.equal(new, px)
    cons = [[[7]], [], [[8, 9]], [], [], [[10]], [], []]
    f2, r2 = frames.flip(0).contiguous() * 0.5, regions.flip(0).contiguous()
    cases = [(dlsg_amd.NBestBeamGraph(net, frames, regions, prefix=px, **OPTS), lambda f, r, p: net.beam_search(f, r, prefix=p, **OPTS), ()),
             (dlsg_amd.EnsembleBeamGraph(ens, frames, regions, prefix=px, **OPTS), lambda f, r, p: ens.beam_search(f, r, prefix=p, **OPTS), ()),
             (dlsg_amd.ConstrainedBeamGraph(net, frames, regions, cons, prefix=px, **OPTS),
              lambda f, r, p: net.constrained_beam_search(f, r, cons, prefix=p, **OPTS), (cons,)),
             (dlsg_amd.SampleGraph(net, frames, regions, n=2, temperature=0.8, top_k=5, prefix=px),
              lambda f, r, p: net.sample(f, r, 2, 0.8, 21, top_k=5, prefix=p), (21,))]
    for graph, eager, extra in cases:
        assert torch.equal(graph.prefix, px) and graph.prefix.data_ptr() != px.data_ptr()
        for f, r in ((f2, r2), (frames, regions)):
            got = [x.clone() for x in graph(f, r, *extra)]
            assert all(torch.equal(a, b) for a, b in zip(got, eager(f, r, px))), type(graph).__name__
        graph.prefix.copy_(new)
        got = [x.clone() for x in graph(frames, regions, *extra)]
        assert all(torch.equal(a, b) for a, b in zip(got, eager(frames, regions, new))), type(graph).__name__
        assert not torch.equal(got[0], eager(frames, regions, px)[0])


@gpu
def test_gather_results_decodes_with_the_prefix(members):
    nets, frames, regions = members
    net = nets[0]
    vids = ['v%d' % i for i in range(frames.shape[0])]
    px = prefix_of(net.beam_search(frames, regions, **OPTS)[0][:, -1], PLEN).cpu()
    table = dict(zip(vids, px.tolist()))
    fn = lambda ids: torch.tensor([table[v] for v in ids])               # noqa: E731
    got = S.gather_results(net, [(frames, regions, None, vids)], decode=dict(prefix=fn, **OPTS))
    ids = net.beam_search(frames, regions, prefix=px.cuda(), n_best=1, **OPTS)[0][:, 0].cpu()
    assert got == {v: net.decoder.decode_tokens(ids[i]) for i, v in enumerate(vids)}
    assert all(ids[b, :n].tolist() == px[b, :n].tolist() for b, n in enumerate(PLEN))

"""GPU: `dlsg_sample_ens` on the MI355X -- the combined row it leaves in `comb` against `emul_ensemble.combined_logp` (float64), its
draw against the existing sampled steps run on `comb` as their logits (equal bits), edge rows, the distribution drawn from, the
refusals, and `Ensemble.sample` / `EnsembleSampleGraph` on small synthetic members.  The CPU side is tests/test_ens_sample_host.py."""
import ctypes as C
import functools
import math

import pytest
import torch

import dlsg_amd
from dlsg_amd import engine as E
from dlsg_amd.hip import ENS_MAX, SAMPLE_FILTER_MAXV
from emul_ensemble import combined_logp
from emul_sample import kept_sets, tempered
from test_ensemble_host import build_members
from test_gpu_sample_filter import CASES

gpu = pytest.mark.gpu
DEV = 'cuda'
ROWS = 64
INF, NAN = float('inf'), float('nan')
TOL = 1e-5          # tests/test_gpu_rescore.py and tests/test_gpu_ensemble.py hold a combined value to this against float64
ENSEMBLES = {1: [1.0], 2: [0.7, 0.3], 3: [0.5, 0.3, 0.2], 8: [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]}
FILTERS = sorted({(k, p) for _, k, p in CASES}) + [(0, 1.0)]           # the (top_k, top_p) of the filtered sampler's cases, and off


@pytest.fixture(scope='module')
def ops():
    from dlsg_amd.hip import HipOps
    return HipOps()


@functools.lru_cache(maxsize=None)
def member_rows(V, M, rows=ROWS):
    """M members' logits (rows, V) on the host, each a view into a wider array of its own width (rows padded by 0, 3, 6, ... floats):
    read-only"""
    g = torch.Generator().manual_seed(7 * V + M)
    return tuple((torch.randn(rows, V + 3 * m, generator=g) * 3)[:, :V] for m in range(M))


def on_device(xs):
    """the members on the device with their paddings kept"""
    out = []
    for x in xs:
        wide = torch.empty(x.shape[0], x.stride(0), device=DEV)
        wide[:, :x.shape[1]] = x.to(DEV)
        out.append(wide[:, :x.shape[1]])
    return out


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def run_ens(ops, xs, weights, mode, t=0, end=-1, tau=1.0, seed=99, row0=128, hist=None, lens=None, **opts):
    rows, V = xs[0].shape
    comb = torch.full((rows, V), -3.0, device=DEV)
    ids = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    logp = torch.full((rows,), 7.0, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lens = torch.full((rows,), 26, dtype=torch.int64, device=DEV) if lens is None else lens.clone()
    ops.sample_ens(xs, weights, mode, comb, ids, logp, lens, t, end, temperature=tau, seed=seed, site_sample=E.SITE_SAMPLE, row0=row0,
                   hist=hist, kept=kept, **opts)
    return comb, ids, logp, lens, kept


def run_parent(ops, comb, t=0, end=-1, tau=1.0, seed=99, row0=128, hist=None, lens=None, top_k=0, top_p=1.0, min_len=0,
               no_repeat_ngram=0, excl_shared=None, excl_clip=None, rows_per_clip=1):
    """the existing step the controls select, on `comb` as its logits -> ids, logp, lens, kept (the plain step counts nothing: the
    number of words above -inf, which is what the filtered step reports with every control off)"""
    rows, V = comb.shape
    Emb = torch.zeros(V, 4, device=DEV)
    ids = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    out = torch.empty(rows, 4, device=DEV)
    logp = torch.full((rows,), 7.0, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lens = torch.full((rows,), 26, dtype=torch.int64, device=DEV) if lens is None else lens.clone()
    common = dict(temperature=tau, p=0.0, seed=seed, site=E.SITE_WORD, site_sample=E.SITE_SAMPLE, row0=row0)
    controls = dict(top_k=top_k, top_p=top_p, min_len=min_len, no_repeat_ngram=no_repeat_ngram, hist=hist, kept=kept)
    if excl_shared is not None or excl_clip is not None:
        ops.sample_excl_embed(comb, Emb, ids, out, logp, lens, t, end, excl_shared=excl_shared, excl_clip=excl_clip,
                              rows_per_clip=rows_per_clip, **common, **controls)
    elif top_k > 0 or top_p < 1.0 or min_len > 0 or no_repeat_ngram > 0:
        ops.sample_filter_embed(comb, Emb, ids, out, logp, lens, t, end, **common, **controls)
    else:
        ops.sample_embed(comb, Emb, ids, out, logp, lens, t, end, **common)
        kept = (comb > -INF).sum(1).int()
    return ids, logp, lens, kept


def check_draw(ops, xs, weights, mode, **kw):
    """one launch against the existing step on its comb: equal bits in ids, logp, lens and kept, every row -> (comb, ids, logp, lens, kept)"""
    got = run_ens(ops, xs, weights, mode, **kw)
    want = run_parent(ops, got[0], **kw)
    torch.cuda.synchronize()
    for name, a, b in zip(('ids', 'logp', 'lens', 'kept'), got[1:], want):
        assert torch.equal(bits(a), bits(b)), (name, kw, (bits(a) != bits(b)).nonzero().flatten()[:8].tolist())
    return got


def histories(t, rows, V, seed):
    """(t, rows) words in 4 .. 11: short alphabets repeat, so the n-gram ban and multi-word entries do match"""
    return torch.randint(4, 12, (t, rows), generator=torch.Generator().manual_seed(seed)).to(DEV)


# ---------------------------------------------------------------------------------------------- 1, 2: the combined row, the draw
@gpu
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('M', sorted(ENSEMBLES))
@pytest.mark.parametrize('V', [1000, 10000])
def test_comb_is_the_combined_row_and_the_draw_is_the_parents(ops, V, M, mode):
    host = member_rows(V, M)
    xs, weights = on_device(host), ENSEMBLES[M]
    assert len({x.stride(0) for x in xs}) == M
    want = combined_logp(host, weights, mode)
    comb, ids, logp, lens, kept = check_draw(ops, xs, weights, mode)
    again = run_ens(ops, xs, weights, mode)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((comb, ids, logp, lens, kept), again))      # two launches: equal bits
    err = float((comb.cpu().double() - want).abs().max())
    print('V %d M %d mode %d: max |comb - float64| %.3g' % (V, M, mode, err))
    assert err <= TOL
    assert int(ids.min()) >= 0 and bool((kept == V).all()) and bool((logp <= 0).all())
    end = int(ids[0])
    for tau in (1.0, 0.7, 0.0):
        for top_k, top_p in FILTERS:
            got = check_draw(ops, xs, weights, mode, tau=tau, top_k=top_k, top_p=top_p, t=2, end=end, seed=31 + top_k, row0=192)
            assert torch.equal(got[0], comb)
            if tau > 0 and top_k:
                assert 1 <= int(got[4].min()) and int(got[4].max()) <= top_k
        # one n-gram ban, one minimum length, one exclusion table of each kind
        hist = histories(5, ROWS, V, V + M)
        banned = check_draw(ops, xs, weights, mode, tau=tau, t=5, hist=hist, no_repeat_ngram=2, top_p=0.9)
        assert int(check_draw(ops, xs, weights, mode, tau=tau, t=5, hist=hist, no_repeat_ngram=1)[4].max()) < V
        early = check_draw(ops, xs, weights, mode, tau=tau, t=1, end=end, min_len=3, top_k=50)
        assert bool((early[1] != end).all()) and bool((early[3] == 26).all())
        shared = torch.tensor([[5, 6, -1], [end, -1, -1], [9, 4, 7]], dtype=torch.int64, device=DEV)
        clip = torch.full((ROWS // 4, 2, 3), -1, dtype=torch.int64)
        clip[:, 0, 0] = torch.arange(ROWS // 4) + 20
        clip[::2, 1, :2] = torch.tensor([8, 10])
        clip = clip.to(DEV)
        under = check_draw(ops, xs, weights, mode, tau=tau, t=5, end=end, hist=hist, excl_shared=shared, top_k=50, top_p=0.9)
        assert bool((under[1] != end).all())
        own = check_draw(ops, xs, weights, mode, tau=tau, t=5, hist=hist, excl_clip=clip, rows_per_clip=4, no_repeat_ngram=3)
        assert bool((own[1] != (torch.arange(ROWS, device=DEV) // 4 + 20)).all()) and int(own[4].max()) < V
        both = check_draw(ops, xs, weights, mode, tau=tau, t=5, end=end, hist=hist, excl_shared=shared, excl_clip=clip, rows_per_clip=4)
        assert int(both[4].max()) <= V - 1
    assert banned is not None


# ---------------------------------------------------------------------------------------------- 3: edge rows
@gpu
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('M', [1, 3])
def test_edge_rows(ops, M, mode):
    """member M - 1: row 3 all NaN, row 4 all -inf, row 7 partly NaN.  comb follows dlsg_seq_logprob's rule for a member row without
    a log-sum-exp, and the draw is still the existing step's on comb.  Second pass, `alone`: class 5 of rows 3 and 4 is -inf in every
    other member, where mode 0 owes -inf, not NaN.  That pass leaves out the set with every control off: such a row holds -inf and
    NaN only, dlsg_sample_embed's tie rule names its first -inf word (5) where the filtered steps, and this one, name word 0."""
    V = 1000
    weights = ENSEMBLES[M]
    sets = ((1.0, dict()), (0.7, dict(top_k=50, top_p=0.9)), (0.0, dict(top_k=3)), (1.0, dict(min_len=2, t=1, end=17)))
    good = torch.ones(ROWS, dtype=torch.bool)
    good[[3, 4, 7]] = False
    for alone in (False, True):
        host = [x.clone() for x in member_rows(V, M)]
        bad = host[M - 1]
        bad[3] = NAN
        bad[4] = -INF
        bad[7, ::7] = NAN
        if alone:
            for x in host[:M - 1]:
                x[3, 5] = x[4, 5] = -INF
        xs = on_device(host)
        want = combined_logp(host, weights, mode)
        for tau, opts in sets[1:] if alone else sets:
            comb, ids, logp, lens, kept = check_draw(ops, xs, weights, mode, tau=tau, **opts)
            c = comb.cpu()
            for r in (3, 4, 7):
                nan = torch.ones(V, dtype=torch.bool)
                if alone and M > 1 and mode == 0 and r != 7:           # the maximum over the members skips the NaN
                    assert bool(c[r, 5] == -INF), r
                    nan[5] = False
                assert bool(c[r][nan].isnan().all()), r
                assert int(ids[r]) == 0 and int(kept[r]) == 0
            assert float((c[good].double() - want[good]).abs().max()) <= TOL and bool((kept.cpu()[good] >= 1).all())
    # one word left: the maximum of c, with probability 1
    good = good.to(DEV)
    for tau, opts in ((1.0, dict(top_k=1)), (0.7, dict(top_p=1e-6))):
        comb, ids, logp, lens, kept = check_draw(ops, xs, weights, mode, tau=tau, seed=3, **opts)
        assert torch.equal(ids[good], comb[good].argmax(1)) and bool((logp[good] == 0).all()) and bool((kept[good] == 1).all())
        assert bool((kept[~good] == 0).all())


@gpu
def test_vocabulary_bound(ops):
    """the threshold searches hold a row in LDS: V = 32768 runs under a control, one more is refused without a launch -- by the
    binding and by the entry point -- and runs with every control off"""
    V = SAMPLE_FILTER_MAXV
    assert V == 32768
    host = member_rows(V + 1, 2)
    xs = on_device([x[:, :V] for x in host])
    got = check_draw(ops, xs, ENSEMBLES[2], 0, tau=0.7, top_k=50, top_p=0.9)
    assert 1 <= int(got[4].min()) and int(got[4].max()) <= 50
    err = float((got[0].cpu().double() - combined_logp([x[:, :V] for x in host], ENSEMBLES[2], 0)).abs().max())
    print('V %d: max |comb - float64| %.3g' % (V, err))
    assert err <= TOL
    wide = on_device(host)
    for opts in (dict(top_k=50), dict(top_p=0.9), dict(min_len=1), dict(no_repeat_ngram=2),
                 dict(excl_shared=torch.tensor([[5]], dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError, match='vocabulary %d > %d' % (V + 1, V)):
            run_ens(ops, wide, ENSEMBLES[2], 0, **opts)
    got = check_draw(ops, wide, ENSEMBLES[2], 1, tau=0.7)              # every control off: no row is held
    assert bool((got[4] == V + 1).all())


@gpu
def test_einval_cases(ops):
    """the entry point itself: EINVAL and no launch"""
    rows, V = 4, 10
    x = torch.randn(rows, V, device=DEV)
    comb = torch.zeros(rows, V, device=DEV)
    ids = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    logp = torch.zeros(rows, device=DEV)
    lens = torch.full((rows,), 26, dtype=torch.int64, device=DEV)
    hist = torch.zeros(64, rows, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(M=1, mode=0, V=V, tau=1.0, t=0, top_k=0, top_p=1.0, min_len=0, g=0, rows=rows, rpc=1, h=hist):
        n = max(M, 1)
        return ops.lib.dlsg_sample_ens((C.c_void_p * n)(*[x.data_ptr()] * n), (C.c_int64 * n)(*[10] * n), (C.c_float * n)(*[1.0 / n] * n),
                                       (C.c_float * n)(*[math.log(1.0 / n)] * n), M, mode, V, C.c_float(tau), p(comb), p(ids), p(logp),
                                       p(lens), t, C.c_int64(3), rows, C.c_uint64(5), C.c_uint32(E.SITE_SAMPLE), C.c_int64(0), None,
                                       top_k, C.c_float(top_p), min_len, g, None if h is None else p(h), C.c_int64(rows), None, None, 0,
                                       None, 0, 1, rpc, ops._stream())
    EINVAL = dlsg_amd.abi.defines['DLSG_EINVAL']
    for bad in (dict(M=0), dict(M=ENS_MAX + 1), dict(mode=2), dict(mode=-1), dict(V=0), dict(tau=-1.0), dict(t=64), dict(t=-1),
                dict(V=SAMPLE_FILTER_MAXV + 1, top_k=3), dict(V=SAMPLE_FILTER_MAXV + 1, min_len=1), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(min_len=-1), dict(g=-1), dict(rpc=0), dict(rpc=3), dict(g=2, t=3, h=None)):
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((comb == 0).all())           # nothing was launched
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert bool((ids == -7).all())
    assert call() == 0 and call(M=ENS_MAX, mode=1, t=63, g=2, top_k=3) == 0
    torch.cuda.synchronize()
    assert bool((ids >= 0).all()) and bool((comb < 0).all())
    with pytest.raises(ValueError):
        run_ens(ops, [x], [0.0], 0)


# ---------------------------------------------------------------------------------------------- 4: the distribution
DIST = {0: dict(tau=0.7, top_p=0.9), 1: dict(tau=1.3, top_k=10)}
DIST_V, DIST_ROWS = 37, 1 << 17


@functools.lru_cache(maxsize=None)
def dist_case(mode):
    """three members' rows of 37 logits, the float64 truncated and renormalised exp(c / tau) of the setting, and its kept set"""
    g = torch.Generator().manual_seed(50 + mode)
    rows = [torch.randn(1, DIST_V, generator=g) * 1.5 for _ in range(3)]
    rows[1][0, 11] = -INF
    c = combined_logp(rows, ENSEMBLES[3], mode)
    opts = DIST[mode]
    keep, _, amb = kept_sets(tempered(c.float(), opts['tau']), opts.get('top_k', 0), opts.get('top_p', 1.0))
    zk = torch.where(torch.from_numpy(keep[0]), c[0] / opts['tau'], torch.full((DIST_V,), -INF, dtype=torch.float64))
    return rows, torch.softmax(zk, 0).numpy(), keep[0], bool(amb[0])


@pytest.mark.parametrize('mode', [0, 1])
def test_the_distribution_case_has_counts_to_test(mode):
    """on the CPU: the setting truncates, float32 can decide its boundary, and every expected count is at least 5"""
    rows, p, keep, amb = dist_case(mode)
    print('mode %d: %d words kept, smallest expected count %.1f' % (mode, int(keep.sum()), DIST_ROWS * p[keep].min()))
    assert 2 <= int(keep.sum()) < DIST_V - 1 and not amb
    assert DIST_ROWS * p[keep].min() >= 5 and abs(p.sum() - 1) < 1e-12


@gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_sampled_words_follow_the_truncated_ensemble_distribution(ops, mode):
    from scipy.stats import chi2
    rows, p, keep, _ = dist_case(mode)
    xs = [r.to(DEV).expand(DIST_ROWS, DIST_V).contiguous() for r in rows]
    opts = DIST[mode]
    comb, ids, logp, lens, kept = run_ens(ops, xs, ENSEMBLES[3], mode, t=3, seed=1234, row0=DIST_ROWS, **opts)
    torch.cuda.synchronize()
    cnt = torch.bincount(ids.cpu(), minlength=DIST_V).double().numpy()
    assert (cnt[~keep] == 0).all() and bool((kept == int(keep.sum())).all())
    stat = float((((cnt - DIST_ROWS * p) ** 2)[keep] / (DIST_ROWS * p[keep])).sum())
    print('mode %d: chi-square %.1f on %d degrees of freedom' % (mode, stat, int(keep.sum()) - 1))
    assert stat < chi2.ppf(1 - 1e-6, int(keep.sum()) - 1), stat
    want = torch.log(torch.from_numpy(p)).to(DEV)
    assert float((logp.double() - want[ids]).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------- 5: model level
B, N = 4, 3


@pytest.fixture(scope='module')
def members():
    nets, frames, regions = build_members()
    return [n.cuda() for n in nets], frames[:B].cuda(), regions[:B].cuda()


@gpu
@pytest.mark.parametrize('setting', ['prob', 'logprob'])
def test_temperature_zero_is_greedy_and_logp_is_the_score(members, setting):
    nets, frames, regions = members
    ens = dlsg_amd.Ensemble(nets, [0.5, 0.3, 0.2], setting)
    L = ens.decoder.max_words
    cold = [x.cpu() for x in ens.sample(frames, regions, n=1, temperature=0.0)]
    greedy = ens.greedy(frames, regions).cpu()
    for b in range(B):
        n = int(cold[2][b])
        assert cold[0][b, :n].tolist() == greedy[b, :n].tolist(), b
    ids, logp, lens = ens.sample(frames, regions, n=N, seed=21)
    again = ens.sample(frames, regions, n=N, seed=21)
    other = ens.sample(frames, regions, n=N, seed=22)
    assert all(torch.equal(a, b) for a, b in zip(again, (ids, logp, lens))) and not torch.equal(other[0], ids)      # two eager calls
    assert ids.shape == (B * N, L) and logp.shape == (B * N, L) and lens.shape == (B * N,)
    assert any(not torch.equal(ids[b * N], ids[b * N + 1]) for b in range(B))
    tok = ens.score(frames, regions, ids.view(B, N, L), return_tokens=True)[2].view(B * N, L)
    live = torch.arange(L, device=DEV).view(1, L) < lens.view(-1, 1)
    diff = (logp - tok)[live]
    print('%s: logp - tok_lp over %d words in [%.3g, %.3g]' % (setting, int(live.sum()), float(diff.min()), float(diff.max())))
    if setting == 'prob':
        # c is the log of a distribution: the sampler's log-sum-exp over the row is 0 in exact arithmetic
        assert float(diff.abs().max()) <= 1e-5
    else:
        # the weighted mean of log-probabilities is not normalised: its log-sum-exp is <= 0 (Jensen), and the sampler, which draws
        # from the renormalised exp(c), reports c minus it
        assert float(diff.min()) >= -1e-5 and float(diff.max()) > 1e-3


@gpu
def test_graph_replays_the_eager_bits(members):
    nets, frames, regions = members
    ens = dlsg_amd.Ensemble(nets, [0.5, 0.3, 0.2], 'prob')
    ex = dlsg_amd.pack_exclusions(ens.decoder.vocab, words=[10, 11], device=DEV)
    for opts in (dict(), dict(top_k=8, top_p=0.9, min_len=3, no_repeat_ngram=2, exclude=ex, return_kept=True)):
        graph = dlsg_amd.EnsembleSampleGraph(ens, frames, regions, N, 0.8, **opts)
        for seed in (21, 22):
            got = [x.clone() for x in graph(frames, regions, seed)]
            want = ens.sample(frames, regions, N, 0.8, seed, **opts)
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), (opts, seed)
        assert not torch.equal(graph(frames, regions, 21)[0], want[0])
    assert graph.valid_for(frames, regions)
    nets[1].train()
    assert not graph.valid_for(frames, regions)
    nets[1].eval()


@gpu
def test_a_baseline_member_alone_samples(members):
    nets, frames, regions = members
    ens = dlsg_amd.Ensemble(nets[2:])
    assert isinstance(nets[2], dlsg_amd.CapBaseline1)
    ids, logp, lens, kept = dlsg_amd.sample(ens, frames, regions, n=N, seed=5, top_k=5, return_kept=True)
    assert ids.shape[0] == B * N and bool(torch.isfinite(logp).all()) and 1 <= int(kept.min()) and int(kept.max()) <= 5
    assert not torch.equal(ids[0], ids[1])

"""GPU: `dlsg_sample_filter_embed` on the MI355X -- the word it draws against `dlsg_sample_embed` on the same row with the words
that are not kept at -inf (kept set from tests/emul_sample.py, float64), the entry point with every control off, edge rows, the
distribution drawn from, the bans, and the controls through `CapGnnModel.sample` / `SampleGraph`.  The CPU side is
tests/test_sample_filter_host.py."""
import functools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import engine as E
from dlsg_amd.hip import HipOps, SAMPLE_FILTER_MAXV
from emul_beam import banned_classes
from emul_sample import apply_bans, kept_sets, tempered
from test_gpu_scst import gpu_net, run_sample
from test_sample_filter_host import repeated_bigrams

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS, W = 64, 64


@pytest.fixture(scope='module')
def ops():
    return HipOps()


@functools.lru_cache(maxsize=None)
def inputs(V):
    """the kernel tests' logits (64, V) and embedding matrix (V, 64), on the host; read-only"""
    x = torch.randn(ROWS, V, generator=torch.Generator().manual_seed(V)) * 3
    return x, torch.randn(V, W, generator=torch.Generator().manual_seed(V + 1))


def run_filter(ops, logits, E_, t=0, end=-1, tau=1.0, p=0.0, seed=7, row0=0, lens=None, hist=None, **opts):
    rows = logits.shape[0]
    ids = torch.empty(rows, dtype=torch.int64, device=DEV)
    out = torch.empty(rows, E_.shape[1], device=DEV)
    logp = torch.empty(rows, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lens = torch.full((rows,), 26, dtype=torch.int64, device=DEV) if lens is None else lens
    ops.sample_filter_embed(logits, E_, ids, out, logp, lens, t, end, temperature=tau, p=p, seed=seed, site=E.SITE_WORD,
                            site_sample=E.SITE_SAMPLE, row0=row0, hist=hist, kept=kept, **opts)
    return ids, out, logp, lens, kept


def check_against_parent(ops, x, E_, tau, top_k=0, top_p=1.0, max_ambiguous=8, t=0, end=-1, min_len=0, g=0, hist=None, seed=99,
                         row0=128):
    """the filtered draw on x against sample_embed on x with the words the float64 rules do not keep at -inf; rows whose nucleus
    boundary float32 cannot decide (emul_sample.AMBIGUOUS) get the looser check.  -> (ids, kept, the CPU kept masks)"""
    z = apply_bans(tempered(x, tau), None if hist is None else hist.cpu().numpy(), t, g, min_len, end)
    if tau > 0:
        keep, larger, amb = kept_sets(z, top_k, top_p)
    else:
        keep = larger = z > -np.inf
        amb = np.zeros(len(z), dtype=bool)
    assert int(amb.sum()) <= max_ambiguous, int(amb.sum())
    masked = x.clone()
    masked[~torch.from_numpy(keep)] = float('-inf')
    xd, Ed = x.to(DEV), E_.to(DEV)
    ids, out, logp, lens, kept = run_filter(ops, xd, Ed, t=t, end=end, tau=tau, p=0.3, seed=seed, row0=row0, hist=hist, top_k=top_k,
                                            top_p=top_p, min_len=min_len, no_repeat_ngram=g)
    wid, wout, wlogp, wlens = run_sample(ops, masked.to(DEV), Ed, t=t, end=end, tau=tau, p=0.3, seed=seed, row0=row0)
    torch.cuda.synchronize()
    ids, kept, wid = ids.cpu(), kept.cpu(), wid.cpu()
    count = torch.from_numpy(keep.sum(1))
    ex = torch.from_numpy(~amb)
    some = ex & (count > 0)
    print('tau %g top_k %d top_p %g: kept %d..%d, ambiguous rows %d, max |dlogp| %.3g' % (
        tau, top_k, top_p, int(kept.min()), int(kept.max()), int(amb.sum()),
        float((logp.cpu()[some] - wlogp.cpu()[some]).abs().max()) if some.any() else 0.0))
    assert torch.equal(ids[ex], wid[ex])
    assert torch.equal(kept[ex].long(), count[ex])
    assert torch.equal(out.cpu()[ex], wout.cpu()[ex]) and torch.equal(lens.cpu()[ex], wlens.cpu()[ex])
    assert (logp.cpu()[some] - wlogp.cpu()[some]).abs().max().item() <= 1e-5 if some.any() else True
    for r in np.nonzero(amb)[0]:
        assert abs(int(kept[r]) - int(count[r])) <= 1, (r, int(kept[r]), int(count[r]))
        assert larger[r, int(ids[r])], (r, int(ids[r]))
    return ids, kept, keep


CASES = [(tau, k, p) for tau in (1.0, 0.7) for k in (0, 50) for p in (1.0, 0.9, 0.5) if (k, p) != (0, 1.0)]


@pytest.mark.parametrize('V', [1000, 10000])
@pytest.mark.parametrize('tau,top_k,top_p', CASES)
def test_draw_equals_sample_embed_on_the_kept_set(ops, V, tau, top_k, top_p):
    x, E_ = inputs(V)
    ids, kept, keep = check_against_parent(ops, x, E_, tau, top_k, top_p)
    assert int(kept.min()) >= 1 and (top_k == 0 or int(kept.max()) <= top_k)


@pytest.mark.parametrize('V', [1000, 10000])
@pytest.mark.parametrize('tau', [1.0, 0.7, 0.0])
def test_all_controls_off_is_sample_embed(ops, V, tau):
    x, E_ = inputs(V)
    x = x.clone()
    x[5, ::13] = float('-inf')
    x[6, 3::17] = float('nan')
    xd, Ed = x.to(DEV), E_.to(DEV)
    end = int(x[0].argmax())
    got = run_filter(ops, xd, Ed, t=2, end=end, tau=tau, p=0.3, seed=31, row0=192)
    want = run_sample(ops, xd, Ed, t=2, end=end, tau=tau, p=0.3, seed=31, row0=192)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3]) and torch.equal(got[1], want[1])
    err = (got[2] - want[2]).abs().max().item()
    print('V %d tau %g: max |dlogp| against sample_embed %.3g' % (V, tau, err))
    assert err <= 1e-6
    assert torch.equal(got[4].cpu().long(), torch.isfinite(x).sum(1))


def test_edge_rows(ops):
    V = 1000
    x, E_ = inputs(V)
    x = x.clone()
    x[3] = float('nan')
    x[4] = float('-inf')
    x[7, ::7] = float('nan')
    # row 8: 9 values above a 5-way tie at the 10th place
    x[8] = torch.randn(V, generator=torch.Generator().manual_seed(8))
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(9))
    x[8, perm[:9]] = 20.0 + torch.arange(9.0)
    x[8, perm[9:14]] = 10.0
    for tau in (1.0, 0.7):
        ids, kept, keep = check_against_parent(ops, x, E_, tau, top_k=50, top_p=0.9)
        assert kept[3] == 0 and kept[4] == 0 and ids[3] == 0 and ids[4] == 0
        ids, kept, keep = check_against_parent(ops, x, E_, tau, top_k=10)
        assert kept[8] == 10 + 5 - 1 and kept[7] == 10 and kept[3] == 0
        fin = torch.isfinite(x).sum(1)
        for k in (V, V + 5):                                          # top_k >= V keeps every finite word
            ids, kept, keep = check_against_parent(ops, x, E_, tau, top_k=k)
            assert torch.equal(kept.long(), fin)
        arg = torch.where(torch.isnan(x), torch.full_like(x, float('-inf')), x).argmax(1)
        arg[3] = arg[4] = 0
        xd, Ed = x.to(DEV), E_.to(DEV)
        for opts in (dict(top_k=1), dict(top_p=1e-6)):                # one word left: the maximum, with probability 1
            got = run_filter(ops, xd, Ed, tau=tau, seed=3, **opts)
            torch.cuda.synchronize()
            ok = fin > 0
            assert torch.equal(got[0].cpu(), arg), opts
            assert (got[2].cpu()[ok] == 0).all() and (got[4].cpu()[ok] == 1).all() and (got[4].cpu()[~ok] == 0).all(), opts
    # temperature 0, <end> the maximum of every row and banned by min_len: the second maximum, untempered log-softmax without <end>
    x[:, 17] = 50.0
    ids, kept, keep = check_against_parent(ops, x, E_, 0.0, top_k=3, top_p=0.2, t=1, end=17, min_len=2)
    y = torch.where(torch.isnan(x), torch.full_like(x, float('-inf')), x)
    y[:, 17] = float('-inf')
    want = y.argmax(1)
    assert torch.equal(ids, want) and (ids != 17).all()
    assert torch.equal(kept.long(), torch.isfinite(y).sum(1))
    ids, kept, keep = check_against_parent(ops, x, E_, 0.0, t=2, end=17, min_len=2)      # t == min_len: <end> is free again
    assert (ids[torch.isfinite(x).any(1)] == 17).all()


def test_sampled_words_follow_the_truncated_distribution(ops):
    from scipy.stats import chi2
    g = torch.Generator().manual_seed(5)
    row = torch.randn(37, generator=g) * 1.5                         # the row of test_sampled_words_follow_the_tempered_softmax
    row[11] = float('-inf')
    rows = 1 << 18
    keep = kept_sets(tempered(row.unsqueeze(0), 1.0), 10, 0.8)[0][0]
    assert 2 <= keep.sum() <= 10
    x = row.to(DEV).unsqueeze(0).expand(rows, 37).contiguous()
    E_ = torch.randn(37, 8, generator=g).to(DEV)
    ids, out, logp, lens, kept = run_filter(ops, x, E_, t=3, tau=1.0, seed=1234, row0=rows, top_k=10, top_p=0.8)
    torch.cuda.synchronize()
    cnt = torch.bincount(ids.cpu(), minlength=37).double().numpy()
    assert (cnt[~keep] == 0).all() and (kept == int(keep.sum())).all()
    zk = torch.where(torch.from_numpy(keep), row.double(), torch.full((37,), float('-inf'), dtype=torch.float64))
    p = torch.softmax(zk, 0).numpy()
    stat = float((((cnt - rows * p) ** 2)[keep] / (rows * p[keep])).sum())
    assert stat < chi2.ppf(1 - 1e-6, int(keep.sum()) - 1), stat
    lsm = torch.log_softmax(zk, 0).to(DEV)
    assert (logp.double() - lsm[ids]).abs().max().item() <= 1e-5
    assert torch.equal(out, E_[ids])


@pytest.mark.parametrize('g,h', [(2, [4, 9, 4, 7, 4]), (3, [4, 9, 5, 4, 9]), (1, [4, 9, 4, 7, 6])])
def test_banned_words_are_never_drawn(ops, g, h):
    V, rows, t, end = 50, 4096, 5, 3
    banned = sorted(banned_classes(h, t, g, 0, end))
    assert banned == {2: [7, 9], 3: [5], 1: [4, 6, 7, 9]}[g]
    row = torch.randn(V, generator=torch.Generator().manual_seed(g))
    row[banned] += 12.0                                               # nearly all of the mass sits on the banned words
    x = row.unsqueeze(0).expand(rows, V).contiguous()
    E_ = torch.randn(V, 8, generator=torch.Generator().manual_seed(1))
    hist = torch.tensor(h, dtype=torch.int64).unsqueeze(1).expand(t, rows).contiguous().to(DEV)
    ids, kept, keep = check_against_parent(ops, x, E_, 1.0, t=t, end=end, g=g, hist=hist)
    assert not np.isin(ids.numpy(), banned).any() and (kept == V - len(banned)).all()
    assert len(set(ids.tolist())) > 10
    plain = run_sample(ops, x.to(DEV), E_.to(DEV), t=t, end=end, seed=99, row0=128)[0].cpu()
    assert np.isin(plain.numpy(), banned).mean() > 0.99
    # with top-k and the nucleus behind the ban, and a history that differs from row to row
    hist2 = hist.clone()
    hist2[:, ::2] = torch.tensor([1, 2, 3, 1, 2], dtype=torch.int64, device=DEV).unsqueeze(1)
    ids, kept, keep = check_against_parent(ops, x, E_, 0.7, top_k=8, top_p=0.9, t=t, end=end, g=g, hist=hist2)
    assert not np.isin(ids[1::2].numpy(), banned).any()


def test_min_len_bans_the_likeliest_end(ops):
    V, rows, end = 50, 4096, 3
    row = torch.randn(V, generator=torch.Generator().manual_seed(2))
    row[end] += 12.0
    x = row.unsqueeze(0).expand(rows, V).contiguous()
    E_ = torch.randn(V, 8, generator=torch.Generator().manual_seed(1))
    ids, kept, keep = check_against_parent(ops, x, E_, 1.0, t=3, end=end, min_len=4)
    assert (ids != end).all() and (kept == V - 1).all()
    ids, kept, keep = check_against_parent(ops, x, E_, 1.0, t=4, end=end, min_len=4)
    assert (ids == end).double().mean() > 0.99 and (kept == V).all()


OPTS = dict(top_k=5, top_p=0.9, min_len=3, no_repeat_ngram=2)


@pytest.mark.parametrize('share', [False, True])
def test_model_level_controls_and_graph_replay(share):
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    net.decoder.word_restore.bias.data[vocab('<end>')] += 3.0          # captions that would end early
    kw = dict(n=4, share_encoder=share, **OPTS)
    a = net.sample(frames, regions, seed=21, return_kept=True, **kw)
    b = net.sample(frames, regions, seed=21, return_kept=True, **kw)
    c = net.sample(frames, regions, seed=22, **kw)
    plain = net.sample(frames, regions, n=4, seed=21, share_encoder=share)
    torch.cuda.synchronize()
    assert len(a) == 4 and len(c) == 3
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], c[0])
    ids, logp, lens, kept = [x.cpu() for x in a]
    assert kept.shape == ids.shape and kept.dtype == torch.int32 and int(kept.min()) >= 1 and int(kept.max()) <= 5
    assert (lens > 3).all() and (plain[2].cpu() <= 3).any()
    assert repeated_bigrams(ids, lens) == []
    assert (logp <= 0).all() and (logp[kept == 1] == 0).all()
    sg = dlsg_amd.SampleGraph(net, frames, regions, n=4, temperature=1.0, share_encoder=share, return_kept=True, **OPTS)
    for s in (21, 22, 5):
        got = [x.clone() for x in sg(frames, regions, s)]
        want = net.sample(frames, regions, seed=s, return_kept=True, **kw)
        torch.cuda.synchronize()
        assert len(got) == 4 and all(torch.equal(x, y) for x, y in zip(got, want)), s


def test_vocabulary_bound(ops):
    """include/dlsg.h: 1 <= V <= DLSG_SAMPLE_FILTER_MAXV (a row is staged in LDS); above it the binding raises before any launch"""
    V = SAMPLE_FILTER_MAXV
    assert V >= 32768
    x = torch.randn(ROWS, V + 1, generator=torch.Generator().manual_seed(V)) * 3
    E_ = torch.randn(V + 1, 8, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError):
        run_filter(ops, x.to(DEV), E_.to(DEV), top_k=50)
    check_against_parent(ops, x[:, :V].contiguous(), E_[:V].contiguous(), 1.0, top_k=50, top_p=0.9)
    ids, kept, keep = check_against_parent(ops, x[:, :V].contiguous(), E_[:V].contiguous(), 0.7, top_p=0.9)
    assert int(kept.max()) > 256
    one = torch.tensor([[0.25]]).to(DEV)                              # V = 1
    got = run_filter(ops, one, torch.ones(1, 8, device=DEV), top_k=3, top_p=0.5)
    torch.cuda.synchronize()
    assert int(got[0]) == 0 and float(got[2]) == 0.0 and int(got[4]) == 1

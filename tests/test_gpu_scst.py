"""GPU: self-critical training on the MI355X -- the sampling kernel (`dlsg_sample_embed`: greedy parity, the distribution it
draws from, its log-probabilities and lengths), the weighted ragged CrossEntropy (`dlsg_ce_ragged_weighted`), replay of the
captured sampler, on-policy log-probabilities, the SCST step against oracle autograd, graphs against eager, and a small run in
which SCST raises CIDEr-D.  The CPU side is tests/test_scst_host.py."""
import math
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import engine as E
from dlsg_amd.hip import HipOps
from dlsg_amd.synth import synth_state_dict, synth_batch
from helpers import small_args
from test_scst_host import LengthReward

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    return HipOps()


def gpu_net(seed=3, n_batch=3, train=False, msvd=False, **kw):
    args = dlsg_amd.msvd_shaped(**kw) if msvd else small_args(**kw)
    V = 1000 if msvd else 50
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    sd = synth_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    net = net.to(DEV).train(train)
    net.update_beam_size(1)
    frames, regions, caps, lens = synth_batch(args, V, n_batch, seed + 1)
    return net, sd, args, vocab, frames.to(DEV), regions.to(DEV), caps.to(DEV), lens


def run_sample(ops, logits, E_, t=0, end=-1, tau=1.0, p=0.0, seed=7, row0=0, lens=None):
    rows = logits.shape[0]
    ids = torch.empty(rows, dtype=torch.int64, device=DEV)
    out = torch.empty(rows, E_.shape[1], device=DEV)
    logp = torch.empty(rows, device=DEV)
    lens = torch.full((rows,), 26, dtype=torch.int64, device=DEV) if lens is None else lens
    ops.sample_embed(logits, E_, ids, out, logp, lens, t, end, temperature=tau, p=p, seed=seed, site=E.SITE_WORD,
                     site_sample=E.SITE_SAMPLE, row0=row0)
    return ids, out, logp, lens


@pytest.mark.parametrize('V', [1000, 10000])
def test_temperature_zero_is_argmax_and_embed(ops, V):
    g = torch.Generator().manual_seed(V)
    rows, W = 64, 512
    x = torch.randn(rows, V, generator=g)
    x[3] = float('nan')                                   # no maximum: word 0
    x[4] = float('-inf')
    x[5, 17] = x[5, 900] = 50.0                           # ties: the first maximum
    x[6, :] = 1.0
    x[7, ::7] = float('nan')
    x = x.to(DEV)
    E_ = torch.randn(V, W, generator=g).to(DEV)
    ids, out, logp, _ = run_sample(ops, x, E_, tau=0.0, p=0.3, seed=99, row0=128)
    want = torch.empty(rows, dtype=torch.int64, device=DEV)
    ops.argmax(x, want)
    torch.cuda.synchronize()
    assert torch.equal(ids, want)
    assert int(ids[3]) == 0 and int(ids[4]) == 0 and int(ids[5]) == 17 and int(ids[6]) == 0
    emb = torch.empty(rows, W, device=DEV)
    ops.embed_fwd(E_, ids, emb, p=0.3, seed=99, site=E.SITE_WORD, row0=128)
    assert torch.equal(out, emb)
    ok = torch.isfinite(x).all(1)
    ref = torch.log_softmax(x[ok].double(), 1).gather(1, ids[ok].view(-1, 1)).view(-1)
    assert (logp[ok].double() - ref).abs().max().item() <= 1e-5


@pytest.mark.parametrize('tau', [1.0, 0.5])
def test_sampled_words_follow_the_tempered_softmax(ops, tau):
    from scipy.stats import chi2
    g = torch.Generator().manual_seed(5)
    row = torch.randn(37, generator=g) * 1.5
    row[11] = float('-inf')
    rows = 1 << 18
    x = row.to(DEV).unsqueeze(0).expand(rows, 37).contiguous()
    E_ = torch.randn(37, 8, generator=g).to(DEV)
    end = int(torch.argsort(row)[-3])                     # a likely word as <end>
    ids, out, logp, lens = run_sample(ops, x, E_, t=3, end=end, tau=tau, seed=1234, row0=rows)
    ids2, _, _, lens2 = run_sample(ops, x, E_, t=5, end=end, tau=tau, seed=4321, row0=2 * rows, lens=lens.clone())
    torch.cuda.synchronize()
    cnt = torch.bincount(ids.cpu(), minlength=37).double().numpy()
    assert cnt[11] == 0
    p = torch.softmax(row.double() / tau, 0).numpy()
    keep = p > 0
    stat = float((((cnt - rows * p) ** 2)[keep] / (rows * p[keep])).sum())
    assert stat < chi2.ppf(1 - 1e-6, int(keep.sum()) - 1), stat
    lsm = torch.log_softmax(row.double() / tau, 0).to(DEV)
    assert (logp.double() - lsm[ids]).abs().max().item() <= 1e-5
    assert torch.equal(out, E_[ids])
    want = torch.where(ids == end, torch.full_like(lens, 4), torch.full_like(lens, 26))
    assert torch.equal(lens, want)
    want2 = torch.where((want == 26) & (ids2 == end), torch.full_like(lens, 6), want)
    assert torch.equal(lens2, want2)
    assert not torch.equal(ids, ids2)


def test_same_seed_same_words_and_graph_replay_equals_eager():
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    a = net.sample(frames, regions, n=4, seed=21)
    b = net.sample(frames, regions, n=4, seed=21)
    c = net.sample(frames, regions, n=4, seed=22)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])
    sg = dlsg_amd.SampleGraph(net, frames, regions, n=4, temperature=1.0)
    for s in (21, 22, 5):
        got = [x.clone() for x in sg(frames, regions, s)]
        want = net.sample(frames, regions, n=4, seed=s)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(got, want)), s


@pytest.mark.parametrize('V', [1000, 10000])
def test_weighted_ce(ops, V):
    B, L = 64, 26
    g = torch.Generator().manual_seed(V + 1)
    logits = torch.randn(L, B, V, generator=g).to(DEV)
    tg = torch.randint(0, V, (B, L), generator=g).to(DEV)
    lens = torch.randint(1, L + 1, (B,), generator=g).to(DEV)
    outs = []
    for w in (None, torch.ones(B, device=DEV), torch.randn(B, generator=g).to(DEV)):
        dl = torch.empty_like(logits)
        rl = torch.empty(L * B, device=DEV)
        loss = torch.empty(1, device=DEV)
        if w is None:
            ops.ce_ragged(logits, tg, lens, dl, rl, loss, time_major=True)
        else:
            ops.ce_ragged_weighted(logits, tg, lens, w, dl, rl, loss, time_major=True)
        outs.append((dl, rl, loss, w))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs[0][:3], outs[1][:3]))
    dl, rl, loss, w = outs[2]
    x = logits.double().transpose(0, 1)                                  # (B, L, V)
    valid = (torch.arange(L, device=DEV).unsqueeze(0) < lens.unsqueeze(1)).double()
    ntot = float(lens.sum())
    lsm = torch.log_softmax(x, -1)
    ce = -lsm.gather(2, tg.unsqueeze(2)).squeeze(2)
    wd = w.double().view(B, 1)
    want_rl = (wd * ce * valid / ntot)
    want_dl = wd.unsqueeze(2) * (lsm.exp() - torch.nn.functional.one_hot(tg, V).double()) * valid.unsqueeze(2) / ntot
    assert (rl.double().view(L, B).t() - want_rl).abs().max().item() <= 1e-6 * want_rl.abs().max().item()
    assert (dl.double().transpose(0, 1) - want_dl).abs().max().item() <= 1e-6 * want_dl.abs().max().item()
    assert abs(float(loss) - float(want_rl.sum())) <= 1e-6 * float(want_rl.abs().sum())


@pytest.mark.parametrize('msvd', [False, True])
def test_sampler_logp_is_on_policy(msvd):
    """train mode: the sampler's log-probabilities equal log_softmax of a teacher-forced train forward over the sampled words
    with the same seed (same dropout masks) -- what the SCST step differentiates."""
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True, msvd=msvd, n_batch=64 if msvd else 3)
    n = 5
    c0 = net.seed_counter
    ids, logp, lens = net.sample(frames, regions, n=n)
    net.seed_counter = c0                               # the forward below draws the same seed
    L = ids.shape[1]
    with torch.no_grad():
        logits = net(frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0), ids, L, 1.0)[0]
    lp = torch.log_softmax(logits.double(), -1).gather(2, ids.unsqueeze(2)).squeeze(2)
    valid = torch.arange(L, device=DEV).unsqueeze(0) < lens.unsqueeze(1)
    err = (lp - logp.double()).abs()[valid].max().item()
    assert err <= 2e-4, err


@pytest.mark.parametrize('msvd', [False, True], ids=['small_3x3', 'msvd_64x5'])
def test_scst_step_gradient_equals_oracle(msvd):
    """The weighted CrossEntropy and the sampled-id backward of one SCST step against oracle autograd on the same weights, ids
    and advantages: a small model with 3 clips x 3 samples, and the MSVD-shaped one at the shape tools/scst_bench.py measures
    (64 clips x 5 samples = 320 rows), every gradient element-wise (helpers.compare_grads)."""
    from oracle import torch_ref as R
    from helpers import compare_grads, oracle_grads
    nb, n = (64, 5) if msvd else (3, 3)
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(dropout=0.0, msvd=msvd, n_batch=nb)
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=n, lr=0.0)
    seen = []
    inner = tr.trainer.step
    tr.trainer.step = lambda *a, **k: seen.append((a, k)) or inner(*a, **k)
    tr.step(frames, regions, [str(i) for i in range(nb)])
    torch.cuda.synchronize()
    (fx, rx, ids, lens, _), kw = seen[0]
    A = kw['seq_weights'].cpu()
    ids, lens = ids.cpu(), lens.cpu()
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    L = ids.shape[1]
    logits = orc(fx.cpu(), rx.cpu(), ids, L, 1.0)[0]
    lp = torch.log_softmax(logits, -1).gather(2, ids.unsqueeze(2)).squeeze(2)
    valid = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).float()
    (-(A.unsqueeze(1) * lp * valid).sum() / lens.sum()).backward()
    G = net.grad_views()
    checked = 0
    for k, p in orc.named_parameters():
        if p.grad is None:
            continue
        err = float((G[k].cpu() - p.grad).abs().max())
        assert err <= 2e-5 + 2e-3 * float(p.grad.abs().max()), (k, err)
        checked += 1
    assert checked > 20
    assert ids.shape[0] == nb * n and float(A.abs().max()) > 0
    compare_grads(G, oracle_grads(orc), 'SCST step, %d clips x %d samples' % (nb, n))


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_scst_graphs_equal_eager(baseline):
    """Three SCST steps replayed as graphs (SampleGraph, GreedyGraph, the Trainer's weighted step) against eager launches
    (device coins in both, so the decoder runs the same launches).  With lr = 0 every sample, advantage, loss, gradient and Adam
    moment is bit-identical.  With a learning rate the eager Adam takes its bias corrections in float on the device and the
    replayed one from the host's double (as for every Trainer), so weights agree to rounding."""
    for lr in (0.0, 1e-3):
        res = []
        for graphs in (True, False):
            net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
            tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=4, baseline=baseline, lr=lr, use_graphs=graphs,
                                      device_coins=True)
            seen = []
            inner = tr.trainer.step
            tr.trainer.step = lambda *a, **k: seen.append((a[2].clone(), k['seq_weights'].clone())) or inner(*a, **k)
            random.seed(1)
            outs = [tr.step(frames, regions, ['0', '1', '2']) for _ in range(3)]
            torch.cuda.synchronize()
            res.append(([float(o['loss']) for o in outs], seen, net._flat.clone(), net._gflat.clone(), tr.trainer.m.clone(),
                        tr.trainer.v.clone()))
        (l0, s0, f0, g0, m0, v0), (l1, s1, f1, g1, m1, v1) = res
        if lr == 0.0:
            assert l0 == l1
            assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(s0, s1))
            assert torch.equal(g0, g1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(f0, f1)
        else:
            assert (f0 - f1).abs().max().item() <= 3e-5


def learning_run(device, ops=None, ce_steps=30, scst_steps=40, lr=1e-4, baseline='mean'):
    """8 clips with distinct features, 3 fixed reference captions each (vocabulary 50): cross-entropy steps on the references,
    then SCST steps with the CIDEr-D of the corpus as the reward.  Returns the greedy CIDEr-D over the 8 clips before and after
    SCST."""
    args = small_args(train_batch_size=8)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    random.seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    if ops is not None:
        net.set_ops(ops)
    net = net.to(device).train()
    net.update_beam_size(1)
    g = torch.Generator().manual_seed(17)
    frames, regions, _, _ = synth_batch(args, 50, 8, 17)
    frames, regions = frames.to(device), regions.to(device)
    words = list(range(4, 50))
    refs, caps, lens = {}, [], []
    for b in range(8):
        pool = [words[i] for i in torch.randperm(len(words), generator=g)[:6].tolist()]
        sents = []
        for k in range(3):
            n = 4 + k
            ids = [pool[(i * (k + 1) + k) % len(pool)] for i in range(n)]
            sents.append(ids)
        refs[str(b)] = [' '.join(vocab.idx2word[i] for i in s) for s in sents]
        caps.append(sents[0] + [vocab('<end>')] + [0] * (26 - len(sents[0]) - 1))
        lens.append(len(sents[0]) + 1)
    caps = torch.tensor(caps, dtype=torch.int64, device=device)
    reward = dlsg_amd.CiderD(refs)
    vids = [str(b) for b in range(8)]

    def greedy_cider():
        net.eval()
        with torch.no_grad():
            ids = net(frames, regions, None)[0].cpu()
        net.train()
        return float(reward.scores(vids, [net.decoder.decode_tokens(x) for x in ids]).mean())
    tr = dlsg_amd.Trainer(net, lr=2e-3)
    for _ in range(ce_steps):
        tr.step(frames, regions, caps, lens, 1.0)
    before = greedy_cider()
    scst = dlsg_amd.SCSTTrainer(net, reward, n_samples=5, baseline=baseline, lr=lr)
    for _ in range(scst_steps):
        scst.step(frames, regions, vids)
    return before, greedy_cider()


def test_scst_raises_greedy_cider():
    """Greedy CIDEr-D over the 8 clips after the 30 cross-entropy steps / after 40 SCST steps: 1.9753 / 2.4476 on an MI355X
    (1.9753 / 2.3955 with the kernel emulation of tests/test_scst_host.py on the CPU)."""
    before, after = learning_run(DEV)
    print('greedy CIDEr-D before / after SCST: %.4f / %.4f' % (before, after))
    assert after > before, (before, after)

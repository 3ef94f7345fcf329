"""GPU: minimum-risk training on the MI355X -- the two launches of csrc/risk.hip against `dlsg_amd.risk_loss_reference` under float64
autograd on the device, their edge cases and refusals, two launches bit for bit, the `MRTTrainer` step against oracle autograd
(with seq_per_clip and with expanded rows), three captured steps against three eager ones for both searches, descent on fixed
lists, and the plain and the SCST step unchanged.  The CPU side is tests/test_risk_host.py.

Tolerance.  The float32 token terms (each within 2^-24 of a few units, up to L of them) enter an exponent scaled by alpha, the
weight c and the row are float32: the project's 1e-6 is not derivable here.  The bound is 4 x the largest error measured on an
MI355X over the cases of test_kernels_against_float64 (the convention of tests/test_gpu_soft_ce.py; DESIGN.md section 36 holds the
measured figures), one bound per quantity: dlogits relative to max|want|, Q absolute (max Q is of order 1), s relative to max|s|,
the loss relative to |loss|.  The largest figure, 1.6e-6 on dlogits, is the L = 64 case: 64 float32 token terms of a few units
each carry about 2e-7, their sum a few 1e-6 in absolute terms, and alpha / len^length_penalty of that enters the exponent of Q."""
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd.hip import HipOps
from test_gpu_scst import gpu_net
from test_risk_host import fixed_lists, risk_case
from test_scst_host import LengthReward

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# the largest error of each quantity over all cases of test_kernels_against_float64, measured on an MI355X; the bound is 4 x that
MEASURED = {'dlogits': 1.585e-6, 'Q': 2.475e-7, 's': 6.278e-8, 'loss': 4.935e-8}
TOL = {k: 4 * v for k, v in MEASURED.items()}
KEYS = ('dlogits', 'Q', 's', 'loss')
GUARD = 256
FILL = 7.5
SHAPES = [(6, 3, 4, 37), (6, 3, 4, 1024), (6, 3, 4, 1031), (64, 1, 2, 37), (4, 2, 32, 37)]       # (L, B, n, V)


@pytest.fixture(scope='module')
def ops():
    return HipOps()


def guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def launch(ops, logits, targets, lens, rewards, mask, n, tm, alpha, lp, only_rows=False):
    """both launches on (rows, L, V) logits given batch-major; -> dict of outputs, dlogits batch-major; every output sits between
    guard blocks that must keep their fill"""
    rows, L, V = logits.shape
    x = (logits.transpose(0, 1) if tm else logits).contiguous()
    bufs = {k: guarded(m, dt) for k, m, dt in (('lse', rows * L, torch.float32), ('tok', rows * L, torch.float32),
                                               ('dl', max(x.numel(), 1), torch.float32), ('Q', rows, torch.float64),
                                               ('s', rows, torch.float64), ('R', max(rows // max(n, 1), 1), torch.float64),
                                               ('loss', 1, torch.float32), ('stats', 4, torch.float64))}
    o = {k: v[1] for k, v in bufs.items()}
    dl = o['dl'][:x.numel()].view(x.shape)
    err = None
    try:
        ops.risk_rows(x, targets, lens, o['lse'], o['tok'], n, tm)
        if not only_rows:
            ops.risk_grad(x, targets, lens, o['lse'], o['tok'], rewards, mask, dl, o['Q'], o['s'], o['R'][:rows // max(n, 1)], o['loss'],
                          o['stats'], n, tm, alpha, lp)
    except RuntimeError as e:
        err = e
    torch.cuda.synchronize()
    for buf, _ in bufs.values():
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())
    o['dlogits'] = dl.transpose(0, 1) if tm else dl
    o['err'] = err
    return o


def reference(logits, targets, lens, rewards, mask, n, alpha, lp):
    x = logits.double().requires_grad_(True)
    loss, parts = dlsg_amd.risk_loss_reference(x, targets, lens, rewards, n, mask=mask, alpha=alpha, length_penalty=lp, return_parts=True)
    loss.backward()
    return loss.detach(), x.grad, {k: v.detach() for k, v in parts.items()}


def on_device(case):
    return [x.to(DEV) for x in case]


@pytest.mark.parametrize('tm', [True, False])
@pytest.mark.parametrize('L,B,n,V', SHAPES)
def test_kernels_against_float64(ops, L, B, n, V, tm):
    logits, targets, lens, rewards, mask = on_device(risk_case(L, B, n, V))
    worst = [0.0] * 4
    for (alpha, lp), m in [((1.0, 1.0), mask), ((0.5, 0.0), mask), ((2.0, 0.5), None), ((0.05, 0.0), mask)]:
        got = launch(ops, logits, targets, lens, rewards, m, n, tm, alpha, lp)
        assert got['err'] is None
        loss, grad, parts = reference(logits, targets, lens, rewards, m, n, alpha, lp)
        assert float(grad.abs().max()) > 0
        e = [float((got['dlogits'].double() - grad).abs().max() / grad.abs().max()),
             float((got['Q'] - parts['Q'].reshape(-1)).abs().max()),
             float((got['s'] - parts['s'].reshape(-1)).abs().max() / parts['s'].abs().max()),
             float(abs(got['stats'][0] - loss) / abs(loss))]
        assert float(got['loss'][0]) == float(got['stats'][0].float())                  # the float32 loss is the rounded float64 one
        print('L %d B %d n %d V %d time_major %d alpha %g lp %g: dlogits %.3g, Q %.3g, s %.3g, loss %.3g' % (L, B, n, V, tm, alpha, lp, *e))
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert all(x <= TOL[k] for k, x in zip(KEYS, e)), (alpha, lp, e)
        # R_b = sum_i Q_bi r_bi: at most n errors of Q, each times the largest reward
        assert float((got['R'][:B] - parts['R']).abs().max()) <= n * TOL['Q'] * float(rewards.abs().max())
        assert float(got['stats'][3]) == -float(got['stats'][0])
        # the zero fill behind a caption's end, a masked candidate and a clip without a counted candidate: exact zeros
        live = torch.arange(L, device=DEV)[None, :] < lens.clamp(max=L)[:, None]
        assert not bool(got['dlogits'][~live].any())
        if m is not None:
            assert not bool(got['dlogits'][~m].any()) and not bool(got['Q'][~m].any())
            if B >= 3:
                assert float(got['R'][B - 1]) == 0.0 and not bool(got['dlogits'][(B - 1) * n:].any())
        keep = (lens >= 1) if m is None else m
        assert float(got['stats'][1]) == pytest.approx(float(rewards[keep].mean()), rel=1e-12)
        assert float(got['stats'][2]) == pytest.approx(float(lens.clamp(max=L)[keep].double().mean()), rel=1e-12)
        again = launch(ops, logits, targets, lens, rewards, m, n, tm, alpha, lp)
        assert all(torch.equal(got[k], again[k]) for k in ('dlogits', 'Q', 's', 'loss', 'stats', 'lse', 'tok'))
    print('L %d B %d n %d V %d time_major %d: largest error dlogits %.3g, Q %.3g, s %.3g, loss %.3g' % (L, B, n, V, tm, *worst))


@pytest.mark.parametrize('tm', [True, False])
@pytest.mark.parametrize('n,alpha', [(1, 1.0), (4, 0.0)])
def test_no_gradient_for_one_candidate_or_alpha_zero(ops, n, alpha, tm):
    logits, targets, lens, rewards, mask = on_device(risk_case(6, 3 if n > 1 else 12, n, 37))
    got = launch(ops, logits, targets, lens, rewards, mask, n, tm, alpha, 1.0)
    loss, grad, parts = reference(logits, targets, lens, rewards, mask, n, alpha, 1.0)
    assert got['err'] is None and not bool(grad.any())
    assert float(got['dlogits'].abs().max()) <= TOL['dlogits']
    assert float(abs(got['stats'][0] - loss)) <= TOL['loss'] * float(abs(loss))
    assert float((got['Q'] - parts['Q'].reshape(-1)).abs().max()) <= TOL['Q']


@pytest.mark.parametrize('tm', [True, False])
def test_bad_target_is_nan_in_its_clip_only(ops, tm):
    L, B, n, V = 6, 3, 4, 37
    logits, targets, lens, rewards, mask = on_device(risk_case(L, B, n, V, bad=True))
    got = launch(ops, logits, targets, lens, rewards, None, n, tm, 1.0, 1.0)
    assert got['err'] is None
    assert bool(torch.isnan(got['loss']).all()) and bool(torch.isnan(got['stats'][0])) and bool(torch.isnan(got['R'][1]))
    assert bool(torch.isnan(got['dlogits'][n, 0]).all())                            # the row of the bad target
    other = torch.cat([got['dlogits'][:n], got['dlogits'][2 * n:]])
    assert bool(torch.isfinite(other).all()) and bool(other.any()) and bool(torch.isfinite(got['R'][[0, 2]]).all())
    live = torch.arange(L, device=DEV)[None, :] < lens.clamp(max=L)[:, None]
    assert not bool(got['dlogits'][~live].any())


def test_refusals_launch_nothing(ops):
    for L, B, n, V, rows in [(6, 1, 33, 37, 33), (65, 2, 2, 37, 4), (6, 2, 2, 0, 4), (6, 2, 3, 37, 7)]:
        g = torch.Generator().manual_seed(1)
        logits = torch.randn(rows, L, V, generator=g).to(DEV)
        targets = torch.zeros(rows, L, dtype=torch.int64, device=DEV)
        lens = torch.full((rows,), L, dtype=torch.int64, device=DEV)
        rewards = torch.ones(rows, dtype=torch.float64, device=DEV)
        got = launch(ops, logits, targets, lens, rewards, None, n, True, 1.0, 1.0, only_rows=True)
        assert got['err'] is not None and 'risk_rows' in str(got['err']), (L, B, n, V, rows)
        assert bool((got['lse'] == FILL).all()) and bool((got['tok'] == FILL).all())
        # the second launch on its own refuses the same shapes, and a negative alpha
        bufs = {k: guarded(m, dt)[1] for k, m, dt in (('lse', rows * L, torch.float32), ('tok', rows * L, torch.float32),
                                                       ('Q', rows, torch.float64), ('s', rows, torch.float64), ('R', rows, torch.float64),
                                                       ('loss', 1, torch.float32), ('stats', 4, torch.float64))}
        dl = torch.full_like(logits.transpose(0, 1).contiguous(), FILL)
        with pytest.raises(RuntimeError, match='risk_grad'):
            ops.risk_grad(logits.transpose(0, 1).contiguous(), targets, lens, bufs['lse'], bufs['tok'], rewards, None, dl, bufs['Q'],
                          bufs['s'], bufs['R'][:max(rows // n, 1)], bufs['loss'], bufs['stats'], n, True, 1.0, 1.0)
        torch.cuda.synchronize()
        assert bool((dl == FILL).all()) and all(bool((b == FILL).all()) for b in bufs.values())
    logits, targets, lens, rewards, mask = on_device(risk_case(6, 3, 4, 37))
    for alpha, lp in ((-1.0, 0.0), (float('nan'), 0.0), (1.0, float('inf'))):
        got = launch(ops, logits, targets, lens, rewards, mask, 4, True, alpha, lp)
        assert got['err'] is not None and 'risk_grad' in str(got['err'])
        assert all(bool((got[k] == FILL).all()) for k in ('dl', 'Q', 's', 'R', 'loss', 'stats'))


@pytest.mark.parametrize('share', [True, False])
def test_mrt_step_gradient_equals_oracle(share):
    """One MRTTrainer step on 3 clips x 3 fixed candidates (a callable), rewards from the LengthReward stub, against autograd of
    risk_loss_reference on the oracle's logits: every gradient element-wise, once with seq_per_clip and once with expanded rows"""
    from oracle import torch_ref as R
    from helpers import compare_grads, oracle_grads
    n = 3
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(dropout=0.0)
    tr = dlsg_amd.MRTTrainer(net, LengthReward(), n_candidates=n, candidates=fixed_lists(n), alpha=0.7, length_penalty=0.5,
                             share_encoder=share, lr=0.0)
    seen = []
    inner = tr.trainer.step
    tr.trainer.step = lambda *a, **k: seen.append((a, k)) or inner(*a, **k)
    out = tr.step(frames, regions, ['0', '1', '2'])
    torch.cuda.synchronize()
    (fx, rx, ids, lens, _), kw = seen[0]
    assert kw.get('seq_per_clip', 1) == (n if share else 1) and fx.shape[0] == (3 if share else 9)
    risk = kw['risk']
    ids, lens, fx, rx = ids.cpu(), lens.cpu(), fx.cpu(), rx.cpu()
    if share:
        fx, rx = fx.repeat_interleave(n, 0), rx.repeat_interleave(n, 0)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    L = ids.shape[1]
    logits = orc(fx, rx, ids, L, 1.0)[0]
    loss = dlsg_amd.risk_loss_reference(logits, ids, lens, risk['rewards'].cpu(), n, mask=risk['mask'].cpu(), alpha=0.7, length_penalty=0.5)
    loss.backward()
    print('loss %.9g, oracle %.9g' % (float(out['loss']), float(loss.detach())))
    assert abs(float(out['loss']) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
    G = net.grad_views()
    checked = 0
    for k, p in orc.named_parameters():
        if p.grad is None:
            continue
        err = float((G[k].cpu() - p.grad).abs().max())
        assert err <= 2e-5 + 2e-3 * float(p.grad.abs().max()), (k, err)
        checked += 1
    assert checked > 20 and max(float(p.grad.abs().max()) for p in orc.parameters() if p.grad is not None) > 1e-4
    compare_grads(G, oracle_grads(orc), 'MRT step, 3 clips x 3 candidates, share_encoder %s' % share)


@pytest.mark.parametrize('source', ['swor', 'beam'])
def test_mrt_graphs_equal_eager(source):
    """Three MRTTrainer steps replayed as graphs (the captured search, the Trainer's risk form) against eager launches, lr = 0:
    candidates, Q, loss, gradient and both Adam moments bit for bit; every candidate is counted, so no masked list hides a difference"""
    res = []
    opts = dict(min_len=2) if source == 'swor' else dict(beam_size=4, length_penalty=0.5)
    for graphs in (True, False):
        net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
        tr = dlsg_amd.MRTTrainer(net, LengthReward(), n_candidates=4, candidates=source, candidate_options=opts, lr=0.0,
                                 use_graphs=graphs, device_coins=True)
        seen = []
        inner = tr.trainer.step
        tr.trainer.step = lambda *a, **k: seen.append((a[2].clone(), a[3].clone(), k['risk']['mask'].clone())) or inner(*a, **k)
        random.seed(1)
        outs = []
        for _ in range(3):
            o = tr.step(frames, regions, ['0', '1', '2'])
            outs.append((float(o['loss']), float(o['expected_reward']), tr.trainer.last_risk['Q'].clone()))
        torch.cuda.synchronize()
        res.append((outs, seen, net._flat.clone(), net._gflat.clone(), tr.trainer.m.clone(), tr.trainer.v.clone()))
    (o0, s0, f0, g0, m0, v0), (o1, s1, f1, g1, m1, v1) = res
    assert all(bool(s[2].all()) for s in s0 + s1)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(s0, s1))
    assert all(a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) for a, b in zip(o0, o1))
    assert bool(g0.any()) and torch.equal(g0, g1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(f0, f1)


def test_mrt_descends_on_fixed_lists():
    """fixed candidate lists, dropout 0, 20 steps at a small lr: the loss -- the negative expected reward -- goes down"""
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(dropout=0.0, train=True)
    tr = dlsg_amd.MRTTrainer(net, LengthReward(), n_candidates=3, candidates=fixed_lists(3), alpha=1.0, length_penalty=1.0, lr=2e-4)
    losses = [float(tr.step(frames, regions, ['0', '1', '2'])['loss']) for _ in range(20)]
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]


def test_plain_and_scst_steps_unchanged():
    """two fresh trainers of each kind, the second built after an MRTTrainer was built and stepped on a model of its own: the same
    launch count and the same bits in loss, weights, gradient and Adam moments"""
    def plain():
        net, sd, args, vocab, frames, regions, caps, lens = gpu_net(train=True)
        tr = dlsg_amd.Trainer(net, lr=1e-3)
        random.seed(5)
        n0 = net.ops.launches
        loss = float(tr.step(frames, regions, caps, lens, 0.8))
        torch.cuda.synchronize()
        return loss, net.ops.launches - n0, net._flat.clone(), net._gflat.clone(), tr.m.clone(), tr.v.clone()

    def scst():
        net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
        tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=3, lr=1e-3)
        random.seed(5)
        n0 = net.ops.launches
        loss = float(tr.step(frames, regions, ['0', '1', '2'])['loss'])
        torch.cuda.synchronize()
        return loss, net.ops.launches - n0, net._flat.clone(), net._gflat.clone(), tr.trainer.m.clone(), tr.trainer.v.clone()

    before = plain(), scst()
    from dlsg_amd import mrt                                              # noqa: F401
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    dlsg_amd.MRTTrainer(net, LengthReward(), n_candidates=3, candidates=fixed_lists(3), lr=1e-3).step(frames, regions, ['0', '1', '2'])
    after = plain(), scst()
    for a, b in zip(before, after):
        assert a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))

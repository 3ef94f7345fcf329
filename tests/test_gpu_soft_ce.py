"""GPU: `dlsg_ce_ragged_soft` on the MI355X against the float64 restatement of tests/emul_soft_ce.py computed with torch on the
device, its edge cases and refusals, two launches bit for bit, and the train step with label smoothing and a two-member teacher:
the gradient arena against the emulated step of tests/test_soft_ce_host.py, and three captured steps against three eager ones.

Tolerances.  M = 0 (label smoothing only) is ce_ragged_weighted's arithmetic plus one sum: the project's 1e-6 * max|want| for
dlogits and the row losses and 1e-6 * sum|want| for the three sums.  With teachers q goes through float32 x - lse, expf and, in
mode 1, a second normalisation; the bound is 4 x the largest error measured over the cases of test_kernel_against_float64
(DESIGN.md section 18 holds the measured figures), and rounding alone cannot exceed about 1e-5 * max|want|."""
import itertools
import random

import pytest
import torch

import dlsg_amd
from dlsg_amd.hip import HipOps
from dlsg_amd.synth import synth_batch, synth_state_dict
from emul_soft_ce import SoftCeEmul, soft_ce_reference
from helpers import compare_grads, small_args
from test_beam_nbest_host import MODELS
from test_ensemble_host import member_specs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, L = 5, 26
LENS = [26, 19, 30, 5, 1]                    # full, ragged, longer than L, short, a single word
TOL0 = 1e-6                                  # M == 0
# M > 0, per mode, relative to max|want| (dlogits, row losses) and to sum|want| (the three sums): 4 x the largest measured
# (measured on an MI355X over that test's cases: mode 0 3.13e-7, mode 1 2.84e-7)
TOL = {0: 4 * 3.13e-7, 1: 4 * 2.84e-7}
CEIL = 1e-5                                  # what rounding alone cannot exceed: log-probabilities below 32 carry at most 2^-19 each
GUARD = 256


@pytest.fixture(scope='module')
def ops():
    return HipOps()


def inputs(V, tm, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 * V + 10 * int(tm) + seed)
    shape = (L, B, V) if tm else (B, L, V)
    logits = (torch.randn(*shape, generator=g) * scale).to(DEV)
    teachers = [(torch.randn(*shape, generator=g) * scale).to(DEV) for _ in range(8)]
    tg = torch.randint(0, V, (B, L), generator=g).to(DEV)
    w = torch.randn(B, generator=g).to(DEV)
    tw = (torch.rand(8, generator=g) + 0.2).tolist()
    return logits, teachers, tg, torch.tensor(LENS, device=DEV), w, tw


def launch(ops, logits, tg, lens, tm, **kw):
    """-> (dlogits, row losses (3, B, L), sums (3,)); dlogits sits between two guard blocks that must keep their fill"""
    buf = torch.full((logits.numel() + 2 * GUARD,), 7.5, device=DEV)
    dl = buf[GUARD:GUARD + logits.numel()].view(logits.shape)
    rbuf = torch.full((3 * B * L + 2 * GUARD,), 7.5, device=DEV)
    rl = rbuf[GUARD:GUARD + 3 * B * L]
    lbuf = torch.full((3 + 2 * GUARD,), 7.5, device=DEV)
    loss = lbuf[GUARD:GUARD + 3]
    ops.ce_ragged_soft(logits, tg, lens, dl, rl, loss, tm, **kw)
    torch.cuda.synchronize()
    for x in (buf, rbuf, lbuf):
        assert bool((x[:GUARD] == 7.5).all()) and bool((x[-GUARD:] == 7.5).all())
    rows = rl.view(3, L, B).transpose(1, 2) if tm else rl.view(3, B, L)
    return dl, rows, loss


def errors(got, want):
    """(dlogits, row losses) relative to max|want|, the three sums relative to sum|row terms|"""
    (dl, rows, loss), (wd, wr, ws) = got, want
    e_dl = float((dl.double() - wd).abs().max() / wd.abs().max())
    e_rows = max(float((rows[k].double() - wr[k]).abs().max() / wr[k].abs().max()) for k in range(3) if float(wr[k].abs().max()) > 0)
    e_sum = max(float(abs(loss[k].double() - ws[k]) / wr[k].abs().sum()) for k in range(3) if float(wr[k].abs().sum()) > 0)
    return e_dl, e_rows, e_sum


# ---------------------------------------------------------------- 1. the kernel against float64
@pytest.mark.parametrize('tm', [True, False])
@pytest.mark.parametrize('V', [61, 1000, 10007])
def test_kernel_against_float64(ops, V, tm):
    logits, teachers, tg, lens, w, tw = inputs(V, tm)
    worst = {None: 0.0, 0: 0.0, 1: 0.0}
    for eps, weights in itertools.product((0.0, 0.1), (None, w)):
        for mode in (0, 1):                                          # M == 0: either mode word is accepted and ignored
            kw = dict(smoothing=eps, weights=weights, mode=mode)
            got = launch(ops, logits, tg, lens, tm, **kw)
            e = errors(got, soft_ce_reference(logits, tg, lens, tm, **kw))
            worst[None] = max(worst[None], *e)
            assert max(e) <= TOL0, (V, tm, kw, e)
            assert float(got[2][2]) == 0.0 and not bool(got[1][2].any())     # no teacher: no kd
        if eps == 0.0 and weights is not None:
            # the existing kernel on the same inputs (bit equality is not required: an fma contraction may differ)
            dl0, rl0, loss0 = torch.empty_like(logits), torch.empty(B * L, device=DEV), torch.empty(1, device=DEV)
            ops.ce_ragged_weighted(logits, tg, lens, weights, dl0, rl0, loss0, tm)
            torch.cuda.synchronize()
            r0 = rl0.view(L, B).t() if tm else rl0.view(B, L)
            assert float((got[0] - dl0).abs().max()) <= TOL0 * float(dl0.abs().max())
            assert float((got[1][1] - r0).abs().max()) <= TOL0 * float(r0.abs().max())
            for k in (0, 1):
                assert abs(float(got[2][k]) - float(loss0)) <= TOL0 * float(r0.abs().sum())
        for M, mode, alpha in itertools.product((1, 2, 8), (0, 1), (0.5, 1.0)):
            kw = dict(smoothing=eps, weights=weights, teachers=teachers[:M], teacher_weights=tw[:M], mode=mode, alpha=alpha)
            got = launch(ops, logits, tg, lens, tm, **kw)
            e = errors(got, soft_ce_reference(logits, tg, lens, tm, **kw))
            worst[mode] = max(worst[mode], *e)
            assert max(e) <= TOL[mode], (V, tm, M, mode, alpha, eps, weights is not None, e)
    print('V %d time_major %d: largest relative error, M = 0: %.3g; mode 0: %.3g; mode 1: %.3g'
          % (V, tm, worst[None], worst[0], worst[1]))


def test_strided_teacher_rows(ops):
    """a teacher whose rows are V floats of a wider buffer (teacher_ld != V)"""
    V = 61
    logits, teachers, tg, lens, w, tw = inputs(V, True)
    wide = torch.full((L, B, V + 3), 1e30, device=DEV)
    wide[..., :V] = teachers[1]
    kw = dict(smoothing=0.1, weights=w, teacher_weights=tw[:2], mode=1, alpha=0.5)
    a = launch(ops, logits, tg, lens, True, teachers=[teachers[0], wide[..., :V]], **kw)
    b = launch(ops, logits, tg, lens, True, teachers=teachers[:2], **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- edge cases
@pytest.mark.parametrize('V', [61, 1000])
def test_teachers_that_disagree_completely_give_a_distribution(ops, V):
    """mode 1, two one-hot-like rows at logit scale 30 on different classes: exp(sum_m w_m l_mj) is ~e^-15 at best, so the
    normaliser must be taken around the row maximum; q is finite and sums to 1 (read off sum_j dlogits_j = (1 - sum_j q_j) / ntot
    at alpha = 1, eps = 0, no weights)"""
    logits, _, tg, lens, _, _ = inputs(V, True)
    g = torch.Generator().manual_seed(V)
    cls = torch.stack([torch.randperm(V, generator=g)[:2] for _ in range(L * B)]).to(DEV)       # two different classes per row
    teachers = []
    for m in range(2):
        x = torch.zeros(L * B, V, device=DEV)
        x.scatter_(1, cls[:, m:m + 1], 30.0)
        teachers.append(x.view(L, B, V))
    kw = dict(teachers=teachers, teacher_weights=[1.0, 1.0], mode=1, alpha=1.0)
    dl, rows, loss = launch(ops, logits, tg, lens, True, **kw)
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(loss).all())
    ntot = float(torch.tensor(LENS).clamp(max=L).sum())
    valid = (torch.arange(L, device=DEV).unsqueeze(1) < lens.clamp(max=L).unsqueeze(0))          # (L, B)
    qsum = 1.0 - dl.double().sum(-1) * ntot
    err = float((qsum - 1.0).abs()[valid].max())
    print('V %d: |sum q - 1| <= %.3g' % (V, err))
    assert err <= 1e-5
    # the two chosen classes share the mass: dlogits there is (p - 1/2) / ntot up to e^-15
    # (teacher log-probabilities of magnitude 30, not the unit-scale rows TOL was measured on: the rounding ceiling applies)
    e = errors((dl, rows, loss), soft_ce_reference(logits, tg, lens, True, **kw))
    print('V %d: largest relative error %.3g' % (V, max(e)))
    assert max(e) <= CEIL


def test_target_outside_the_vocabulary_is_nan_and_writes_nothing_out_of_bounds(ops):
    V = 61
    logits, teachers, tg, lens, w, tw = inputs(V, False)
    tg = tg.clone()
    tg[1, 3], tg[2, 0], tg[3, 20] = V, -1, V + 5                  # two counted rows; (3, 20) is padding and stays zero
    for kw in (dict(smoothing=0.1), dict(teachers=teachers[:2], teacher_weights=tw[:2], mode=0, alpha=0.5)):
        dl, rows, loss = launch(ops, logits, tg, lens, False, **kw)                  # (the guard blocks are checked in there)
        assert bool(torch.isnan(loss).all())
        bad = torch.zeros(B, L, dtype=torch.bool, device=DEV)
        bad[1, 3] = bad[2, 0] = True
        assert bool(torch.isnan(dl[bad]).all()) and bool(torch.isnan(rows[:, bad]).all())
        assert bool(torch.isfinite(dl[~bad]).all()) and bool(torch.isfinite(rows[:, ~bad]).all())
        assert not bool(dl[3, 20].any()) and not bool(rows[:, 3, 20].any())
        wd, wr, _ = soft_ce_reference(logits, tg, lens, False, **kw)
        assert float((dl.double() - wd)[~bad].abs().max()) <= TOL[0] * float(wd[~bad].abs().max())


@pytest.mark.parametrize('V', [1000, 10007])
def test_nll_part_is_the_weighted_kernels_loss(ops, V):
    logits, teachers, tg, lens, w, tw = inputs(V, True)
    w = w.abs() + 0.5
    dl0, rl0, loss0 = torch.empty_like(logits), torch.empty(B * L, device=DEV), torch.empty(1, device=DEV)
    ops.ce_ragged_weighted(logits, tg, lens, w, dl0, rl0, loss0, True)
    for kw in (dict(smoothing=0.1), dict(smoothing=0.1, teachers=teachers[:3], teacher_weights=tw[:3], mode=1, alpha=0.5)):
        _, _, loss = launch(ops, logits, tg, lens, True, weights=w, **kw)
        d = abs(float(loss[1]) - float(loss0))
        print('V %d: nll part %.9g, ce_ragged_weighted %.9g' % (V, float(loss[1]), float(loss0)))
        assert d <= 1e-6 * abs(float(loss0))


def test_refusals(ops):
    V = 61
    logits, teachers, tg, lens, w, tw = inputs(V, True)
    dl = torch.full_like(logits, 7.5)
    rl = torch.full((3 * B * L,), 7.5, device=DEV)
    loss = torch.full((3,), 7.5, device=DEV)
    two = dict(teachers=teachers[:2], alpha=0.5)
    for kw in (dict(teachers=teachers + teachers[:1], alpha=0.5), dict(mode=2, **two), dict(mode=-1, **two), dict(mode=2),
               dict(smoothing=-0.1), dict(smoothing=1.0), dict(smoothing=float('nan')),
               dict(teachers=teachers[:2], alpha=-0.1), dict(teachers=teachers[:2], alpha=1.5), dict(teachers=teachers[:2], alpha=float('nan')),
               dict(alpha=0.5), dict(teachers=teachers[:2], alpha=0.0)):
        with pytest.raises(RuntimeError, match='ce_ragged_soft'):
            ops.ce_ragged_soft(logits, tg, lens, dl, rl, loss, True, **kw)
    torch.cuda.synchronize()
    assert bool((dl == 7.5).all()) and bool((rl == 7.5).all()) and bool((loss == 7.5).all())       # a refusal launches nothing
    # no rows: nothing to launch
    ops.ce_ragged_soft(logits[:0], tg[:, :0].contiguous(), lens, dl[:0], rl, loss, True, smoothing=0.1)
    torch.cuda.synchronize()
    assert bool((loss == 7.5).all())


# ---------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize('mode', [0, 1])
def test_two_launches_give_the_same_bits(ops, mode):
    logits, teachers, tg, lens, w, tw = inputs(1000, True)
    kw = dict(smoothing=0.1, weights=w, teachers=teachers[:3], teacher_weights=tw[:3], mode=mode, alpha=0.5)
    a, b = launch(ops, logits, tg, lens, True, **kw), launch(ops, logits, tg, lens, True, **kw)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---------------------------------------------------------------- 3. the train step
def nets(dev, train=False, emul=False):
    """student (CapGnnModel) and a two-member teacher of two classes (a CapGnnModel of other hidden sizes, a CapBaseline1) with
    seeded weights, vocabulary 50, on `dev`; emul: on the emulated kernels"""
    vocab = dlsg_amd.make_vocab(50)
    specs = [('capgnn', small_args(), 3)] + member_specs()[1:]
    out = []
    for kind, args, seed in specs:
        args.dropout = 0.3 if train and not out else 0.0
        torch.manual_seed(0)
        net = MODELS[kind][0](args, vocab)
        net.load_state_dict(synth_state_dict(net.state_dict(), seed))
        net = net.to(dev).train(train and not out)
        if emul:
            net.set_ops(SoftCeEmul())
        net.update_beam_size(1)
        out.append(net)
    return out[0], dlsg_amd.Ensemble(out[1:], weights=[0.6, 0.4])


def batch(n, dev):
    args = small_args()
    frames, regions, caps, lens = synth_batch(args, 50, 3, 4)
    if n > 1:
        _, _, caps, lens = synth_batch(args, 50, 3 * n, 61)
    return frames.to(dev), regions.to(dev), caps[:, :26].contiguous().to(dev), torch.as_tensor(lens).to(dev)


OPTS = dict(label_smoothing=0.1, distill_weight=0.5)


@pytest.mark.parametrize('n', [1, 2])
def test_step_gradient_equals_the_emulated_step(n):
    got = {}
    for dev in ('cpu', DEV):
        net, teacher = nets(dev, emul=dev == 'cpu')
        tr = dlsg_amd.Trainer(net, lr=0.0, teacher=teacher, **OPTS)
        tr.step(*batch(n, dev), 1.0, seq_per_clip=n)
        if dev == DEV:
            torch.cuda.synchronize()
        got[dev] = (net, net.grad_views(), tr.last_loss_parts.detach().cpu().clone())
    net = got['cpu'][0]
    want = {k: (None if k in net.unused_parameters else got['cpu'][1][k]) for k, _ in net.named_parameters()}
    compare_grads(got[DEV][1], want, 'GPU step against the emulated step, n %d' % n)
    err = float((got[DEV][2] - got['cpu'][2]).abs().max())
    print('loss parts %s, emulated %s' % (got[DEV][2].tolist(), got['cpu'][2].tolist()))
    assert err <= 1e-4               # (the two sides' logits differ by rounding of the whole forward pass; the parts are ~4)


def run_steps(use_graphs, n, steps=3, repack_after=None, **kw):
    net, teacher = nets(DEV, train=True)
    tr = dlsg_amd.Trainer(net, lr=1e-3, use_graphs=use_graphs, device_coins=True, teacher=teacher, check_every=0, **OPTS, **kw)
    data = batch(n, DEV)
    random.seed(1)
    parts, old = [], None
    for i in range(steps):
        if i == repack_after:
            m = teacher.members[0]
            graphs = tr._graphs
            assert graphs is not None
            old, m._flat = m._flat, None
            m.flatten_parameters_()                       # what load_state_dict into a copy / .to() lead to: a new arena
            assert m._flat is not old and m._flat.data_ptr() != old.data_ptr()
        tr.step(*data, 1.0, seq_per_clip=n)
        if i == repack_after:
            assert tr._graphs is not None and tr._graphs is not graphs          # dropped and captured again
        parts.append(tr.last_loss_parts.clone())
    torch.cuda.synchronize()
    assert (tr._graphs is not None) == use_graphs
    return net._flat.clone(), tr.m.clone(), tr.v.clone(), parts


def same_bits(a, b):
    (fa, ma, va, pa), (fb, mb, vb, pb) = a, b
    assert torch.equal(fa, fb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert len(pa) == len(pb) and all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert all(bool(torch.isfinite(x).all()) and float(x[2]) > 0.0 for x in pa)


@pytest.mark.parametrize('n,kw', [(1, {}), (2, {'max_grad_norm': 1.0})], ids=['n1', 'n2_clipped'])
def test_three_captured_steps_equal_three_eager_steps(n, kw):
    same_bits(run_steps(False, n, **kw), run_steps(True, n, **kw))


# ---------------------------------------------------------------- 4. a re-packed teacher arena
def test_repacked_teacher_arena_recaptures():
    same_bits(run_steps(False, 1), run_steps(True, 1, repack_after=2))

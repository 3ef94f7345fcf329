"""GPU (-m gpu): gradient clipping on the device -- dlsg_grad_sumsq / dlsg_clip_coef against numpy float64 on the same values,
dlsg_adam_clipped against dlsg_adam (bit for bit where the clip is idle), the emulation and torch, and the Trainer / SCSTTrainer
steps that carry them (eager, captured, with the RCCL collectives in the graph).  Host logic: tests/test_grad_clip_host.py."""
import functools
import math
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from helpers import load_case, weights_and_inputs
from test_grad_clip_host import ClipEmul, Oracle, check_weights, NORM, COEF, NONFINITE

pytestmark = pytest.mark.gpu
DEV = 'cuda'

U64, U32 = 2.0 ** -53, 2.0 ** -24


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def slots_of(hip):
    from dlsg_amd.hip import GRAD_SUMSQ_SLOTS
    return GRAD_SUMSQ_SLOTS


@functools.lru_cache(maxsize=None)
def values():
    """2^22 + 5 gradient-like floats (host float32 array and its device copy), made once for every size"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2 ** 22 + 5, generator=g) * torch.rand(2 ** 22 + 5, generator=g) * 3e-2
    return x.numpy(), x.to(DEV)


def poisoned_view(n, off, src=None):
    """a device view of n floats starting `off` floats past a 16-byte boundary, NaN on either side of it"""
    buf = torch.full((n + 12,), float('nan'), device=DEV)
    view = buf[4 + off:4 + off + n]
    assert view.data_ptr() % 16 == 4 * off
    view.copy_(values()[1][:n] if src is None else src)
    return buf, view


def record_of(hip, views, grad_scale, max_norm, skipped=None):
    S = slots_of(hip)
    slots = torch.full((S * len(views),), float('nan'), dtype=torch.float64, device=DEV)     # never pre-zeroed
    for i, v in enumerate(views):
        hip.grad_sumsq(v, slots[i * S:(i + 1) * S])
    rec = torch.full((4,), -1.0, device=DEV)
    hip.clip_coef(slots, grad_scale, max_norm, rec, skipped)
    torch.cuda.synchronize()
    return slots.cpu().numpy(), rec.cpu().numpy()


@functools.lru_cache(maxsize=None)
def exact_sumsq(n):
    x64 = values()[0][:n].astype(np.float64)
    return math.fsum((x64 * x64).tolist())


def check_record(slots, rec, want, n, grad_scale, max_norm):
    """want: the exact sum of the n squares.  The squares are exact in float64 and the terms non-negative, so any order of
    summation is within n * 2^-53 of it; the norm adds the rounding of the root and of the float32 store."""
    got = math.fsum(slots.tolist())
    print('n = %d: sum %.17g, exact %.17g, rel err %.3g (bound %.3g)' % (n, got, want, abs(got - want) / max(want, 1e-300), n * U64))
    assert abs(got - want) <= n * U64 * want
    norm = grad_scale * math.sqrt(want)
    assert abs(float(rec[NORM]) - norm) <= 3 * U32 * norm, (float(rec[NORM]), norm)
    # the coefficient is float32 arithmetic on the float32 norm of the record: the same in numpy, the device's divide allowed 2 ulp
    coef = min(np.float32(1), np.float32(max_norm) / (rec[NORM] + np.float32(1e-6)))
    assert abs(float(rec[COEF]) - float(coef)) <= 4 * U32 * float(coef) and rec[NONFINITE] == 0.0 and float(rec[COEF]) <= 1.0


def sizes(hip=None):
    from dlsg_amd import abi
    sweep = abi.defines['DLSG_GRAD_SUMSQ_SLOTS'] * 256 * 4        # floats one pass of the grid covers with 16-byte loads
    return [1, 3, 4, 5, 255, 256, 257, 1023, sweep - 1, sweep, sweep + 1, 2 ** 22 + 5]


@pytest.mark.parametrize('n', sizes())
def test_sumsq_and_coef_against_numpy_float64(hip, n):
    for off in range(4):
        buf, view = poisoned_view(n, off)
        slots, rec = record_of(hip, [view], 0.25, 1e-3 if off % 2 else 1e9)
        assert np.isfinite(slots).all()                  # the NaNs around the range were not read
        check_record(slots, rec, exact_sumsq(n), n, 0.25, 1e-3 if off % 2 else 1e9)
        assert bool(torch.isnan(buf[:4 + off]).all()) and bool(torch.isnan(buf[4 + off + n:]).all())


@pytest.mark.parametrize('lens', [(1000, 300001), (77, 1000, 300001)])
def test_ranges_combine_to_the_sum_over_their_union(hip, lens):
    x = values()[0]
    views, parts, at = [], [], 0
    for i, n in enumerate(lens):
        parts.append(x[at:at + n])
        views.append(poisoned_view(n, (i + 1) % 4, values()[1][at:at + n]))
        at += n
    slots, rec = record_of(hip, [v for _, v in views], 0.5, 0.01)
    x64 = np.concatenate(parts).astype(np.float64)
    check_record(slots, rec, math.fsum((x64 * x64).tolist()), x64.size, 0.5, 0.01)
    assert float(rec[COEF]) < 1.0


def test_record_is_bit_identical_across_launches_and_graph_replay(hip):
    S = slots_of(hip)
    _, a = poisoned_view(300001, 1)
    _, b = poisoned_view(4099, 3)
    slots = torch.empty(2 * S, dtype=torch.float64, device=DEV)
    rec = torch.empty(4, device=DEV)

    def launch():
        hip.grad_sumsq(a, slots[:S])
        hip.grad_sumsq(b, slots[S:])
        hip.clip_coef(slots, 1.0, 0.05, rec)
    got = []
    for _ in range(2):
        slots.fill_(float('nan')); rec.fill_(-1.0)
        launch()
        torch.cuda.synchronize()
        got.append((slots.clone(), rec.clone()))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        slots.fill_(float('nan')); rec.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got.append((slots.clone(), rec.clone()))
    for s, r in got[1:]:
        assert torch.equal(s.view(torch.int64), got[0][0].view(torch.int64)) and torch.equal(r.view(torch.int32), got[0][1].view(torch.int32))
    assert 0.0 < float(got[0][1][COEF]) < 1.0


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')])
def test_non_finite_element_sets_the_flag_and_counts(hip, bad):
    skipped = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    for i, at in enumerate((0, 70001, 300000)):                       # scalar head, aligned body, tail
        _, v = poisoned_view(300001, 1)
        v[at] = bad
        _, rec = record_of(hip, [v], 1.0, 1.0, skipped)
        assert rec[NONFINITE] == 1.0 and rec[COEF] == 0.0 and not np.isfinite(rec[NORM])
        assert int(skipped.item()) == 42 + i
    _, v = poisoned_view(300001, 1)
    _, rec = record_of(hip, [v], 1.0, 1.0, skipped)                   # a clean gradient leaves the counter alone
    assert rec[NONFINITE] == 0.0 and int(skipped.item()) == 44


def adam_state(seed, tot):
    g = torch.Generator().manual_seed(seed)
    p0, gr = torch.randn(tot, generator=g), torch.randn(tot, generator=g)
    m0, v0 = torch.randn(tot, generator=g).abs() * 0.1, torch.randn(tot, generator=g).abs() * 0.1
    return p0, gr, m0, v0


HP = (1.6e-4, 0.5, 0.9, 1e-8, 3, 0.5)           # lr, b1, b2, eps, step, grad_scale of tests/test_gpu_ops.py's Adam range test


def bits(t):
    return t.view(torch.int32)


def test_adam_clipped_has_adams_bits_when_the_clip_is_idle_and_skips_a_non_finite_step(hip):
    off, n = 1, 100003
    p0, gr, m0, v0 = adam_state(5, off + n + 9)
    sl = slice(off, off + n)

    def run(fn, **kw):
        p, m, v, g = p0.to(DEV), m0.to(DEV), v0.to(DEV), gr.to(DEV)
        fn(p[sl], g[sl], m[sl], v[sl], *HP, **kw)
        torch.cuda.synchronize()
        return p, m, v
    want = run(hip.adam)
    S = slots_of(hip)
    slots = torch.empty(S, dtype=torch.float64, device=DEV)
    rec = torch.empty(4, device=DEV)
    hip.grad_sumsq(gr.to(DEV)[sl], slots)
    hip.clip_coef(slots, 0.5, 1e4, rec)                               # norm ~ 158 < max_norm: coef == 1.0
    torch.cuda.synchronize()
    assert float(rec[COEF]) == 1.0 and abs(float(rec[NORM]) - 0.5 * float(gr[sl].double().norm())) <= 3 * U32 * float(rec[NORM])
    for kw in (dict(record=rec), dict(record=None, clip_value=0.0), dict()):
        got = run(hip.adam_clipped, **kw)
        for a, b in zip(got, want):
            assert torch.equal(bits(a), bits(b)), kw
    assert not torch.equal(want[0], p0.to(DEV))
    rec[NONFINITE] = 1.0
    rec[COEF] = 0.0
    got = run(hip.adam_clipped, record=rec)
    for a, b in zip(got, (p0, m0, v0)):
        assert torch.equal(bits(a.cpu()), bits(b))


@pytest.mark.parametrize('mode', ['norm', 'value'])
@pytest.mark.parametrize('off,n', [(0, 5000), (1, 4999), (3, 1026), (2, 3), (5, 1), (0, 4), (7, 100003)])
def test_adam_clipped_ranges_at_any_offset(hip, off, n, mode):
    """offsets and sizes of tests/test_gpu_ops.py::test_adam_ranges_at_any_offset, against the emulation at its 1e-6"""
    tot = off + n + 9
    p0, gr, m0, v0 = adam_state(off * 100 + n, tot)
    rec = torch.tensor([3.0, 0.37, 0.0, 0.0]) if mode == 'norm' else None
    kw = dict(record=rec, clip_value=0.0) if mode == 'norm' else dict(record=None, clip_value=0.3)
    p, gg, m, v = p0.clone().to(DEV), gr.to(DEV), m0.clone().to(DEV), v0.clone().to(DEV)
    sl = slice(off, off + n)
    hip.adam_clipped(p[sl], gg[sl], m[sl], v[sl], *HP, **dict(kw, record=None if rec is None else rec.to(DEV)))
    torch.cuda.synchronize()
    pe, me, ve = p0.clone(), m0.clone(), v0.clone()
    ClipEmul().adam_clipped(pe[sl], gr[sl], me[sl], ve[sl], *HP, **kw)
    for a, b in ((p, pe), (m, me), (v, ve)):
        assert (a.cpu() - b).abs().max().item() <= 1e-6
        assert torch.equal(a.cpu()[:off], b[:off]) and torch.equal(a.cpu()[off + n:], b[off + n:])        # nothing outside the range
    assert not torch.equal(pe, p0)


def test_clipped_adam_matches_clip_grad_norm_and_torch_optim(hip):
    """tests/test_gpu_ops.py::test_adam_matches_torch_optim with clip_grad_norm_ in front of the update, at its 1e-6"""
    g = torch.Generator().manual_seed(3)
    p0, grads = torch.randn(5000, generator=g), [torch.randn(5000, generator=g) for _ in range(3)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1.6e-4, betas=(0.5, 0.9))
    p = p0.clone().to(DEV); m = torch.zeros_like(p); v = torch.zeros_like(p)
    slots = torch.empty(slots_of(hip), dtype=torch.float64, device=DEV)
    rec = torch.empty(4, device=DEV)
    max_norm = 5.0                                                    # |randn(5000) / 4| ~ 17.7: every step clips
    for i, gr in enumerate(grads):
        ref.grad = gr.clone() / 4
        norm = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        gd = gr.to(DEV)
        hip.grad_sumsq(gd, slots)
        hip.clip_coef(slots, 0.25, max_norm, rec)
        hip.adam_clipped(p, gd, m, v, 1.6e-4, 0.5, 0.9, 1e-8, i + 1, 0.25, record=rec)
        torch.cuda.synchronize()
        want = float((gr.double() / 4).norm())               # (torch's own norm is a float32 sum: not the yardstick here)
        assert float(norm) > max_norm and abs(float(rec[NORM]) - want) <= 3 * U32 * want
    assert (p.cpu() - ref.detach()).abs().max().item() <= 1e-6


# ---------------------------------------------------------------- Trainer, small config (B = 3)
def build():
    args, vocab, g, kind = load_case('small_msvd')
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd, frames, regions, caps, lens = weights_and_inputs(net, g, args)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV), args, vocab, sd, (frames, regions, caps, lens)


def two_steps(**kw):
    """-> (trainer, [(weights, record) after each of two steps])"""
    collectives = kw.pop('force_collectives', False)
    net, args, vocab, sd, (frames, regions, caps, lens) = build()
    tr = dlsg_amd.Trainer(net, **kw)
    tr.force_collectives = collectives
    out = []
    for _ in range(2):
        tr.step(frames.to(DEV), regions.to(DEV), caps.to(DEV), lens, 1.0)
        torch.cuda.synchronize()
        out.append((net._flat.clone(), None if tr.last_grad_norm is None else tr._clip_rec.clone()))
    return tr, out


@functools.lru_cache(maxsize=None)
def reference_runs():
    """the oracle's two clipped steps (max_norm = half the unclipped norm of step 1) and the captured trainer's, made once"""
    net, args, vocab, sd, batch = build()
    probe = Oracle(args, vocab, sd)
    probe.grads(*batch)
    max_norm = 0.5 * probe.norm()
    orc = Oracle(args, vocab, sd)
    tr, got = two_steps(use_graphs=True, max_grad_norm=max_norm)
    return max_norm, orc, batch, tr, got


def test_trainer_eager_and_captured_steps_agree_bit_for_bit():
    max_norm, _, _, tr_g, captured = reference_runs()
    tr_e, eager = two_steps(use_graphs=False, device_coins=True, max_grad_norm=max_norm)
    assert tr_g._graphs is not None and len(tr_g._graphs) == 1 and tr_e._graphs is None
    for (fe, re_), (fg, rg) in zip(eager, captured):
        print('grad norm eager %.9g captured %.9g; max|dw| %.3g' % (float(re_[NORM]), float(rg[NORM]), float((fe - fg).abs().max())))
        assert torch.equal(bits(re_), bits(rg))
        assert torch.equal(bits(fe), bits(fg))
    assert float(captured[0][1][COEF]) < 1.0


def test_trainer_with_a_huge_max_norm_has_the_unclipped_trainers_bits():
    tr, got = two_steps(use_graphs=True, max_grad_norm=1e30)
    tr0, want = two_steps(use_graphs=True)
    for (f, r), (f0, _) in zip(got, want):
        assert float(r[COEF]) == 1.0 and float(r[NORM]) > 0.0
        assert torch.equal(bits(f), bits(f0))
    assert torch.equal(bits(tr.m), bits(tr0.m)) and torch.equal(bits(tr.v), bits(tr0.v)) and int(tr.skipped_steps) == 0


def test_trainer_clipped_steps_match_the_oracle():
    """as tests/test_grad_clip_host.py, at the bound of tests/test_gpu_parity.py::test_trainer_step_loss_and_adam (1e-4)"""
    max_norm, orc, batch, _, _ = reference_runs()
    net, args, vocab, sd, (frames, regions, caps, lens) = build()
    tr = dlsg_amd.Trainer(net, max_grad_norm=max_norm)
    for step in range(2):
        want_loss = orc.step(*batch, max_norm=max_norm)
        loss = tr.step(frames.to(DEV), regions.to(DEV), caps.to(DEV), lens, 1.0)
        assert abs(float(loss) - float(want_loss)) <= 1e-4
        got, want = float(tr.last_grad_norm), orc.norms[-1]
        print('step %d: grad norm %.9g, oracle %.9g, max_norm %.9g' % (step + 1, got, want, max_norm))
        assert want > max_norm and abs(got - want) <= 1e-4 * want
        check_weights(net, orc, 1e-4)
    assert int(tr.skipped_steps) == 0


def test_captured_clipped_step_makes_no_host_synchronisation():
    _, _, (frames, regions, caps, lens), tr, _ = reference_runs()
    f, r, c, ln = frames.to(DEV), regions.to(DEV), caps.to(DEV), lens.to(DEV)
    every, tr.check_every = tr.check_every, 0
    before = tr.model._flat.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        tr.step(f, r, c, ln, 1.0)
        norm, skipped = tr.last_grad_norm, tr.skipped_steps
    finally:
        torch.cuda.set_sync_debug_mode('default')
        tr.check_every = every
    torch.cuda.synchronize()
    assert norm.is_cuda and norm.dim() == 0 and skipped.is_cuda and skipped.dim() == 0
    assert float(norm) > 0 and int(skipped) == 0 and not torch.equal(before, tr.model._flat)


def test_clip_launches_stay_inside_the_one_graph_with_rccl_collectives():
    max_norm, _, _, _, captured = reference_runs()
    tr, got = two_steps(use_graphs=True, comm='rccl', max_grad_norm=max_norm, force_collectives=True)
    try:
        info = tr.collectives_info()
        assert info['graph_replays_per_step'] == 1 and info['where'] == "inside the step's hipGraph", info
        assert tr._adam_in_graph and tr._rccl is not None
        # one rank: the all-reduce is the identity, the step that of the trainer without collectives
        for (f, r), (f0, r0) in zip(got, captured):
            assert torch.equal(bits(r), bits(r0)) and torch.equal(bits(f), bits(f0))
    finally:
        tr.close()


def test_scst_step_with_clipping_reports_the_norm_without_a_host_synchronisation():
    from dlsg_amd import scoring as S
    from test_gpu_cider_device import gpu_net, scst_corpus, no_host_sync
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    reward = S.CiderD(scst_corpus(vocab)).to_device(vocab)
    tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, lr=1e-3, use_graphs=True, check_every=0, max_grad_norm=0.1)
    vids = ['0', '1', '2']
    random.seed(1)
    for _ in range(2):
        tr.step(frames, regions, vids)                      # captures
    torch.cuda.synchronize()
    with no_host_sync():
        out = tr.step(frames, regions, vids)
    torch.cuda.synchronize()
    gn = out['grad_norm']
    assert torch.is_tensor(gn) and gn.is_cuda and gn.dim() == 0 and gn.dtype == torch.float32
    assert math.isfinite(float(gn)) and float(gn) > 0 and float(gn) == float(tr.trainer.last_grad_norm)
    assert np.isfinite(float(out['loss']))

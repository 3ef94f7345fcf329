"""CPU: gradient clipping inside the train step (`Trainer(max_grad_norm=...)` / `Trainer(clip_grad_value=...)`) -- where the
clip launches sit in the schedule, what they compute against torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam
on the oracle, the skipped non-finite step, and two ranks over gloo.  The three new kernels are emulated in torch (`ClipEmul`,
below; tests/test_gpu_grad_clip.py holds the real ones against it)."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dlsg_amd
from emul_ops import EmulOps
from test_scst_host import ScstEmul, LengthReward

HERE = os.path.dirname(os.path.abspath(__file__))
NORM, COEF, NONFINITE = 0, 1, 2            # include/dlsg.h DLSG_CLIP_*
CLIP_OPS = ('grad_sumsq', 'clip_coef', 'adam_clipped')


def _sig(x):
    """what a launch argument is, without its values: a tensor by dtype / shape / strides / offset into its storage"""
    if torch.is_tensor(x):
        return ('T', str(x.dtype), tuple(x.shape), tuple(x.stride()), x.storage_offset())
    if isinstance(x, (list, tuple)):
        return tuple(_sig(y) for y in x)
    if isinstance(x, dict):
        return tuple((k, _sig(v)) for k, v in sorted(x.items()))
    if isinstance(x, (int, float, bool, str)) or x is None:
        return x
    return type(x).__name__


class ClipEmul(ScstEmul):
    """ScstEmul + dlsg_grad_sumsq / dlsg_clip_coef / dlsg_adam_clipped.  `log` (a list) collects (name, arguments) of every public
    op called while it is set; `inject` (a callable) runs once on the gradient view of the next grad_sumsq launch."""

    log = None
    inject = None

    def __getattribute__(self, name):
        v = ScstEmul.__getattribute__(self, name)
        log = object.__getattribute__(self, '__dict__').get('log')
        if log is not None and not name.startswith('_') and callable(v) and name not in ('log', 'inject'):
            def call(*a, **k):
                log.append((name, _sig(a), _sig(k)))
                return v(*a, **k)
            return call
        return v

    def grad_sumsq(self, g, slots):
        hook = self.__dict__.get('inject')
        if hook is not None:
            self.inject = None
            hook(g)
        assert slots.dtype == torch.float64
        slots.zero_()                                   # every slot is written: the caller never clears them
        slots[0] = (g.double() ** 2).sum()

    def clip_coef(self, slots, grad_scale, max_norm, record, skipped=None):
        with np.errstate(all='ignore'):
            norm = np.float32(float(grad_scale) * math.sqrt(float(slots.sum()))) if float(slots.sum()) >= 0 else np.float32('nan')
            bad = not np.isfinite(norm)
            coef = np.float32(0) if bad else min(np.float32(1), np.float32(max_norm) / (norm + np.float32(1e-6)))
        record[NORM], record[COEF], record[NONFINITE], record[3] = float(norm), float(coef), float(bad), 0.0
        if bad and skipped is not None:
            skipped += 1

    def adam_clipped(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, hyper=None, record=None, clip_value=0.0):
        coef = 1.0
        if record is not None:
            if float(record[NONFINITE]) != 0.0:
                return
            coef = record[COEF]
        gi = (g * grad_scale) * coef
        if clip_value > 0:
            gi = gi.clamp(-clip_value, clip_value)
        EmulOps.adam(self, p, gi, m, v, lr, b1, b2, eps, step, 1.0, hyper=hyper)


def small_net(seed=3, emul=ClipEmul, batch=3, **kw):
    from dlsg_amd.synth import synth_state_dict, synth_batch
    from helpers import small_args
    args = small_args(dropout=0.0, **kw)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    net.set_ops(emul())
    net.update_beam_size(1)
    frames, regions, caps, lens = synth_batch(args, 50, batch, seed + 1)
    return net, sd, args, vocab, frames, regions, caps, lens


class Oracle(object):
    """oracle.torch_ref gradients -> clip -> torch.optim.Adam(betas=(0.5, 0.9)); `norms` holds each step's unclipped norm"""

    def __init__(self, args, vocab, sd, lr=1.6e-4):
        from oracle import torch_ref as R
        self.R = R
        self.model = R.CapGnnModelRef(args, vocab).eval()
        self.model.load_state_dict(sd)
        self.opt = torch.optim.Adam(self.model.parameters(), lr=lr, betas=(0.5, 0.9))
        self.norms = []

    def grads(self, frames, regions, caps, lens):
        self.opt.zero_grad()
        outs = self.model(frames, regions, caps, 26, 1.0)[0]
        loss = self.R.ragged_ce(outs, caps, lens)
        loss.backward()
        return loss.detach()

    def norm(self):
        return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in self.model.parameters() if p.grad is not None)))

    def step(self, frames, regions, caps, lens, max_norm=None, clip_value=None):
        loss = self.grads(frames, regions, caps, lens)
        self.norms.append(self.norm())
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_norm)
        if clip_value is not None:
            torch.nn.utils.clip_grad_value_(self.model.parameters(), clip_value)
        self.opt.step()
        return loss


def check_weights(net, orc, tol):
    """tests/test_engine_host_logic.py::test_trainer_step_matches_reference_adam's criterion -- every parameter's sum against the
    oracle's within tol * max(1, sum |p|) -- with the oracle's weights computed here instead of read from a fixture"""
    ref = dict(orc.model.named_parameters())
    for k, p in net.named_parameters():
        r = ref[k].detach().double()
        s, a = float(r.sum()), float(r.abs().sum())
        got = float(p.detach().double().sum())
        assert abs(got - s) <= tol * max(1.0, a), (k, got, s)


def test_default_path_issues_the_launches_it_issued_before():
    logs = []
    for kw in ({}, {'max_grad_norm': None, 'clip_grad_value': None}):
        net, sd, args, vocab, frames, regions, caps, lens = small_net()
        tr = dlsg_amd.Trainer(net, lr=1e-3, **kw)
        assert tr.last_grad_norm is None and tr.skipped_steps is None
        net.ops.log = []
        for _ in range(2):
            tr.step(frames, regions, caps, lens, 1.0)
        logs.append(net.ops.log)
        net.ops.log = None
    assert logs[0] == logs[1]
    names = [c[0] for c in logs[0]]
    assert 'adam' in names and not set(names) & set(CLIP_OPS)
    # and with an option: the same launches up to the update, then one grad_sumsq per trainable range, one clip_coef, and
    # adam_clipped in place of adam
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    tr = dlsg_amd.Trainer(net, lr=1e-3, max_grad_norm=1.0)
    net.ops.log = []
    tr.step(frames, regions, caps, lens, 1.0)
    log, net.ops.log = net.ops.log, None
    one = logs[0][:len(logs[0]) // 2]
    cut = [c[0] for c in one].index('adam')
    assert log[:cut] == one[:cut]
    n = len(tr._train_ranges)
    assert [c[0] for c in log[cut:]] == ['grad_sumsq'] * n + ['clip_coef'] + ['adam_clipped'] * n
    assert [c[0] for c in one[cut:]] == ['adam'] * n


def test_both_options_exclude_each_other():
    net = small_net()[0]
    with pytest.raises(ValueError):
        dlsg_amd.Trainer(net, max_grad_norm=1.0, clip_grad_value=0.1)
    with pytest.raises(ValueError):
        dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, max_grad_norm=1.0, clip_grad_value=0.1)


def test_two_clipped_steps_match_clip_grad_norm_and_torch_adam():
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    probe = Oracle(args, vocab, sd)
    probe.grads(frames, regions, caps, lens)
    max_norm = 0.5 * probe.norm()                        # half the unclipped norm of step 1: the clip is active
    orc = Oracle(args, vocab, sd)
    tr = dlsg_amd.Trainer(net, max_grad_norm=max_norm)
    for step in range(2):
        want_loss = orc.step(frames, regions, caps, lens, max_norm=max_norm)
        loss = tr.step(frames, regions, caps, lens, 1.0)
        assert abs(float(loss) - float(want_loss)) <= 1e-5
        got, want = float(tr.last_grad_norm), orc.norms[-1]
        print('step %d: grad norm %.9g, oracle %.9g, max_norm %.9g' % (step + 1, got, want, max_norm))
        assert tr.last_grad_norm.dim() == 0 and abs(got - want) <= 1e-5 * want
        assert want > max_norm                           # both steps clip
        check_weights(net, orc, 2e-5)
    assert int(tr.skipped_steps) == 0
    # the clip took part: the unclipped trainer ends elsewhere
    net2 = small_net()[0]
    tr2 = dlsg_amd.Trainer(net2)
    for step in range(2):
        tr2.step(frames, regions, caps, lens, 1.0)
    assert not torch.equal(net2._flat, net._flat)


def test_infinite_max_norm_reports_and_clips_nothing():
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    net2 = small_net()[0]
    tr, tr2 = dlsg_amd.Trainer(net, max_grad_norm=float('inf')), dlsg_amd.Trainer(net2)
    for _ in range(2):
        tr.step(frames, regions, caps, lens, 1.0)
        tr2.step(frames, regions, caps, lens, 1.0)
    assert torch.equal(net._flat, net2._flat) and torch.equal(tr.m, tr2.m) and torch.equal(tr.v, tr2.v)
    assert float(tr.last_grad_norm) > 0 and float(tr._clip_rec[COEF]) == 1.0


def test_two_value_clipped_steps_match_clip_grad_value_and_torch_adam():
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    probe = Oracle(args, vocab, sd)
    probe.grads(frames, regions, caps, lens)
    gmax = max(float(p.grad.abs().max()) for p in probe.model.parameters() if p.grad is not None)
    c = 0.1 * gmax                                       # a tenth of the largest element: the clamp is active
    orc = Oracle(args, vocab, sd)
    tr = dlsg_amd.Trainer(net, clip_grad_value=c)
    for step in range(2):
        want_loss = orc.step(frames, regions, caps, lens, clip_value=c)
        loss = tr.step(frames, regions, caps, lens, 1.0)
        assert abs(float(loss) - float(want_loss)) <= 1e-5
        assert abs(float(tr.last_grad_norm) - orc.norms[-1]) <= 1e-5 * orc.norms[-1]          # the norm before the clamp
        check_weights(net, orc, 2e-5)
    assert float(net._gflat.abs().max()) > c


def test_non_finite_gradient_skips_the_step():
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    tr = dlsg_amd.Trainer(net, max_grad_norm=1.0)
    tr.step(frames, regions, caps, lens, 1.0)
    assert int(tr.skipped_steps) == 0
    before = [t.clone() for t in (net._flat, tr.m, tr.v)]

    def poison(g):
        g[g.numel() // 2] = float('nan')
    net.ops.inject = poison
    tr.step(frames, regions, caps, lens, 1.0)
    for a, b in zip(before, (net._flat, tr.m, tr.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))       # bit for bit
    assert int(tr.skipped_steps) == 1 and math.isnan(float(tr.last_grad_norm)) and tr.t == 2
    tr.step(frames, regions, caps, lens, 1.0)                               # the next clean step updates
    assert int(tr.skipped_steps) == 1 and math.isfinite(float(tr.last_grad_norm))
    assert not torch.equal(before[0], net._flat) and not torch.equal(before[1], tr.m)
    assert bool(torch.isfinite(net._flat).all()) and bool(torch.isfinite(tr.v).all())


def test_scst_stats_carry_the_grad_norm_only_when_clipping():
    net, sd, args, vocab, frames, regions, _, _ = small_net()
    plain = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, lr=1e-4)
    assert sorted(plain.step(frames, regions, ['0', '1', '2'])) == ['baseline_mean', 'loss', 'mean_len', 'reward_mean']
    net = small_net()[0]
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, lr=1e-4, max_grad_norm=0.1)
    out = tr.step(frames, regions, ['0', '1', '2'])
    assert sorted(out) == ['baseline_mean', 'grad_norm', 'loss', 'mean_len', 'reward_mean']
    gn = out['grad_norm']
    assert torch.is_tensor(gn) and gn.dim() == 0 and float(gn) == float(tr.trainer.last_grad_norm) > 0
    want = float(net._gflat.double().norm())
    assert abs(float(gn) - want) <= 1e-6 * want


# ---------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build4():
    return small_net(seed=7, batch=4)


def _worker(rank, world, port, out_dir, max_norm):
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    net, sd, args, vocab, frames, regions, caps, lens = _build4()
    sl = slice(rank * 2, rank * 2 + 2)
    tr = dlsg_amd.Trainer(net, world_size=world, max_grad_norm=max_norm)
    tr.step(frames[sl], regions[sl], caps[sl], lens[sl], 1.0)
    np.save(os.path.join(out_dir, 'flat%d.npy' % rank), net._flat.numpy())
    np.save(os.path.join(out_dir, 'rec%d.npy' % rank), tr._clip_rec.numpy())
    dist.destroy_process_group()


def test_two_ranks_clip_alike_on_the_norm_of_the_mean_gradient(tmp_path):
    # one process: the gradients of the two shards, their mean, its norm
    net, sd, args, vocab, frames, regions, caps, lens = _build4()
    tr = dlsg_amd.Trainer(net, lr=0.0)
    grads = []
    for r in range(2):
        sl = slice(r * 2, r * 2 + 2)
        tr.step(frames[sl], regions[sl], caps[sl], lens[sl], 1.0)
        grads.append(net._gflat.clone())
    want_norm = float((0.5 * (grads[0].double() + grads[1].double())).norm())
    max_norm = 0.5 * want_norm
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), max_norm), nprocs=2, join=True)
    f0, f1 = np.load(tmp_path / 'flat0.npy'), np.load(tmp_path / 'flat1.npy')
    r0, r1 = np.load(tmp_path / 'rec0.npy'), np.load(tmp_path / 'rec1.npy')
    assert np.array_equal(r0.view(np.int32), r1.view(np.int32))            # same norm, coefficient and skip decision, bit for bit
    assert np.array_equal(f0, f1)                                          # replicas stay bit-identical
    print('two ranks: grad norm %.9g, one process %.9g' % (r0[NORM], want_norm))
    assert abs(float(r0[NORM]) - want_norm) <= 1e-5 * want_norm and r0[NONFINITE] == 0 and 0.49 < r0[COEF] < 0.51
    # one Adam step on the clipped mean, in one process
    net2 = _build4()[0]
    tr2 = dlsg_amd.Trainer(net2, max_grad_norm=max_norm)
    net2._gflat.copy_(grads[0] + grads[1])
    tr2.world_size = 2
    tr2._clip_grads()
    tr2._adam(1)
    assert np.abs(net2._flat.numpy() - f0).max() <= 1e-6

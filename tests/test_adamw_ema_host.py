"""CPU: weight decay and the averaged weights inside the fused optimizer step (`Trainer(weight_decay=, decoupled_weight_decay=,
decay_filter=, ema_decay=, ema_warmup=)`) -- the launches of a trainer without the options, three steps against torch.optim.AdamW /
torch.optim.Adam(weight_decay=) on the oracle with an EMA kept by lerp_, the skipped step, `averaged()`, the two state dicts and
two ranks over gloo.  dlsg_adamw_ema and dlsg_swap_f32 are emulated in torch (`DecayEmul`, below; tests/test_gpu_adamw_ema.py holds
the real ones against it)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dlsg_amd
from emul_ops import EmulOps
from test_grad_clip_host import ClipEmul, Oracle, small_net, check_weights, _free_port, NORM, COEF, NONFINITE
from test_scst_host import LengthReward

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_OPS = ('adamw_ema', 'swap')


def decay_mask(n, decay_ranges):
    """float mask over n elements: 1 inside one of the [lo, hi) intervals (None: everywhere)"""
    if decay_ranges is None:
        return torch.ones(n)
    mask = torch.zeros(n)
    for lo, hi in decay_ranges.tolist():
        mask[lo:hi] = 1.0
    return mask


class DecayEmul(ClipEmul):
    """ClipEmul + dlsg_adamw_ema / dlsg_swap_f32, in the order include/dlsg.h gives"""

    def adamw_ema(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, weight_decay=0.0, decoupled=True, ema=None, ema_decay=0.0,
                  hyper=None, record=None, clip_value=0.0, decay_ranges=None):
        if int(self._persist_word().item()) != 0:
            return
        coef = 1.0
        if record is not None:
            if float(record[NONFINITE]) != 0.0:
                return
            coef = record[COEF]
        gi = (g * grad_scale) * coef
        if clip_value > 0:
            gi = gi.clamp(-clip_value, clip_value)
        if hyper is not None:
            assert hyper.numel() == 4
            wdf, ew = float(hyper[2]), float(hyper[3])
        else:                                            # float64, rounded once: what the entry point does with its scalars
            wdf = float(np.float32(1.0 - float(np.float32(lr)) * float(np.float32(weight_decay)))) if decoupled else float(np.float32(weight_decay))
            ew = float(np.float32(1.0 - float(np.float32(ema_decay))))
        if weight_decay > 0:
            mask = decay_mask(p.numel(), decay_ranges).to(p.device)
            if decoupled:
                p.mul_(torch.where(mask > 0, torch.tensor(wdf), torch.tensor(1.0)))
            else:
                gi = gi + (wdf * p) * mask
        EmulOps.adam(self, p, gi, m, v, lr, b1, b2, eps, step, 1.0, hyper=None if hyper is None else hyper[:2])
        if ema is not None:
            ema.add_(ew * (p - ema))

    def swap(self, a, b):
        t = a.clone()
        a.copy_(b)
        b.copy_(t)


def ndim_filter(name, p):
    return p.ndim > 1


def ema_decay_at(d, t, warmup):
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


class DecayOracle(Oracle):
    """the oracle with torch.optim.AdamW, or torch.optim.Adam(weight_decay=) for L2, in torch's two-group idiom under a filter, and an
    EMA of its parameters kept with lerp_"""

    def __init__(self, args, vocab, sd, lr, wd, decoupled=True, filt=None, ema_decay=None, warmup=False):
        Oracle.__init__(self, args, vocab, sd, lr=lr)
        named = list(self.model.named_parameters())
        if filt is None:
            groups = [p for _, p in named]
        else:
            groups = [{'params': [p for n, p in named if filt(n, p)]},
                      {'params': [p for n, p in named if not filt(n, p)], 'weight_decay': 0}]
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        self.opt = cls(groups, lr=lr, betas=(0.5, 0.9), weight_decay=wd)
        self.d, self.warmup, self.t = ema_decay, warmup, 0
        self.ema = {n: p.detach().clone() for n, p in named}

    def step(self, *batch, **kw):
        loss = Oracle.step(self, *batch, **kw)
        self.t += 1
        if self.d is not None:
            w = 1.0 - ema_decay_at(self.d, self.t, self.warmup)
            for n, p in self.model.named_parameters():
                self.ema[n].lerp_(p.detach(), w)
        return loss


def arena_error(net, arena, ref):
    """check_weights' measure, as a number: max over parameters of |sum got - sum ref| / max(1, sum |ref|), got read from `arena`"""
    worst = 0.0
    for k, p in net.named_parameters():
        o = net._offsets[k]
        r = ref[k].detach().double()
        got = float(arena[o:o + p.numel()].double().sum())
        worst = max(worst, abs(got - float(r.sum())) / max(1.0, float(r.abs().sum())))
    return worst


def bits(t):
    return t.view(torch.int32)


def net_for(**kw):
    return small_net(emul=DecayEmul, **kw)


# ---------------------------------------------------------------- the default path
def test_default_path_issues_the_launches_it_issued_before():
    off = dict(weight_decay=0.0, decoupled_weight_decay=True, decay_filter=None, ema_decay=None, ema_warmup=False)
    for clip, name in (({}, 'adam'), ({'max_grad_norm': 1.0}, 'adam_clipped')):
        logs = []
        for kw in ({}, off, dict(off, decay_filter=ndim_filter, decoupled_weight_decay=False)):
            net, sd, args, vocab, frames, regions, caps, lens = net_for()
            tr = dlsg_amd.Trainer(net, lr=1e-3, **dict(clip, **kw))
            assert tr.ema is None
            net.ops.log = []
            for _ in range(2):
                tr.step(frames, regions, caps, lens, 1.0)
            logs.append(net.ops.log)
            net.ops.log = None
        assert logs[0] == logs[1] == logs[2]             # every launch, by name and argument signature
        names = [c[0] for c in logs[0]]
        assert names.count(name) == 2 * len(tr._train_ranges) and not set(names) & set(NEW_OPS)
    # and with an option on: the same launches up to the update, then adamw_ema in place of adam, one per trainable range
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    tr = dlsg_amd.Trainer(net, lr=1e-3, ema_decay=0.9)
    net.ops.log = []
    tr.step(frames, regions, caps, lens, 1.0)
    log, net.ops.log = net.ops.log, None
    net2 = net_for()[0]
    tr2 = dlsg_amd.Trainer(net2, lr=1e-3)
    net2.ops.log = []
    tr2.step(frames, regions, caps, lens, 1.0)
    one, net2.ops.log = net2.ops.log, None
    cut = [c[0] for c in one].index('adam')
    assert log[:cut] == one[:cut]
    assert [c[0] for c in log[cut:]] == ['adamw_ema'] * len(tr._train_ranges)


def test_validation_errors():
    net = net_for()[0]
    for kw in (dict(weight_decay=-1e-3), dict(weight_decay=float('nan')), dict(ema_decay=0.0), dict(ema_decay=1.0),
               dict(ema_decay=-0.5), dict(ema_decay=1.5), dict(ema_warmup=True), dict(decay_filter='bias')):
        with pytest.raises(ValueError):
            dlsg_amd.Trainer(net, **kw)
    with pytest.raises(ValueError):
        dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, ema_warmup=True)
    tr = dlsg_amd.Trainer(net)
    for call in (tr.ema_state_dict, lambda: tr.load_ema_state_dict({}), lambda: tr.averaged().__enter__()):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------- against torch on the oracle
LR, WD, D = 1e-3, 0.5, 0.9         # lr * wd = 5e-4 a step: three steps of decay are 15 times the 1e-4 bound on a LayerNorm gain


@pytest.mark.parametrize('decoupled, filt, warmup', [(True, None, False), (True, ndim_filter, True), (False, None, True),
                                                     (False, ndim_filter, False)])
def test_three_steps_match_torch_adamw_or_adam_l2_and_a_lerp_ema(decoupled, filt, warmup):
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    orc = DecayOracle(args, vocab, sd, LR, WD, decoupled, filt, D, warmup)
    plain = DecayOracle(args, vocab, sd, LR, 0.0, decoupled, None, D, warmup)              # the same, without decay
    tr = dlsg_amd.Trainer(net, lr=LR, weight_decay=WD, decoupled_weight_decay=decoupled, decay_filter=filt, ema_decay=D,
                          ema_warmup=warmup)
    assert torch.equal(tr.ema, net._flat) and tr.ema.data_ptr() != net._flat.data_ptr()
    unused = {k: p.detach().clone() for k, p in net.named_parameters() if k in net.unused_parameters}
    assert unused
    for step in range(3):
        want_loss = orc.step(frames, regions, caps, lens)
        plain.step(frames, regions, caps, lens)
        loss = tr.step(frames, regions, caps, lens, 1.0)
        ew, ee = arena_error(net, net._flat, dict(orc.model.named_parameters())), arena_error(net, tr.ema, orc.ema)
        print('step %d: loss %.9g oracle %.9g; weights %.3g, ema %.3g (bound 1e-4)' % (step + 1, float(loss), float(want_loss), ew, ee))
        assert abs(float(loss) - float(want_loss)) <= 1e-4
        check_weights(net, orc, 1e-4)
        assert ew <= 1e-4 and ee <= 1e-4
    # an unused parameter keeps its bits under decay, in the weights and in the average
    for k, p0 in unused.items():
        o = net._offsets[k]
        assert torch.equal(bits(dict(net.named_parameters())[k].detach()), bits(p0))
        assert torch.equal(bits(tr.ema[o:o + p0.numel()]), bits(p0.view(-1)))
    # the decay and the average took part: element by element the oracle without decay is far off, the oracle itself is not, and
    # the weights are no "average"
    def far(ref):
        return max(float((p.detach() - ref[k].detach()).abs().max()) for k, p in net.named_parameters())
    d_orc, d_plain, d_ema = far(dict(orc.model.named_parameters())), far(dict(plain.model.named_parameters())), far(orc.ema)
    print('max |dw| against the oracle %.3g, against the oracle without decay %.3g, against the oracle\'s average %.3g'
          % (d_orc, d_plain, d_ema))
    # (three steps of decay move an element by about 3 * lr * wd * |p| = 1.5e-3 |p|; an Adam step moves it by about lr = 1e-3, of which
    #  the average lags a share)
    assert d_plain > 1e-3 and d_plain > 10 * d_orc and d_ema > 1e-4


@pytest.mark.parametrize('filt', [None, ndim_filter])
def test_decay_tables_cover_exactly_the_chosen_used_trainable_elements(filt):
    net = net_for()[0]
    frozen = next(n for n, p in net.named_parameters() if p.ndim > 1 and n.startswith('decoder.'))
    dict(net.named_parameters())[frozen].requires_grad_(False)
    tr = dlsg_amd.Trainer(net, weight_decay=0.1, decay_filter=filt)
    want = torch.zeros(net._flat.numel())
    for n, p in net.named_parameters():
        if (filt is None or filt(n, p)) and n not in net.unused_parameters and n != frozen:
            want[net._offsets[n]:net._offsets[n] + p.numel()] = 1.0
    got = torch.zeros_like(want)
    assert sorted(tr._decay_tabs) == sorted(tr._train_ranges) and len(tr._train_ranges) >= 2
    for (lo, hi), (wd, tab) in tr._decay_tabs.items():
        if wd == 0.0:
            assert tab is None
            continue
        assert wd == 0.1
        if tab is not None:
            t = tab.tolist()
            assert tab.dtype == torch.int64 and all(0 <= a < b <= hi - lo for a, b in t)
            assert all(t[i][1] < t[i + 1][0] for i in range(len(t) - 1))            # sorted, disjoint, joined where they touch
        got[lo:hi] = decay_mask(hi - lo, tab)
    pad = torch.ones_like(want)                          # (the padding between parameters holds zeros: either way is right)
    for n, p in net.named_parameters():
        pad[net._offsets[n]:net._offsets[n] + p.numel()] = 0.0
    assert torch.equal(got * (1 - pad), want) and float(want.sum()) > 0
    if filt is not None:
        assert any(tab is not None and len(tab) > 1 for _, tab in tr._decay_tabs.values())


def test_non_finite_gradient_skips_the_step_and_leaves_the_average():
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    tr = dlsg_amd.Trainer(net, max_grad_norm=1.0, weight_decay=0.1, ema_decay=0.9, decay_filter=ndim_filter)
    start = net._flat.clone()
    tr.step(frames, regions, caps, lens, 1.0)
    assert int(tr.skipped_steps) == 0 and not torch.equal(tr.ema, start) and not torch.equal(tr.ema, net._flat)
    before = [t.clone() for t in (net._flat, tr.m, tr.v, tr.ema)]

    def poison(g):
        g[g.numel() // 2] = float('inf')
    net.ops.inject = poison
    tr.step(frames, regions, caps, lens, 1.0)
    for a, b in zip(before, (net._flat, tr.m, tr.v, tr.ema)):
        assert torch.equal(bits(a), bits(b))
    assert int(tr.skipped_steps) == 1 and tr.t == 2
    tr.step(frames, regions, caps, lens, 1.0)
    assert int(tr.skipped_steps) == 1 and not torch.equal(before[0], net._flat) and not torch.equal(before[3], tr.ema)
    assert bool(torch.isfinite(tr.ema).all())


# ---------------------------------------------------------------- using the average
def averaging_trainer(steps=2, **kw):
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    tr = dlsg_amd.Trainer(net, lr=1e-3, ema_decay=0.5, **kw)
    for _ in range(steps):
        tr.step(frames, regions, caps, lens, 1.0)
    return net, tr, (frames, regions, caps, lens)


def test_averaged_exchanges_the_arenas_and_puts_them_back():
    net, tr, batch = averaging_trainer()
    w0, e0 = net._flat.clone(), tr.ema.clone()
    assert not torch.equal(w0, e0)
    ptrs = (net._flat.data_ptr(), tr.ema.data_ptr())
    with tr.averaged() as m:
        assert m is net and torch.equal(bits(net._flat), bits(e0)) and torch.equal(bits(tr.ema), bits(w0))
        name, p = next(iter(net.named_parameters()))
        assert torch.equal(p.detach().view(-1), e0[net._offsets[name]:net._offsets[name] + p.numel()])    # the parameters are views
        with pytest.raises(RuntimeError):
            tr.step(*batch, 1.0)
        with pytest.raises(RuntimeError):
            tr.ema_state_dict()
        with pytest.raises(RuntimeError):
            with tr.averaged():
                pass
        assert torch.equal(bits(net._flat), bits(e0)) and tr.t == 2
    assert torch.equal(bits(net._flat), bits(w0)) and torch.equal(bits(tr.ema), bits(e0))
    with pytest.raises(KeyError):
        with tr.averaged():
            assert torch.equal(bits(net._flat), bits(e0))
            raise KeyError('inside')
    assert torch.equal(bits(net._flat), bits(w0)) and torch.equal(bits(tr.ema), bits(e0))
    assert (net._flat.data_ptr(), tr.ema.data_ptr()) == ptrs
    tr.step(*batch, 1.0)                                 # and the trainer goes on
    assert tr.t == 3 and not torch.equal(net._flat, w0)


def test_ema_state_dict_loads_into_a_deep_copy_and_round_trips():
    net, tr, batch = averaging_trainer()
    sd = tr.ema_state_dict()
    own = net.state_dict()
    assert list(sd) == list(own) and all(sd[k].shape == own[k].shape and sd[k].dtype == own[k].dtype for k in own)
    name = next(iter(dict(net.named_parameters())))
    sd[name].add_(1.0)                                   # clones: neither the average nor the weights move
    assert float((tr.ema_state_dict()[name] - sd[name]).abs().max()) == 1.0
    sd = tr.ema_state_dict()
    twin = copy.deepcopy(net).set_ops(DecayEmul())
    twin.load_state_dict(sd)
    twin.flatten_parameters_()
    assert twin._flat.data_ptr() != net._flat.data_ptr()
    for k, p in net.named_parameters():
        o = net._offsets[k]
        assert twin._offsets[k] == o and torch.equal(bits(twin._flat[o:o + p.numel()]), bits(tr.ema[o:o + p.numel()])), k
    assert not torch.equal(twin._flat, net._flat)
    # resume: a fresh trainer takes the average back
    net2 = net_for()[0]
    tr2 = dlsg_amd.Trainer(net2, lr=1e-3, ema_decay=0.5)
    tr2.load_ema_state_dict(sd)
    assert torch.equal(bits(tr2.ema), bits(tr.ema))
    with pytest.raises(KeyError):
        tr2.load_ema_state_dict({})


def test_the_average_survives_a_rebind_with_the_same_layout():
    net, tr, batch = averaging_trainer()
    e0, m0 = tr.ema.clone(), tr.m.clone()
    name, p = next((n, p) for n, p in net.named_parameters() if n.startswith('decoder.'))
    p.requires_grad_(False)
    tr.step(*batch, 1.0)                                 # the frozen set changed: _bind runs again
    o = net._offsets[name]
    assert torch.equal(bits(tr.ema[o:o + p.numel()]), bits(e0[o:o + p.numel()])) and torch.equal(tr.m[o:o + p.numel()], m0[o:o + p.numel()])
    assert not torch.equal(tr.ema, e0)


# ---------------------------------------------------------------- optimizer state dict
def assert_same_state(a, b):
    assert a['param_groups'] == b['param_groups'] and sorted(a['state']) == sorted(b['state'])
    for i in a['state']:
        for k in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(a['state'][i][k], b['state'][i][k]), (i, k)


@pytest.mark.parametrize('filt', [None, ndim_filter])
def test_optimizer_state_dict_round_trips(filt):
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    tr = dlsg_amd.Trainer(net, lr=1e-3, weight_decay=0.1, decay_filter=filt, decoupled_weight_decay=filt is None)
    for _ in range(2):
        tr.step(frames, regions, caps, lens, 1.0)
    osd = tr.optimizer_state_dict()
    n = len(list(net.named_parameters()))
    groups = osd['param_groups']
    if filt is None:
        assert len(groups) == 1 and groups[0]['weight_decay'] == 0.1 and groups[0]['decoupled_weight_decay'] is True
        assert groups[0]['params'] == list(range(n))
    else:
        k = sum(1 for _, p in net.named_parameters() if p.ndim > 1)
        assert [g['params'] for g in groups] == [list(range(k)), list(range(k, n))] and 0 < k < n
        assert [g['weight_decay'] for g in groups] == [0.1, 0] and groups[0]['decoupled_weight_decay'] is False
    net2 = net_for()[0]
    tr2 = dlsg_amd.Trainer(net2, decay_filter=filt)
    tr2.load_optimizer_state_dict(osd)
    assert (tr2.t, tr2.lr, tr2.weight_decay, tr2.decoupled_weight_decay) == (2, 1e-3, 0.1, filt is None)
    assert torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v)
    assert_same_state(tr2.optimizer_state_dict(), osd)
    # the loaded decay is applied: one more step on both gives the same bits
    net2.load_state_dict(net.state_dict())
    tr.step(frames, regions, caps, lens, 1.0)
    tr2.step(frames, regions, caps, lens, 1.0)
    assert torch.equal(bits(net2._flat), bits(net._flat))
    if filt is not None:
        with pytest.raises(ValueError):
            dlsg_amd.Trainer(net_for()[0]).load_optimizer_state_dict(osd)      # two groups need the filter that made them


def test_filtered_state_dict_loads_into_torch_adamw_and_one_further_step_agrees():
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    lr, wd = 1e-3, 0.1
    tr = dlsg_amd.Trainer(net, lr=lr, weight_decay=wd, decay_filter=ndim_filter)
    for _ in range(2):
        tr.step(frames, regions, caps, lens, 1.0)
    osd = tr.optimizer_state_dict()
    ref = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in net.named_parameters()]
    opt = torch.optim.AdamW([{'params': [p for n, p in ref if ndim_filter(n, p)]},
                             {'params': [p for n, p in ref if not ndim_filter(n, p)], 'weight_decay': 0}],
                            lr=lr, betas=(0.5, 0.9), weight_decay=wd)
    opt.load_state_dict(osd)
    assert [g['weight_decay'] for g in opt.param_groups] == [wd, 0]
    tr.step(frames, regions, caps, lens, 1.0)
    grads = net.grad_views()
    for n, p in ref:                                     # the gradient the trainer's third step applied (one rank: no scaling)
        p.grad = None if n in net.unused_parameters else grads[n].detach().clone()
    opt.step()
    worst = max(float((p.detach() - q.detach()).abs().max()) for (_, p), (_, q) in zip(ref, net.named_parameters()))
    print('third step, trainer against torch.optim.AdamW on the loaded state: max |dw| %.3g' % worst)
    assert worst <= 1e-6
    got = opt.state_dict()
    want = tr.optimizer_state_dict()
    assert sorted(got['state']) == sorted(want['state'])
    for i in got['state']:
        assert float(got['state'][i]['step']) == 3.0
        assert float((got['state'][i]['exp_avg'] - want['state'][i]['exp_avg']).abs().max()) <= 1e-6


def test_a_reference_layout_state_dict_still_loads():
    """one param group, decay 0: what torch.optim.Adam(model.parameters()) writes -- into a decaying, filtering trainer too"""
    net, sd, args, vocab, frames, regions, caps, lens = net_for()
    src = dlsg_amd.Trainer(net, lr=2e-4)
    src.step(frames, regions, caps, lens, 1.0)
    osd = src.optimizer_state_dict()
    assert len(osd['param_groups']) == 1 and osd['param_groups'][0]['weight_decay'] == 0
    assert osd['param_groups'][0]['decoupled_weight_decay'] is False
    for kw in ({}, dict(weight_decay=0.1, decay_filter=ndim_filter, ema_decay=0.9)):
        net2 = net_for()[0]
        tr = dlsg_amd.Trainer(net2, **kw)
        tr.load_optimizer_state_dict(osd)
        assert (tr.t, tr.lr, tr.weight_decay) == (1, 2e-4, 0.0)
        assert torch.equal(tr.m, src.m) and torch.equal(tr.v, src.v)
        net2.ops.log = []
        tr.step(frames, regions, caps, lens, 1.0)
        names, net2.ops.log = [c[0] for c in net2.ops.log], None
        assert ('adamw_ema' in names) == bool(kw) and ('adam' in names) != bool(kw)


def test_scst_trainer_forwards_the_keywords():
    net, sd, args, vocab, frames, regions, _, _ = net_for()
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, lr=1e-3, weight_decay=0.1, decay_filter=ndim_filter, ema_decay=0.5)
    start = net._flat.clone()
    assert torch.equal(tr.trainer.ema, start)
    tr.step(frames, regions, ['0', '1', '2'])
    assert not torch.equal(tr.trainer.ema, start) and not torch.equal(tr.trainer.ema, net._flat)
    with tr.trainer.averaged():
        assert not torch.equal(net._flat, start)


# ---------------------------------------------------------------- two ranks over gloo
def _build4():
    return net_for(seed=7, batch=4)


def _worker(rank, world, port, out_dir):
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    net, sd, args, vocab, frames, regions, caps, lens = _build4()
    sl = slice(rank * 2, rank * 2 + 2)
    tr = dlsg_amd.Trainer(net, world_size=world, lr=1e-3, weight_decay=0.1, decay_filter=ndim_filter, ema_decay=0.9, ema_warmup=True,
                          max_grad_norm=1.0)
    for _ in range(2):
        tr.step(frames[sl], regions[sl], caps[sl], lens[sl], 1.0)
    np.save(os.path.join(out_dir, 'flat%d.npy' % rank), net._flat.numpy())
    np.save(os.path.join(out_dir, 'ema%d.npy' % rank), tr.ema.numpy())
    dist.destroy_process_group()


def test_two_ranks_keep_bit_equal_weights_and_averages(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    f0, f1 = np.load(tmp_path / 'flat0.npy'), np.load(tmp_path / 'flat1.npy')
    e0, e1 = np.load(tmp_path / 'ema0.npy'), np.load(tmp_path / 'ema1.npy')
    assert np.array_equal(f0.view(np.int32), f1.view(np.int32)) and np.array_equal(e0.view(np.int32), e1.view(np.int32))
    start = _build4()[0]
    start.flatten_parameters_()
    assert not np.array_equal(e0, f0) and not np.array_equal(e0, start._flat.numpy()) and np.isfinite(e0).all()

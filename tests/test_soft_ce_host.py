"""CPU: label smoothing and ensemble word-level distillation in the train step (`Trainer(label_smoothing=, teacher=,
distill_weight=)`, `Ensemble.teacher_logits`) through the kernel emulation: the gradient arena of a step against torch autograd
on the oracle models with the soft target row restated in float64, the fixed point of a student distilled from its own copy, the
launch sequence with and without the options, what the step leaves of the teacher, and every refusal.  The new kernel is
emulated in tests/emul_soft_ce.py; tests/test_gpu_soft_ce.py holds the real one against the same restatement."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import dlsg_amd
from dlsg_amd.synth import synth_batch, synth_state_dict
from emul_ensemble import combined_logp
from emul_soft_ce import SoftCeEmul
from helpers import compare_grads, oracle_grads, small_args
from test_beam_nbest_host import MODELS
from test_ensemble_host import member_specs
from test_grad_clip_host import small_net
from test_scst_host import LengthReward

WEIGHTS = [0.5, 0.3, 0.2]
MODE_ID = {'prob': 0, 'logprob': 1}


def student(batch=3):
    return small_net(emul=SoftCeEmul, batch=batch)


def members(ops=None, oracles=False):
    """the three members of tests/test_ensemble_host.py's case -- two CapGnnModels of different hidden sizes and a CapBaseline1,
    vocabulary 50 -- on the emulated kernels, or their oracles"""
    vocab = dlsg_amd.make_vocab(50)
    out = []
    for kind, args, seed in member_specs():
        torch.manual_seed(0)
        net = MODELS[kind][0](args, vocab).eval()
        sd = synth_state_dict(net.state_dict(), seed)
        if oracles:
            net = MODELS[kind][1](args, vocab).eval()
        net.load_state_dict(sd)
        if not oracles:
            net.set_ops(SoftCeEmul() if ops is None else ops)
        out.append(net)
    return out


def batch_for(args, n):
    """3 clips and their 3 * n captions (a clip's lengths not sorted)"""
    frames, regions, caps, lens = synth_batch(args, 50, 3, 4)
    if n > 1:
        _, _, caps, lens = synth_batch(args, 50, 3 * n, 61)
        lens = torch.as_tensor(lens)[torch.randperm(3 * n, generator=torch.Generator().manual_seed(61))]
    return frames, regions, caps[:, :26].contiguous(), torch.as_tensor(lens)


def counted(caps, lens):
    L = caps.shape[1]
    return torch.arange(L).unsqueeze(0) < lens.clamp(max=L).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def teacher_oracle_rows(n):
    """the oracle members' teacher-forced logits on batch_for(n), as (B*n*L, V) rows (computed once, never modified)"""
    args = small_args(dropout=0.0)
    frames, regions, caps, lens = batch_for(args, n)
    with torch.no_grad():
        return tuple(o(frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0), caps, caps.shape[1], 1.0)[0].reshape(-1, 50)
                     for o in members(oracles=True))


def oracle_soft_grads(args, vocab, sd, frames, regions, caps, lens, n, eps, alpha=0.0, q=None):
    """autograd of -sum_j r_j log p_j / ntot over the counted rows on the oracle student -> {name: grad}"""
    from oracle import torch_ref as R
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    logits = orc(frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0), caps, caps.shape[1], 1.0)[0]
    V = logits.shape[-1]
    r = (1.0 - eps) * F.one_hot(caps, V).double() + eps / V
    if q is not None:
        r = (1.0 - alpha) * r + alpha * q.view(r.shape)
    valid = counted(caps, lens)
    loss = -(r * torch.log_softmax(logits.double(), -1))[valid].sum() / float(valid.sum())
    loss.backward()
    return float(loss.detach()), oracle_grads(orc)


# ---------------------------------------------------------------- 1. label smoothing
def test_label_smoothing_step_equals_torch_cross_entropy():
    from oracle import torch_ref as R
    net, sd, args, vocab, frames, regions, caps, lens = student()
    lens = torch.as_tensor(lens)
    tr = dlsg_amd.Trainer(net, lr=0.0, label_smoothing=0.1)
    loss = tr.step(frames, regions, caps, lens, 1.0)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    logits = orc(frames, regions, caps[:, :26], 26, 1.0)[0]
    valid = counted(caps[:, :26], lens)
    want = F.cross_entropy(logits[valid], caps[:, :26][valid], label_smoothing=0.1, reduction='sum') / float(valid.sum())
    want.backward()
    assert loss.shape == (1,) and abs(float(loss) - float(want.detach())) <= 1e-5
    compare_grads(net.grad_views(), oracle_grads(orc), 'emulated step, label_smoothing 0.1')
    parts = tr.last_loss_parts
    assert parts.shape == (3,) and float(parts[0]) == float(loss) and float(parts[2]) == 0.0
    # the NLL beside it is the loss of a plain step on the same weights
    net2 = student()[0]
    plain = dlsg_amd.Trainer(net2, lr=0.0).step(frames, regions, caps, lens, 1.0)
    assert abs(float(parts[1]) - float(plain)) <= 1e-6 and float(parts[0]) != float(parts[1])
    assert not torch.equal(net.grad_views()['decoder.word_restore.weight'], net2.grad_views()['decoder.word_restore.weight'])


# ---------------------------------------------------------------- 2. distillation
@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('alpha', [0.5, 1.0])
@pytest.mark.parametrize('mode', ['prob', 'logprob'])
def test_distillation_step_equals_autograd_of_the_soft_target(mode, alpha, eps, n):
    net, sd, args, vocab, _, _, _, _ = student()
    frames, regions, caps, lens = batch_for(args, n)
    teacher = dlsg_amd.Ensemble(members(), weights=WEIGHTS, mode=mode)
    tr = dlsg_amd.Trainer(net, lr=0.0, teacher=teacher, distill_weight=alpha, label_smoothing=eps)
    loss = tr.step(frames, regions, caps, lens, 1.0, seq_per_clip=n)
    c = combined_logp(list(teacher_oracle_rows(n)), WEIGHTS, MODE_ID[mode])
    q = c.exp() if mode == 'prob' else torch.softmax(c, 1)
    assert float((q.sum(1) - 1.0).abs().max()) <= 1e-12
    want_loss, want = oracle_soft_grads(args, vocab, sd, frames, regions, caps, lens, n, eps, alpha, q)
    assert abs(float(loss) - want_loss) <= 1e-5
    compare_grads(net.grad_views(), want, 'emulated step, %s, alpha %g, eps %g, n %d' % (mode, alpha, eps, n))
    # the three parts: mixed = (1 - alpha) * (smoothed CrossEntropy) + alpha * kd, and the plain NLL beside them
    mixed, nll, kd = [float(x) for x in tr.last_loss_parts]
    hard, _ = oracle_soft_grads(args, vocab, sd, frames, regions, caps, lens, n, eps)
    plain, _ = oracle_soft_grads(args, vocab, sd, frames, regions, caps, lens, n, 0.0)
    assert abs(mixed - ((1.0 - alpha) * hard + alpha * kd)) <= 1e-5 and abs(nll - plain) <= 1e-5 and kd > 0.0


def test_single_model_teacher_is_wrapped_as_an_ensemble():
    net = student()[0]
    tr = dlsg_amd.Trainer(net, lr=0.0, teacher=members()[0], distill_weight=0.5)
    assert isinstance(tr.teacher, dlsg_amd.Ensemble) and len(tr.teacher.members) == 1 and tr.teacher.weights == [1.0]


# ---------------------------------------------------------------- 3. fixed point
def test_student_distilled_from_its_own_copy_is_at_the_fixed_point():
    net, sd, args, vocab, frames, regions, caps, lens = student()
    lens = torch.as_tensor(lens)
    twin = copy.deepcopy(net).set_ops(SoftCeEmul())
    tr = dlsg_amd.Trainer(net, lr=0.0, teacher=twin, distill_weight=1.0)
    tr.step(frames, regions, caps, lens, 1.0)
    dlogits, _ = net.ops.last_soft
    assert float(dlogits.abs().max()) <= 1e-7                      # p == q up to rounding: (p - q) / ntot
    logits = tr.teacher.teacher_logits(frames, regions, caps[:, :26])[0].transpose(0, 1).double()
    lsm = torch.log_softmax(logits, -1)
    valid = counted(caps[:, :26], lens)
    entropy = float(-(lsm.exp() * lsm).sum(-1)[valid].sum() / float(valid.sum()))
    assert abs(float(tr.last_loss_parts[2]) - entropy) <= 1e-5 and abs(float(tr.last_loss_parts[0]) - entropy) <= 1e-5


# ---------------------------------------------------------------- 4. the launch log
def _names(ops, fn):
    ops.log = []
    fn()
    log, ops.log = ops.log, None
    return [c[0] for c in log]


def test_defaults_launch_what_they_launched_and_options_put_the_teacher_in_front():
    logs = []
    for kw in ({}, {'label_smoothing': 0.0, 'teacher': None, 'distill_weight': 0.0}):
        net, sd, args, vocab, frames, regions, caps, lens = student()
        tr = dlsg_amd.Trainer(net, lr=1e-3, **kw)
        assert tr.last_loss_parts is None
        net.ops.log = []
        for _ in range(2):
            tr.step(frames, regions, caps, lens, 1.0)
        logs.append(net.ops.log)
        net.ops.log = None
    assert logs[0] == logs[1]                                      # names and argument signatures
    plain = [c[0] for c in logs[0][:len(logs[0]) // 2]]
    assert plain.count('ce_ragged') == 1 and 'ce_ragged_soft' not in plain
    # with the options: one ops handle for the student and the members, so that one log holds every launch of the step
    net, sd, args, vocab, frames, regions, caps, lens = student()
    teacher = dlsg_amd.Ensemble(members(ops=net.ops), weights=WEIGHTS)
    forward = _names(net.ops, lambda: teacher.teacher_logits(frames, regions, caps[:, :26]))
    assert len(forward) > 100 and 'ce_ragged' not in forward
    tr = dlsg_amd.Trainer(net, lr=1e-3, teacher=teacher, distill_weight=0.5, label_smoothing=0.1)
    got = _names(net.ops, lambda: tr.step(frames, regions, caps, lens, 1.0))
    assert got == forward + ['ce_ragged_soft' if c == 'ce_ragged' else c for c in plain]
    # label smoothing alone: no teacher launches
    net, sd, args, vocab, frames, regions, caps, lens = student()
    tr = dlsg_amd.Trainer(net, lr=1e-3, label_smoothing=0.1)
    got = _names(net.ops, lambda: tr.step(frames, regions, caps, lens, 1.0))
    assert got == ['ce_ragged_soft' if c == 'ce_ragged' else c for c in plain]


# ---------------------------------------------------------------- 5. the teacher is left alone
def test_three_steps_leave_the_teacher_untouched():
    net, sd, args, vocab, frames, regions, caps, lens = student()
    mem = members()
    mem[1].train()
    teacher = dlsg_amd.Ensemble(mem, weights=WEIGHTS, mode='logprob')
    tr = dlsg_amd.Trainer(net, lr=1e-3, teacher=teacher, distill_weight=0.5)
    before = [{k: p.detach().clone() for k, p in m.named_parameters()} for m in mem]
    w0 = net._flat.clone()
    losses = [float(tr.step(frames, regions, caps, lens, 1.0)) for _ in range(3)]
    assert not torch.equal(w0, net._flat) and losses[2] < losses[0]
    assert [m.training for m in mem] == [False, True, False]
    for m, old in zip(mem, before):
        for k, p in m.named_parameters():
            assert torch.equal(p.detach(), old[k]) and p.grad is None, k
        assert m._gflat is None or float(m._gflat.abs().max()) == 0.0


def test_teacher_logits_run_without_dropout_whatever_the_training_flag():
    args, vocab = small_args(dropout=0.3), dlsg_amd.make_vocab(50)
    for kind in ('capgnn', 'baseline1'):
        torch.manual_seed(0)
        m = MODELS[kind][0](args, vocab)
        m.load_state_dict(synth_state_dict(m.state_dict(), 7))
        m.set_ops(SoftCeEmul()).train()
        for n in (1, 2):
            frames, regions, caps, lens = batch_for(args, n)
            got = dlsg_amd.Ensemble([m]).teacher_logits(frames, regions, caps, seq_per_clip=n)
            assert m.training and len(got) == 1 and got[0].shape == (26, 3 * n, 50) and not got[0].requires_grad
            m.eval()
            with torch.no_grad():
                want = m(frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0), caps, 26, 1.0)[0]
            m.train()
            assert float((got[0].transpose(0, 1) - want).abs().max()) <= 1e-5
        short = dlsg_amd.Ensemble([m]).teacher_logits(frames, regions, caps, max_words=9, seq_per_clip=2)[0]
        assert short.shape == (9, 6, 50)
        with pytest.raises(ValueError):
            dlsg_amd.Ensemble([m]).teacher_logits(frames, regions, caps[:5], seq_per_clip=2)
    # the ensemble still refuses to be called with captions
    with pytest.raises(ValueError):
        dlsg_amd.Ensemble([m])(frames, regions, caps)


# ---------------------------------------------------------------- 6. refusals
def test_bad_options_raise():
    net, sd, args, vocab, frames, regions, caps, lens = student()
    mem = members()
    for kw in ({'label_smoothing': -0.1}, {'label_smoothing': 1.0}, {'label_smoothing': float('nan')},
               {'distill_weight': -0.5, 'teacher': mem[0]}, {'distill_weight': 1.5, 'teacher': mem[0]},
               {'distill_weight': float('nan'), 'teacher': mem[0]},
               {'distill_weight': 0.5}, {'teacher': mem[0]}, {'teacher': dlsg_amd.Ensemble(mem), 'distill_weight': 0.0},
               {'teacher': net, 'distill_weight': 0.5}, {'teacher': dlsg_amd.Ensemble([mem[0], net]), 'distill_weight': 0.5}):
        with pytest.raises(ValueError):
            dlsg_amd.Trainer(net, **kw)
    # another vocabulary: another length, and the same length with two words swapped
    for other in (dlsg_amd.make_vocab(49), dlsg_amd.make_vocab(50)):
        if len(other) == 50:
            a, b = other.idx2word[7], other.idx2word[8]
            other.idx2word[7], other.idx2word[8] = b, a
            other.word2idx[a], other.word2idx[b] = 8, 7
        torch.manual_seed(0)
        alien = dlsg_amd.CapGnnModel(small_args(dropout=0.0), other).eval().set_ops(SoftCeEmul())
        with pytest.raises(ValueError, match='vocabulary'):
            dlsg_amd.Trainer(net, teacher=alien, distill_weight=0.5)
    # another device
    with pytest.raises(ValueError, match='the teacher is on'):
        dlsg_amd.Trainer(net, teacher=copy.deepcopy(mem[0]).to('meta'), distill_weight=0.5)
    # a policy gradient against a smoothed or a teacher's target row is not one
    for kw in ({'label_smoothing': 0.1}, {'teacher': mem[0], 'distill_weight': 0.5}, {'distill_weight': 0.5}):
        with pytest.raises(ValueError):
            dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, **kw)
    dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=2, label_smoothing=0.0, teacher=None, distill_weight=0.0)

"""CPU: minimum-risk training host logic -- the numpy emulation of the two launches (tests/emul_risk.py) against
`dlsg_amd.risk_loss_reference` under float64 autograd, the refusals of `Trainer.step(risk=...)` and `MRTTrainer`, the addon
headers (`abi.addons`: read, bound, documented), `MRTTrainer`'s host loop through an emulated ops object, and the launches of a
step without the keyword.  The GPU side is tests/test_gpu_risk.py."""
import os

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import abi
from emul_risk import RiskOps, emul_risk_grad, emul_risk_rows
from emul_sbs import SbsEmul
from test_scst_host import LengthReward, small_net
from test_seq_per_clip_host import SeqEmul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RiskEmul(RiskOps, SeqEmul, SbsEmul):
    """the emulated ops with seq_per_clip's kernels, both searches' steps and the two risk launches"""


def risk_case(L, B, n, V, seed=0, bad=False):
    """seeded logits (rows, L, V), targets, lens (1, L and above L among them), rewards, a mask with one candidate of clip 0 off (n > 2) and --
    from three clips on -- the last clip all off"""
    g = torch.Generator().manual_seed(seed)
    rows = B * n
    logits = torch.randn(rows, L, V, generator=g) * 2.0
    targets = torch.randint(0, V, (rows, L), generator=g)
    lens = torch.randint(1, L + 1, (rows,), generator=g)
    lens[0], lens[rows - 1] = 1, L
    if rows > 2:
        lens[1] = L + 3
    else:
        lens[0], lens[1] = L, L + 3  # two candidates: both of full length, so that neither's share underflows float32
    rewards = torch.rand(rows, generator=g, dtype=torch.float64) * 3.0
    mask = torch.ones(rows, dtype=torch.bool)
    if n > 2:
        mask[n - 1] = False
    if B >= 3:
        mask[(B - 1) * n:] = False
    if bad:
        targets[n, 0] = V            # clip 1, candidate 0, its first word
    return logits, targets, lens, rewards, mask


def emulate(logits, targets, lens, rewards, mask, n, tm, alpha, lp):
    x = logits.transpose(0, 1).contiguous() if tm else logits
    lse, tok = emul_risk_rows(x.numpy(), targets.numpy(), lens.numpy(), tm)
    out = emul_risk_grad(x.numpy(), targets.numpy(), lens.numpy(), lse, tok, rewards.numpy(), None if mask is None else mask.numpy(),
                         n, tm, alpha, lp)
    if tm:
        out['dlogits'] = np.swapaxes(out['dlogits'], 0, 1)
    return out, lse, tok


def reference(logits, targets, lens, rewards, mask, n, alpha, lp):
    x = logits.double().requires_grad_(True)
    loss, parts = dlsg_amd.risk_loss_reference(x, targets, lens, rewards, n, mask=mask, alpha=alpha, length_penalty=lp, return_parts=True)
    loss.backward()
    return float(loss.detach()), x.grad, parts


@pytest.mark.parametrize('tm', [False, True])
@pytest.mark.parametrize('L,B,n,V,alpha,lp', [(6, 3, 4, 37, 1.0, 1.0), (6, 3, 4, 37, 0.5, 0.0), (5, 2, 1, 11, 1.0, 1.0), (5, 2, 3, 11, 0.0, 0.7),
                                              (64, 1, 2, 13, 0.05, 0.0), (4, 1, 32, 9, 2.0, 0.5)])
def test_emulation_equals_reference_autograd(L, B, n, V, alpha, lp, tm):
    logits, targets, lens, rewards, mask = risk_case(L, B, n, V)
    out, lse, tok = emulate(logits, targets, lens, rewards, mask, n, tm, alpha, lp)
    loss, grad, parts = reference(logits, targets, lens, rewards, mask, n, alpha, lp)
    # float32 token terms (2^-24 relative, up to L of them) scaled by alpha in an exponent, a float32 weight and row: 1e-5 of the
    # largest value holds with room at these sizes; the device kernels' own bound is measured in tests/test_gpu_risk.py
    tol = 1e-5
    assert abs(float(out['stats'][0]) - loss) <= tol * max(1.0, abs(loss)) and out['stats'][3] == -out['stats'][0]
    assert np.allclose(out['Q'], parts['Q'].detach().numpy().reshape(-1), rtol=0, atol=tol)
    assert np.allclose(out['s'], parts['s'].detach().numpy().reshape(-1), rtol=tol, atol=tol)
    assert np.allclose(out['R'], parts['R'].detach().numpy(), rtol=0, atol=3 * tol)
    g = grad.numpy()
    assert np.abs(out['dlogits'] - g).max() <= tol * max(np.abs(g).max(), 1e-3)
    # the zero fill behind a caption's end, a masked candidate, a clip without a counted candidate
    live = np.arange(L)[None, :] < np.minimum(lens.numpy(), L)[:, None]
    assert not out['dlogits'][~live].any()
    off = ~mask.numpy()
    assert not out['dlogits'][off].any() and not out['Q'][off].any()
    if B >= 3:
        assert out['R'][B - 1] == 0.0
    if n == 1 or alpha == 0.0:
        assert not out['dlogits'].any() and not g.any()
    else:
        assert np.abs(g).max() > 0
    keep = mask.numpy() & (lens.numpy() >= 1)
    assert out['stats'][1] == pytest.approx(rewards.numpy()[keep].mean()) and \
        out['stats'][2] == pytest.approx(np.minimum(lens.numpy(), L)[keep].mean())


def test_emulation_bad_target_and_minus_inf():
    logits, targets, lens, rewards, mask = risk_case(6, 3, 4, 37, bad=True)
    mask[:] = True
    out, lse, tok = emulate(logits, targets, lens, rewards, mask, 4, False, 1.0, 1.0)
    assert np.isnan(out['stats'][0]) and np.isnan(out['loss']) and np.isnan(out['R'][1]) and np.isnan(out['dlogits'][4, 0]).all()
    assert np.isfinite(out['dlogits'][:4]).all() and np.isfinite(out['dlogits'][8:]).all() and np.isfinite(out['R'][[0, 2]]).all()
    # a candidate whose log-probability is -inf is not counted: Q = 0, a zero gradient, and the rest as if it were masked
    logits, targets, lens, rewards, mask = risk_case(6, 3, 4, 37)
    logits[5, 0, targets[5, 0]] = -float('inf')
    out, _, _ = emulate(logits, targets, lens, rewards, mask, 4, True, 1.0, 1.0)
    m2 = mask.clone()
    m2[5] = False
    loss, grad, parts = reference(logits, targets, lens, rewards, m2, 4, 1.0, 1.0)
    assert out['Q'][5] == 0.0 and not out['dlogits'][5].any() and out['s'][5] == -np.inf
    assert abs(float(out['stats'][0]) - loss) <= 1e-5 and np.abs(out['dlogits'] - grad.numpy()).max() <= 1e-5 * np.abs(grad.numpy()).max()
    loss2 = float(dlsg_amd.risk_loss_reference(logits, targets, lens, rewards, 4, mask=mask, alpha=1.0, length_penalty=1.0))
    assert loss2 == loss


def test_addon_headers_are_read_bound_and_documented():
    assert {'dlsg_risk_rows', 'dlsg_risk_grad'} <= set(abi.addons)
    assert len(abi.functions) == 130 and not set(abi.addons) & (set(abi.functions) | set(abi.extensions))
    import ctypes as C
    rt, at = abi.addons['dlsg_risk_grad']
    assert rt is C.c_int and at.count(C.c_double) == 2 and at[-1] is C.c_void_p
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        doc = f.read()
    assert 'dlsg_risk_rows' in doc and 'dlsg_risk_grad' in doc and 'include/addons/dlsg_risk.h' in doc
    with open(os.path.join(ROOT, 'd-lsg-video-caption_amd', 'csrc', 'Makefile')) as f:
        assert 'include/addons/*.h' in f.read()
    lib = os.path.join(ROOT, 'd-lsg-video-caption_amd', 'dlsg_amd', 'libdlsg_hip.so')
    if os.path.exists(lib):
        from dlsg_amd import hip
        bound = hip.load_library()
        assert bound.dlsg_risk_grad.argtypes == at and bound.dlsg_risk_rows.restype is C.c_int


def test_addon_headers_hold_new_prototypes_only(tmp_path):
    d = tmp_path / 'addons'
    d.mkdir()
    (d / 'b.h').write_text('/* c */\nint dlsg_two(const float* x, int n, void* stream);\n')
    (d / 'a.h').write_text('#ifndef A_H\n#define A_H\nint dlsg_one(int n);\n#endif\n')
    got = abi.read_addons(str(d), {'dlsg_gemm'})
    assert list(got) == ['dlsg_one', 'dlsg_two']
    (d / 'c.h').write_text('/* dlsg_gemm, in a comment\n of two lines */\nint dlsg_gemm(int n);\n')
    with pytest.raises(ValueError, match=r'c\.h line 3: dlsg_gemm'):
        abi.read_addons(str(d), {'dlsg_gemm'})
    (d / 'c.h').write_text('int dlsg_three(int n);\nint dlsg_one(int n);\n')
    with pytest.raises(ValueError, match=r'c\.h line 2: dlsg_one'):
        abi.read_addons(str(d), {'dlsg_gemm'})
    (d / 'c.h').write_text('int dlsg_three(int n);\n#define DLSG_X 3\n')
    with pytest.raises(ValueError, match=r'c\.h line 2: DLSG_X .*prototypes only'):
        abi.read_addons(str(d), set())
    (d / 'c.h').write_text('typedef struct { int a; } dlsg_s;\n')
    with pytest.raises(ValueError, match='prototypes only'):
        abi.read_addons(str(d), set())


def fixed_lists(n, L=7):
    """a candidate source: seeded words, distinct lengths, every candidate valid but clip 1's last"""
    def source(model, frames, regions, seed):
        B = frames.shape[0]
        g = torch.Generator().manual_seed(11)
        ids = torch.randint(4, 50, (B, n, L), generator=g)
        lens = torch.randint(2, L + 1, (B, n), generator=g)
        end = model.decoder.vocab('<end>')
        for b in range(B):
            for i in range(n):
                ids[b, i, int(lens[b, i]) - 1:] = end
        valid = torch.ones(B, n, dtype=torch.bool)
        valid[1, n - 1] = False
        return ids.to(frames.device), lens.to(frames.device), valid.to(frames.device)
    return source


def risk_net():
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    net.set_ops(RiskEmul())
    return net, sd, args, vocab, frames, regions, caps, lens


def test_trainer_step_refusals():
    net, sd, args, vocab, frames, regions, caps, lens = risk_net()
    net.train()
    tr = dlsg_amd.Trainer(net, lr=0.0)
    ok = dict(rewards=torch.ones(3, dtype=torch.float64), n=3, alpha=1.0)
    with pytest.raises(ValueError, match='risk with seq_weights'):
        tr.step(frames, regions, caps, lens, 1.0, seq_weights=torch.ones(3), risk=ok)
    with pytest.raises(ValueError, match='risk with extra_dlogits'):
        tr.step(frames, regions, caps, lens, 1.0, extra_dlogits=lambda lg, sv: lg, risk=ok)
    with pytest.raises(ValueError, match='risk with tf_ratio != 1'):
        tr.step(frames, regions, caps, lens, 0.8, risk=ok)
    with pytest.raises(ValueError, match='risk with label_smoothing'):
        dlsg_amd.Trainer(net, lr=0.0, label_smoothing=0.1).step(frames, regions, caps, lens, 1.0, risk=ok)
    for bad, what in ((dict(ok, n=2), 'n must be'), (dict(ok, n=33), 'n must be'), (dict(ok, n=0), 'n must be'),
                      (dict(ok, alpha=-1.0), 'alpha'), (dict(ok, alpha=float('nan')), 'alpha'), (dict(ok, length_penalty=float('inf')), 'alpha'),
                      (dict(ok, rewards=torch.ones(4, dtype=torch.float64)), 'rewards'), (dict(ok, rewards=[1.0, 1.0, 1.0]), 'rewards'),
                      (dict(ok, rewards=torch.ones(3, dtype=torch.int64)), 'rewards'), (dict(ok, mask=torch.ones(3)), 'mask'),
                      (dict(ok, beta=1.0), 'risk must be'), (dict(n=3, alpha=1.0), 'risk must be')):
        with pytest.raises(ValueError, match=what):
            tr.step(frames, regions, caps, lens, 1.0, risk=bad)
    assert tr.t == 0 and tr.last_risk is None
    teacher = small_net(seed=4)[0]
    with pytest.raises(ValueError, match='risk with teacher'):
        dlsg_amd.Trainer(net, lr=0.0, teacher=teacher, distill_weight=0.5).step(frames, regions, caps, lens, 1.0, risk=ok)


def test_mrt_trainer_refusals():
    net = risk_net()[0]
    rw = LengthReward()
    from dlsg_amd.ensemble import Ensemble
    with pytest.raises(ValueError, match='Ensemble'):
        dlsg_amd.MRTTrainer(Ensemble([net]), rw)
    with pytest.raises(ValueError, match='label_smoothing'):
        dlsg_amd.MRTTrainer(net, rw, label_smoothing=0.1)
    with pytest.raises(ValueError, match='label_smoothing / teacher'):
        dlsg_amd.MRTTrainer(net, rw, teacher=small_net(seed=4)[0], distill_weight=0.5)
    with pytest.raises(ValueError, match='counted twice'):
        dlsg_amd.MRTTrainer(net, rw, candidates='sample')
    with pytest.raises(ValueError, match='candidates must be'):
        dlsg_amd.MRTTrainer(net, rw, candidates='greedy')
    with pytest.raises(ValueError, match='n_candidates'):
        dlsg_amd.MRTTrainer(net, rw, n_candidates=33)
    with pytest.raises(ValueError, match='alpha'):
        dlsg_amd.MRTTrainer(net, rw, alpha=-0.5)
    with pytest.raises(ValueError, match='set by MRTTrainer'):
        dlsg_amd.MRTTrainer(net, rw, candidates='beam', candidate_options=dict(n_best=2))
    with pytest.raises(ValueError, match='callable takes its own'):
        dlsg_amd.MRTTrainer(net, rw, candidates=fixed_lists(3), candidate_options=dict(min_len=2))


@pytest.mark.parametrize('share', [False, True])
def test_mrt_host_loop_and_gradient_equals_oracle_autograd(share):
    """MRTTrainer on a callable's lists and a host reward through the emulated ops: what reaches Trainer.step, the statistics, and the
    whole gradient against autograd of risk_loss_reference on the oracle model's logits (small config, dropout 0)"""
    from oracle import torch_ref as R
    net, sd, args, vocab, frames, regions, _, _ = risk_net()
    n = 3
    tr = dlsg_amd.MRTTrainer(net, LengthReward(), n_candidates=n, candidates=fixed_lists(n), alpha=0.7, length_penalty=0.5,
                             share_encoder=share, lr=0.0)
    seen = []
    inner = tr.trainer.step
    tr.trainer.step = lambda *a, **k: seen.append((a, k)) or inner(*a, **k)
    net.ops.recording = []
    out = tr.step(frames, regions, ['0', '1', '2'])
    log, net.ops.recording = net.ops.recording, None
    assert log.count('risk_rows') == 1 and log.count('risk_grad') == 1 and not [c for c in log if c.startswith('ce_ragged')]
    assert log.index('risk_grad') == log.index('risk_rows') + 1
    (fx, rx, ids, lens, tf), kw = seen[0]
    assert tf == 1.0 and kw.get('seq_per_clip', 1) == (n if share else 1) and fx.shape[0] == (3 if share else 9)
    risk = kw['risk']
    vids = [str(b) for b in range(3) for _ in range(n)]
    r = LengthReward().scores(vids, [net.decoder.decode_tokens(x) for x in ids])
    assert np.array_equal(risk['rewards'].numpy(), r) and risk['n'] == n and (risk['alpha'], risk['length_penalty']) == (0.7, 0.5)
    keep = risk['mask'].numpy()
    assert keep.sum() == 8 and not keep[2 * n - 1]
    assert out['reward_mean'] == float(r[keep].mean()) and out['mean_len'] == float(lens.double().numpy()[keep].mean())
    assert float(out['expected_reward']) == -float(tr.trainer.last_risk['stats'][0])
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    L = ids.shape[1]
    ex = (lambda x: x.repeat_interleave(n, 0)) if share else (lambda x: x)
    logits = orc(ex(fx), ex(rx), ids, L, 1.0)[0]
    loss = dlsg_amd.risk_loss_reference(logits, ids, lens, risk['rewards'], n, mask=risk['mask'], alpha=0.7, length_penalty=0.5)
    loss.backward()
    assert abs(float(out['loss']) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
    assert torch.allclose(tr.trainer.last_risk['Q'].sum(1), torch.ones(3, dtype=torch.float64), atol=1e-12)
    G = net.grad_views()
    checked = 0
    for k, p in orc.named_parameters():
        if p.grad is None:
            continue
        err = float((G[k] - p.grad).abs().max())
        assert err <= 2e-5 + 2e-3 * float(p.grad.abs().max()), (k, err, float(p.grad.abs().max()))
        checked += 1
    assert checked > 20 and max(float(p.grad.abs().max()) for p in orc.parameters() if p.grad is not None) > 1e-4


def test_step_without_the_keyword_issues_the_same_launches():
    import random
    logs, res = [], []
    for kw in ({}, {'risk': None}):
        net, sd, args, vocab, frames, regions, caps, lens = risk_net()
        net.train()
        tr = dlsg_amd.Trainer(net, lr=1e-3)
        random.seed(3)
        net.ops.recording = []
        loss = tr.step(frames, regions, caps, lens, 1.0, **kw)
        logs.append(net.ops.recording)
        net.ops.recording = None
        res.append((float(loss), net._flat.clone(), net._gflat.clone()))
    assert logs[0] == logs[1] and logs[0].count('ce_ragged') == 1 and 'risk_rows' not in logs[0] and 'risk_grad' not in logs[0]
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    # with the keyword, the two launches stand where the CrossEntropy's stood and nothing else moves
    net, sd, args, vocab, frames, regions, caps, lens = risk_net()
    net.train()
    tr = dlsg_amd.Trainer(net, lr=1e-3)
    random.seed(3)
    net.ops.recording = []
    tr.step(frames, regions, caps, lens, 1.0, risk=dict(rewards=torch.tensor([1.0, 2.0, 4.0]), n=3, alpha=1.0))
    log, net.ops.recording = net.ops.recording, None
    plain = []
    for c in logs[0]:
        plain += ['risk_rows', 'risk_grad'] if c == 'ce_ragged' else [c]
    assert log == plain


@pytest.mark.parametrize('source', ['swor', 'beam'])
def test_mrt_searches_decode_in_eval_mode_and_feed_the_step(source):
    """the two searches as candidate sources: the lists are the model's own eval-mode search results, the mask is where their scores
    are finite, the train pass runs in the model's mode on a seed of its own"""
    net, sd, args, vocab, frames, regions, _, _ = risk_net()
    net.train()
    n = 3
    opts = dict(min_len=2) if source == 'swor' else dict(beam_size=4, length_penalty=0.5)
    tr = dlsg_amd.MRTTrainer(net, LengthReward(), n_candidates=n, candidates=source, candidate_options=opts, lr=0.0)
    seen = []
    inner = tr.trainer.step
    tr.trainer.step = lambda *a, **k: seen.append((a, k, net.training)) or inner(*a, **k)
    seed0 = net.seed_counter
    out = tr.step(frames, regions, ['0', '1', '2'])
    (fx, rx, ids, lens, tf), kw, training = seen[0]
    assert training and net.training and kw.get('seed') is None and net.seed_counter == seed0 + 2
    seed = (0x5DEECE66D * (seed0 + 1) + 0xB) & 0xFFFFFFFFFFFF
    net.eval()
    if source == 'swor':
        want_ids, score, want_lens = net.sample_without_replacement(frames, regions, n, 1.0, seed, **opts)
    else:
        want_ids, score, want_lens = net.beam_search(frames, regions, n_best=n, **opts)
    assert torch.equal(ids, want_ids.reshape(9, -1)) and torch.equal(lens, want_lens.reshape(-1))
    assert torch.equal(kw['risk']['mask'], torch.isfinite(score).reshape(-1)) and kw['risk']['mask'].any()
    assert torch.equal(fx, frames.repeat_interleave(n, 0))
    assert np.isfinite(float(out['loss'])) and float(out['expected_reward']) == -float(tr.trainer.last_risk['stats'][0])
    assert float(out['loss']) == float(np.float32(-float(out['expected_reward'])))

"""CPU: self-critical training (SCST) host logic -- CIDEr-D as a reward (`scoring.CiderD`), the sampled-decoding schedule
(`CapGnnModel.sample`), baselines and advantages (`SCSTTrainer`), the policy gradient against autograd on the oracle, and the
launch sequence of a Trainer step without the new keywords.  The two new kernels are emulated in numpy (`ScstEmul`, below);
the GPU side is tests/test_gpu_scst.py."""
import json
import os
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from emul_ops import EmulOps, _M32, _mix32
from helpers import small_args


def counter_hash(seed, site, idx):
    """numpy restatement of dlsg::counter_hash (csrc/common.hpp); idx uint64 ndarray"""
    idx = idx.astype(np.uint64)
    seed = np.uint64(seed)
    inner = ((idx >> np.uint64(32)) + (np.uint64(0x9e3779b9) * np.uint64(site) & _M32) + (seed & _M32)) & _M32
    h = _mix32((idx & _M32) ^ _mix32(inner))
    return _mix32(h ^ (seed >> np.uint64(32)))


def gumbel_keys(x, temperature, seed, site, row0):
    """x / temperature + g (float64), g = -log(-log u), u = ((h >> 8) + 1/2) 2^-24"""
    rows, V = x.shape
    idx = (np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(row0)) * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :]
    u = ((counter_hash(seed, site, idx) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    return x.double().numpy() / temperature - np.log(-np.log(u))


class ScstEmul(EmulOps):
    """EmulOps + the two new ops.  `recording` (a list) collects the name of every public op called while it is set."""

    recording = None

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        rec = object.__getattribute__(self, '__dict__').get('recording')
        if rec is not None and not name.startswith('_') and callable(v) and name != 'recording':
            def call(*a, **k):
                rec.append(name)
                return v(*a, **k)
            return call
        return v

    def sample_embed(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature=1.0, p=0.0, seed=0, site=0, site_sample=0,
                     row0=0):
        if torch.is_tensor(seed):
            seed = int(seed.item())
        if temperature > 0:
            ids = torch.from_numpy(gumbel_keys(logits, temperature, seed, site_sample, row0).argmax(1))
            z = logits.double() / temperature
        else:
            ids = logits.max(1)[1]
            z = logits.double()
        ids_out.copy_(ids)
        logp.copy_(torch.log_softmax(z, 1).gather(1, ids.view(-1, 1)).view(-1).float())
        hit = (ids == end_id) & (lens > t)
        lens.copy_(torch.where(hit, torch.full_like(lens, t + 1), lens))
        self.embed_fwd(E, ids, out, p=p, seed=seed, site=site, row0=row0)

    def ce_ragged_weighted(self, logits, targets, lens, weights, dlogits, row_loss, loss, time_major):
        self.ce_ragged(logits, targets, lens, dlogits, row_loss, loss, time_major)
        B = lens.shape[0]
        L = targets.shape[1]
        w = weights.view(1, B, 1) if time_major else weights.view(B, 1, 1)
        dlogits.mul_(w)
        rl = row_loss.view(L, B) if time_major else row_loss.view(B, L)
        rl.mul_(weights.view(1, B) if time_major else weights.view(B, 1))
        loss.copy_(row_loss.sum().reshape(1))


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scoring.json')


class LengthReward(object):
    """a deterministic stand-in for CIDEr-D with distinct values per caption: words + 0.1 * distinct words + clip index"""

    def scores(self, vids, hyps):
        return np.array([len(h.split()) + 0.1 * len(set(h.split())) + 0.01 * int(v) for v, h in zip(vids, hyps)], dtype=np.float64)


def small_net(seed=3, **kw):
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = small_args(dropout=0.0, **kw)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    net.set_ops(ScstEmul())
    net.update_beam_size(1)                      # net(frames, regions, None) is greedy decoding
    frames, regions, caps, lens = synth_batch(args, 50, 3, seed + 1)
    return net, sd, args, vocab, frames, regions, caps, lens


def test_ciderd_matches_reference_scorer_and_cider():
    for case in json.load(open(GOLD)):
        gts, res = case['gts'], case['res']
        ids = sorted(gts)
        got = S.CiderD(gts).scores(ids, [res[i][0] for i in ids])
        assert np.allclose(got, case['cider_per'], rtol=0, atol=1e-9)
    case = json.load(open(GOLD))[1]
    rng = random.Random(7)
    sub = sorted(rng.sample(sorted(case['gts']), 6))
    gts = {v: case['gts'][v] for v in sub}
    res = {v: case['res'][v] for v in sub}
    want = S.cider(gts, res)[1]
    scorer = S.CiderD(gts)
    assert np.allclose(scorer.scores(sub, [res[v][0] for v in sub]), want, rtol=0, atol=1e-12)
    # order, repeats and memoisation do not change a score
    got = scorer.scores(sub[::-1] + sub[:2], [res[v][0] for v in sub[::-1] + sub[:2]])
    assert np.allclose(got, list(want[::-1]) + list(want[:2]), rtol=0, atol=1e-12)


def test_sample_site_is_not_a_dropout_site():
    from dlsg_amd import engine as E
    sites = {E.SITE_PSL_OBJ, E.SITE_PSL_MOT, E.SITE_LSTM, E.SITE_PE, E.SITE_SA, E.SITE_WORD}
    sites |= {E.STEP_SITE * (t + 1) + k for t in range(64) for k in (E.SITE_QUERY, E.SITE_ATT1, E.SITE_ATT2, E.SITE_LANG)}
    assert E.SITE_SAMPLE not in sites


def test_sample_expansion_order_and_lengths():
    """temperature 0 is greedy: each of a clip's n rows is the clip's greedy caption; the rows of clip b are b*n .. b*n+n-1;
    lens is the first <end> position + 1 (else L); logp is the untempered log-softmax of the chosen word."""
    net, sd, args, vocab, frames, regions, _, _ = small_net()
    net.decoder.word_restore.bias.data[vocab('<end>')] += 1.2           # some captions end early
    with torch.no_grad():
        greedy = net(frames, regions, None)[0]
    n = 3
    ids, logp, lens = net.sample(frames, regions, n=n, temperature=0.0, seed=5)
    L = net.decoder.max_words
    assert ids.shape == (3 * n, L) and logp.shape == (3 * n, L) and lens.shape == (3 * n,)
    assert torch.equal(ids, greedy.repeat_interleave(n, 0))
    assert (logp <= 0).all()
    end = vocab('<end>')
    a, _, lens1 = net.sample(frames, regions, n=n, temperature=1.0, seed=11)
    for x, ln in ((ids, lens), (a, lens1)):
        for r in range(3 * n):
            hits = (x[r] == end).nonzero()
            assert int(ln[r]) == (int(hits[0]) + 1 if len(hits) else L)
        assert (ln < L).any() and (ln == L).any()
    # sampling (temperature 1): the draw depends on the seed only, every row is a different stream
    b = net.sample(frames, regions, n=n, temperature=1.0, seed=11)[0]
    c = net.sample(frames, regions, n=n, temperature=1.0, seed=12)[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a[0], a[1])


def test_other_models_do_not_sample():
    args, vocab = small_args(), dlsg_amd.make_vocab(50)
    for cls in (dlsg_amd.CapBaseline1, dlsg_amd.CapBaselineModel):
        with pytest.raises(NotImplementedError):
            cls(args, vocab).sample(torch.zeros(1, 26, 112), torch.zeros(1, 26, 16, 32))


def _spy(tr):
    """record the arguments of every Trainer.step call"""
    seen = []
    inner = tr.trainer.step

    def step(*a, **k):
        seen.append((a, k))
        return inner(*a, **k)
    tr.trainer.step = step
    return seen


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_baselines_and_advantages(baseline):
    net, sd, args, vocab, frames, regions, _, _ = small_net()
    n = 4
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=n, baseline=baseline, lr=0.0)
    seen = _spy(tr)
    seed0 = net.seed_counter
    out = tr.step(frames, regions, ['0', '1', '2'])
    (fx, rx, ids, lens, tf), kw = seen[0]
    assert tf == 1.0 and kw['seed'] == (0x5DEECE66D * (seed0 + 1) + 0xB) & 0xFFFFFFFFFFFF
    assert torch.equal(fx, frames.repeat_interleave(n, 0)) and torch.equal(rx, regions.repeat_interleave(n, 0))
    want_ids, _, want_lens = net.sample(frames, regions, n=n, seed=kw['seed'])
    assert torch.equal(ids, want_ids) and torch.equal(lens, want_lens)
    vids = [str(b) for b in range(3) for _ in range(n)]
    r = LengthReward().scores(vids, [net.decoder.decode_tokens(x) for x in ids])
    if baseline == 'mean':
        R = r.reshape(3, n)
        b = np.array([(R[i].sum() - R[i, j]) / (n - 1) for i in range(3) for j in range(n)])
    else:
        with torch.no_grad():
            g = net(frames, regions, None)[0]
        b = np.repeat(LengthReward().scores(['0', '1', '2'], [net.decoder.decode_tokens(x) for x in g]), n)
    assert np.array_equal(kw['seq_weights'].numpy(), (r - b).astype(np.float32))
    assert out['reward_mean'] == float(r.mean()) and out['baseline_mean'] == float(b.mean())
    assert out['mean_len'] == float(lens.double().mean())
    with pytest.raises(ValueError):
        dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=1, baseline='mean')


def test_scst_gradient_equals_oracle_autograd():
    """one SCST step's gradient == autograd of -sum_b A_b sum_{t<len_b} log p(w_bt) / sum_b len_b on the oracle model,
    teacher-forced on the sampled words (small config, dropout 0)."""
    from oracle import torch_ref as R
    net, sd, args, vocab, frames, regions, _, _ = small_net()
    n = 3
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=n, lr=0.0)
    seen = _spy(tr)
    tr.step(frames, regions, ['0', '1', '2'])
    (fx, rx, ids, lens, _), kw = seen[0]
    A = kw['seq_weights']
    assert float(A.abs().max()) > 0
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    L = ids.shape[1]
    logits = orc(fx, rx, ids, L, 1.0)[0]
    lp = torch.log_softmax(logits, -1).gather(2, ids.unsqueeze(2)).squeeze(2)
    valid = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).float()
    loss = -(A.unsqueeze(1) * lp * valid).sum() / lens.sum()
    loss.backward()
    G = net.grad_views()
    checked = 0
    for k, p in orc.named_parameters():
        if p.grad is None:
            continue
        ref, got = p.grad, G[k]
        err = float((got - ref).abs().max())
        assert err <= 2e-5 + 2e-3 * float(ref.abs().max()), (k, err, float(ref.abs().max()))
        checked += 1
    assert checked > 20


def test_trainer_step_without_new_keywords_issues_the_same_launches():
    logs, grads = [], []
    for kw in ({}, {'seed': None, 'seq_weights': None}):
        net, sd, args, vocab, frames, regions, caps, lens = small_net()
        net.train()
        tr = dlsg_amd.Trainer(net, lr=1e-3)
        random.seed(3)
        net.ops.recording = []
        loss = tr.step(frames, regions, caps, lens, 0.8, **kw)
        logs.append(net.ops.recording)
        net.ops.recording = None
        grads.append((float(loss), net._flat.clone(), net._gflat.clone()))
    assert logs[0] == logs[1] and 'ce_ragged' in logs[0] and 'ce_ragged_weighted' not in logs[0]
    assert grads[0][0] == grads[1][0] and torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][2], grads[1][2])
    # with weights, the one difference is the loss launch; weights of 1 give the same loss and gradients
    net, sd, args, vocab, frames, regions, caps, lens = small_net()
    net.train()
    tr = dlsg_amd.Trainer(net, lr=1e-3)
    random.seed(3)
    net.ops.recording = []
    loss = tr.step(frames, regions, caps, lens, 0.8, seq_weights=torch.ones(3))
    log = net.ops.recording
    net.ops.recording = None
    assert [('ce_ragged' if c == 'ce_ragged_weighted' else c) for c in log if c != 'ce_ragged'] == logs[0] or \
        log == [('ce_ragged_weighted' if c == 'ce_ragged' else c) for c in logs[0]]
    assert abs(float(loss) - grads[0][0]) <= 1e-7 and torch.allclose(net._gflat, grads[0][2], atol=1e-8)

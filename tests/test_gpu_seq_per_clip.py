"""GPU: several captions per clip on one encoder pass -- the two kernels (`dlsg_rows_repeat`, `dlsg_clip_fold`) against torch
and a float64 reference, the model and the Trainer step with seq_per_clip against the oracle on repeated clips, on-policy
log-probabilities of the shared sampler, graphs against eager, the device-reward step without host transfer, and a small run
in which shared SCST raises CIDEr-D.  The CPU side is tests/test_seq_per_clip_host.py."""
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.hip import HipOps
from dlsg_amd.synth import synth_batch
from helpers import compare_grads, load_case, small_args, weights_and_inputs
from test_gpu_scst import gpu_net
from test_scst_host import LengthReward
from test_seq_per_clip_host import captions_for, oracle_step_grads

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    return HipOps()


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize('row', [8 * 64, 5 * 70, 7])           # 350 and 7 are no multiples of 4: the scalar path
@pytest.mark.parametrize('n', [1, 2, 5])
@pytest.mark.parametrize('B', [1, 3])
def test_rows_repeat(ops, B, n, row):
    g = torch.Generator().manual_seed(1000 * B + 10 * n + row)
    x = torch.randn(B, row, generator=g).to(DEV)
    guard = 64
    buf = torch.full((B * n * row + 2 * guard,), 7.5, device=DEV)          # nothing outside y may be written
    y = buf[guard:guard + B * n * row].view(B * n, row)
    ops.rows_repeat(x, y, n)
    torch.cuda.synchronize()
    assert torch.equal(y, x.repeat_interleave(n, 0))
    assert bool((buf[:guard] == 7.5).all()) and bool((buf[-guard:] == 7.5).all())
    # a 3-d operand (the proposals), and a base that is 4- but not 16-byte aligned (scalar path whatever the width)
    if row % 8 == 0:
        x3 = x.view(B, 8, row // 8)
        y3 = torch.empty(B * n, 8, row // 8, device=DEV)
        ops.rows_repeat(x3, y3, n)
        xo = torch.empty(B * row + 1, device=DEV)[1:].view(B, row).copy_(x)
        yo = torch.zeros(B * n * row + 1, device=DEV)[1:].view(B * n, row)
        ops.rows_repeat(xo, yo, n)
        torch.cuda.synchronize()
        assert torch.equal(y3.view(B * n, row), y) and torch.equal(yo, y)


@pytest.mark.parametrize('accum', [0, 1])
@pytest.mark.parametrize('with_dg', [None, 'half', 'odd'])
@pytest.mark.parametrize('P,H', [(8, 64), (5, 70), (1, 1024)])
@pytest.mark.parametrize('n', [1, 2, 5])
@pytest.mark.parametrize('B', [1, 3])
def test_clip_fold(ops, B, n, P, H, with_dg, accum):
    """against float64: |err| <= (n + 2) 2^-24 sum|terms| per element -- n + 1 float32 additions (a row's two terms, the n - 1
    rows, the old value) plus the division, each within half an ulp of a partial sum bounded by sum|terms|"""
    g = torch.Generator().manual_seed(B * 7919 + n * 101 + P * 13 + H + 2 * len(with_dg or '') + accum)
    dmem = torch.randn(B * n, P, H, generator=g).to(DEV)
    # dg is a column slice of a wider tensor: the second half of (B*n, 2H) as the model passes it (16-byte accesses where H
    # allows), or columns H+2 .. 2H+2 of (B*n, 2H+6) -- a leading dimension and an offset that are no multiples of 4 floats
    wide = torch.randn(B * n, 2 * H + 6, generator=g).to(DEV)
    dg = {None: None, 'half': wide[:, :2 * H].clone(memory_format=torch.contiguous_format)[:, H:], 'odd': wide[:, H + 2:2 * H + 2]}[with_dg]
    assert dg is None or dg.shape == (B * n, H) and (B * n == 1 or dg.stride(0) == {'half': 2 * H, 'odd': 2 * H + 6}[with_dg])
    old = torch.randn(B, P, H, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        dx = old.clone()
        ops.clip_fold(dmem, dg, dx, n, accum=bool(accum))
        outs.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])                         # two launches, identical bits
    terms = dmem.double().view(B, n, P, H)
    mag = terms.abs().sum(1)
    ref = terms.sum(1)
    if dg is not None:
        t = (dg.double() / P).view(B, n, 1, H)
        ref = ref + t.sum(1)
        mag = mag + t.abs().sum(1)
    if accum:
        ref = ref + old.double()
        mag = mag + old.double().abs()
    err = (outs[0].double() - ref).abs()
    bound = (n + 2) * 2.0 ** -24 * mag
    worst = float((err / bound).max())
    print('clip_fold B=%d n=%d P=%d H=%d dg=%s accum=%d: worst error / bound %.3f' % (B, n, P, H, with_dg, accum, worst))
    assert bool((err <= bound).all()), worst
    if n == 1 and dg is None and not accum:
        assert torch.equal(outs[0], dmem)


# ---------------------------------------------------------------- the model against the oracle
def case_net(tag):
    args, vocab, g, kind = load_case(tag)
    args.dropout = 0.0
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd, frames, regions, _, _ = weights_and_inputs(net, g, args)
    net.load_state_dict(sd)
    net = net.to(DEV)
    net.update_beam_size(1)
    return net, sd, args, vocab, frames, regions


@pytest.mark.parametrize('tag,clips,n', [('small_msvd', 3, 3), ('small_msrvtt', 2, 5), ('small_noobj', 2, 2), ('full_msvd_b2', 2, 2)])
def test_model_and_step_equal_oracle_on_repeated_clips(tag, clips, n):
    net, sd, args, vocab, frames, regions = case_net(tag)
    assert frames.shape[0] >= clips
    frames, regions = frames[:clips].contiguous(), regions[:clips].contiguous()
    if tag == 'small_msrvtt':
        assert args.num_proposals == 5 and args.num_obj == 6
    caps, lens = captions_for(args, vocab, clips * n, 51)
    L = caps.shape[1]
    fd, rd, cd = frames.to(DEV), regions.to(DEV), caps.to(DEV)
    with torch.no_grad():
        logits, obj, mot, alpha = net(fd, rd, cd, L, 1.0, seq_per_clip=n)
    want_logits, want = oracle_step_grads(args, vocab, sd, frames, regions, caps, lens, n)
    torch.cuda.synchronize()
    assert logits.shape == want_logits.shape and obj.shape[0] == clips and mot.shape[0] == clips and alpha.shape[0] == clips * n
    err = float((logits.cpu() - want_logits).abs().max())
    print('%s %d x %d: max logit error %.3g' % (tag, clips, n, err))
    assert err <= 1e-3, err
    tr = dlsg_amd.Trainer(net, lr=0.0)
    tr.step(fd, rd, cd, lens, 1.0, seq_per_clip=n)
    torch.cuda.synchronize()
    compare_grads(net.grad_views(), want, '%s, %d clips x %d captions' % (tag, clips, n))


@pytest.mark.parametrize('msvd', [False, True], ids=['small_3x5', 'msvd_4x5'])
def test_shared_sampler_logp_is_on_policy(msvd):
    """train mode: the shared sampler's log-probabilities equal log_softmax of the teacher-forced train forward with
    seq_per_clip over the sampled words under the same seed (the encoder's masks keyed by clip, the decoder's by caption row)"""
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True, msvd=msvd, n_batch=4 if msvd else 3)
    n = 5
    c0 = net.seed_counter
    ids, logp, lens = net.sample(frames, regions, n=n, share_encoder=True)
    net.seed_counter = c0                               # the forward below draws the same seed
    L = ids.shape[1]
    with torch.no_grad():
        logits = net(frames, regions, ids, L, 1.0, seq_per_clip=n)[0]
    lp = torch.log_softmax(logits.double(), -1).gather(2, ids.unsqueeze(2)).squeeze(2)
    valid = torch.arange(L, device=DEV).unsqueeze(0) < lens.unsqueeze(1)
    err = (lp - logp.double()).abs()[valid].max().item()
    print('on-policy error %.3g' % err)
    assert err <= 2e-4, err
    # a clip's samples differ (their decoder masks and draws are keyed by the caption row)
    assert not torch.equal(ids[0], ids[1])


# ---------------------------------------------------------------- graphs against eager
def test_shared_sample_graph_replay_equals_eager():
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    sg = dlsg_amd.SampleGraph(net, frames, regions, n=4, temperature=1.0, share_encoder=True)
    for s in (21, 22, 5):
        got = [x.clone() for x in sg(frames, regions, s)]
        want = net.sample(frames, regions, n=4, seed=s, share_encoder=True)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(got, want)), s
    other = net.sample(frames, regions, n=4, seed=5)
    torch.cuda.synchronize()
    assert got[0].shape == other[0].shape


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_shared_scst_graphs_equal_eager(baseline):
    """the criteria of test_gpu_scst.test_scst_graphs_equal_eager, for SCSTTrainer(share_encoder=True)"""
    for lr in (0.0, 1e-3):
        res = []
        for graphs in (True, False):
            net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
            tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=4, baseline=baseline, lr=lr, use_graphs=graphs,
                                      device_coins=True, share_encoder=True)
            seen = []
            inner = tr.trainer.step
            tr.trainer.step = lambda *a, **k: seen.append((a[2].clone(), k['seq_weights'].clone(), a[0].shape[0], k['seq_per_clip'])) \
                or inner(*a, **k)
            random.seed(1)
            outs = [tr.step(frames, regions, ['0', '1', '2']) for _ in range(3)]
            torch.cuda.synchronize()
            if graphs:
                st = tr.trainer.static_inputs()
                assert st[0].shape[0] == 3 and st[1].shape[0] == 3 and st[2].shape[0] == 12 and st[3].shape[0] == 12
            res.append(([float(o['loss']) for o in outs], seen, net._flat.clone(), net._gflat.clone(), tr.trainer.m.clone(),
                        tr.trainer.v.clone()))
        (l0, s0, f0, g0, m0, v0), (l1, s1, f1, g1, m1, v1) = res
        assert all(a[2] == 3 and a[3] == 4 for a in s0 + s1)
        if lr == 0.0:
            assert l0 == l1
            assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(s0, s1))
            assert torch.equal(g0, g1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(f0, f1)
        else:
            assert (f0 - f1).abs().max().item() <= 3e-5


def test_shared_device_reward_step_makes_no_host_transfer():
    from test_gpu_cider_device import no_host_sync, scst_corpus
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    reward = S.CiderD(scst_corpus(vocab)).to_device(vocab)
    tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, baseline='greedy', lr=1e-3, use_graphs=True, check_every=0, share_encoder=True)
    vids = ['0', '1', '2']
    for _ in range(2):
        tr.step(frames, regions, vids)                      # captures
    torch.cuda.synchronize()
    with no_host_sync():
        out = tr.step(frames, regions, vids)
    torch.cuda.synchronize()
    assert all(torch.is_tensor(out[k]) and out[k].is_cuda and out[k].dim() == 0 for k in ('reward_mean', 'baseline_mean', 'mean_len'))
    assert np.isfinite(float(out['loss'])) and float(out['mean_len']) >= 1.0


# ---------------------------------------------------------------- training still works
def shared_learning_run(device, ce_steps=30, scst_steps=40, lr=1e-4, baseline='mean'):
    """the recipe of test_gpu_scst.learning_run -- 8 clips, 3 fixed reference captions each, cross-entropy steps on the first
    reference, then SCST steps rewarded with the corpus's CIDEr-D -- with SCSTTrainer(share_encoder=True)"""
    args = small_args(train_batch_size=8)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    random.seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).to(device).train()
    net.update_beam_size(1)
    g = torch.Generator().manual_seed(17)
    frames, regions, _, _ = synth_batch(args, 50, 8, 17)
    frames, regions = frames.to(device), regions.to(device)
    words = list(range(4, 50))
    refs, caps, lens = {}, [], []
    for b in range(8):
        pool = [words[i] for i in torch.randperm(len(words), generator=g)[:6].tolist()]
        sents = [[pool[(i * (k + 1) + k) % len(pool)] for i in range(4 + k)] for k in range(3)]
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
    scst = dlsg_amd.SCSTTrainer(net, reward, n_samples=5, baseline=baseline, lr=lr, share_encoder=True)
    for _ in range(scst_steps):
        scst.step(frames, regions, vids)
    return before, greedy_cider()


def test_shared_scst_raises_greedy_cider():
    before, after = shared_learning_run(DEV)
    print('greedy CIDEr-D before / after shared SCST: %.4f / %.4f' % (before, after))
    assert after > before, (before, after)

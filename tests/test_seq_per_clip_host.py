"""CPU: several captions per clip on one encoder pass (`seq_per_clip` / `share_encoder` / `captions_per_clip`) -- the host
logic through the kernel emulation: gradients of a Trainer step against oracle autograd on the clips repeated n times, the
launch sequence of the default forms, the row counts `forward` returns and refuses, two gloo ranks against one process, and the
clip-wise loader.  The two new kernels are emulated in torch (`SeqEmul`, below); the GPU side is tests/test_gpu_seq_per_clip.py."""
import os
import pickle
import random
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dlsg_amd
from dlsg_amd import data as D
from helpers import compare_grads, load_case, oracle_grads, small_args, weights_and_inputs
from test_scst_host import LengthReward, ScstEmul

HERE = os.path.dirname(os.path.abspath(__file__))


class SeqEmul(ScstEmul):
    """ScstEmul + rows_repeat / clip_fold (the kernels' order of additions: a row's two terms first, then the rows i = 0..n-1)"""

    def rows_repeat(self, x, y, n):
        self._count('rows_repeat')
        assert y.shape[0] == x.shape[0] * n and y.shape[1:] == x.shape[1:]
        y.copy_(x.repeat_interleave(n, 0))

    def clip_fold(self, dmem, dg, dx, n, accum=False):
        self._count('clip_fold')
        B, P, H = dx.shape
        assert dmem.shape == (B * n, P, H) and (dg is None or dg.shape == (B * n, H))
        t = dmem.view(B, n, P, H)
        if dg is not None:
            t = t + (dg / float(P)).view(B, n, 1, H)
        s = t[:, 0].clone()
        for i in range(1, n):
            s += t[:, i]
        dx.copy_(dx + s if accum else s)


def case_net(tag='small_msvd', dropout=0.0):
    """the fixture's config and seeded weights on the emulated kernels, its clips, and n captions per clip drawn with the
    fixture's seed"""
    args, vocab, g, kind = load_case(tag)
    args.dropout = dropout
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd, frames, regions, _, _ = weights_and_inputs(net, g, args)
    net.load_state_dict(sd)
    net.set_ops(SeqEmul())
    net.update_beam_size(1)
    return net, sd, args, vocab, frames, regions


def captions_for(args, vocab, rows, seed):
    from dlsg_amd.synth import synth_batch
    _, _, caps, lens = synth_batch(args, len(vocab), rows, seed)
    return caps, lens[torch.randperm(rows, generator=torch.Generator().manual_seed(seed))]      # (a clip's lengths are not sorted)


def oracle_step_grads(args, vocab, sd, frames, regions, caps, lens, n, weights=None):
    """autograd of the ragged CrossEntropy on the oracle model over the clips repeated n times -> (logits, {name: grad})"""
    from oracle import torch_ref as R
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    L = caps.shape[1]
    logits = orc(frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0), caps, L, 1.0)[0]
    if weights is None:
        R.ragged_ce(logits, caps, lens).backward()
    else:
        lp = torch.log_softmax(logits, -1).gather(2, caps.unsqueeze(2)).squeeze(2)
        valid = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).float()
        (-(weights.unsqueeze(1) * lp * valid).sum() / lens.sum()).backward()
    return logits.detach(), oracle_grads(orc)


# ---------------------------------------------------------------- 1. gradients against the oracle
def test_step_gradient_equals_oracle_on_repeated_clips():
    n = 3
    net, sd, args, vocab, frames, regions = case_net('small_msvd')
    assert frames.shape[0] == 3
    caps, lens = captions_for(args, vocab, 3 * n, 41)
    tr = dlsg_amd.Trainer(net, lr=0.0)
    loss = tr.step(frames, regions, caps, lens, 1.0, seq_per_clip=n)
    assert net.ops.calls['rows_repeat'] == 2 and net.ops.calls['clip_fold'] == 2
    logits, want = oracle_step_grads(args, vocab, sd, frames, regions, caps, lens, n)
    from oracle import torch_ref as R
    assert abs(float(loss) - float(R.ragged_ce(logits, caps, lens))) <= 1e-5
    G = net.grad_views()
    checked = 0
    for k, ref in want.items():
        if ref is None:
            continue
        err = float((G[k] - ref).abs().max())
        assert err <= 2e-5 + 2e-3 * float(ref.abs().max()), (k, err, float(ref.abs().max()))
        checked += 1
    assert checked > 20
    compare_grads(G, want, 'emulated step, 3 clips x 3 captions')
    # and with per-caption weights (the self-critical form of the step)
    w = torch.linspace(-1.0, 1.5, 3 * n)
    tr.step(frames, regions, caps, lens, 1.0, seq_per_clip=n, seq_weights=w)
    _, want = oracle_step_grads(args, vocab, sd, frames, regions, caps, lens, n, weights=w)
    compare_grads(net.grad_views(), want, 'emulated weighted step, 3 clips x 3 captions')


def test_autograd_bridge_folds_caption_rows_and_adds_proposal_gradients():
    """loss.backward() through forward(seq_per_clip=n), with a term on the B-row proposals as well"""
    from oracle import torch_ref as R
    n = 2
    net, sd, args, vocab, frames, regions = case_net('small_msvd')
    caps, lens = captions_for(args, vocab, 3 * n, 43)
    logits, obj, mot, alpha = net(frames, regions, caps, caps.shape[1], 1.0, seq_per_clip=n)
    (R.ragged_ce(logits, caps, lens) + 0.3 * obj.sum() - 0.2 * (mot * mot).sum()).backward()
    got = {k: p.grad for k, p in net.named_parameters()}
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    fx, rx = frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0)
    lo, oo, mo, _ = orc(fx, rx, caps, caps.shape[1], 1.0)
    (R.ragged_ce(lo, caps, lens) + 0.3 * oo[::n].sum() - 0.2 * (mo[::n] * mo[::n]).sum()).backward()
    compare_grads(got, oracle_grads(orc), 'autograd bridge, 3 clips x 2 captions')


# ---------------------------------------------------------------- 2. the default forms are untouched
def _recorded(fn, net):
    net.ops.recording = []
    out = fn()
    log, net.ops.recording = net.ops.recording, None
    return log, out


def test_default_forms_issue_the_same_launches():
    logs, state = [], []
    for kw in ({}, {'seq_per_clip': 1}):
        net, sd, args, vocab, frames, regions = case_net('small_msvd', dropout=0.3)
        net.train()
        caps, lens = captions_for(args, vocab, 3, 45)
        tr = dlsg_amd.Trainer(net, lr=1e-3)
        random.seed(3)
        log, loss = _recorded(lambda: tr.step(frames, regions, caps, lens, 0.8, **kw), net)
        logs.append(log)
        state.append((float(loss), net._flat.clone(), net._gflat.clone()))
    assert logs[0] == logs[1] and len(logs[0]) > 100
    assert 'rows_repeat' not in logs[0] and 'clip_fold' not in logs[0] and 'mean_rows_bwd' in logs[0]
    assert state[0][0] == state[1][0] and torch.equal(state[0][1], state[1][1]) and torch.equal(state[0][2], state[1][2])
    # sample(n=3) against sample(n=3, share_encoder=False)
    slogs, draws = [], []
    for kw in ({}, {'share_encoder': False}):
        net, sd, args, vocab, frames, regions = case_net('small_msvd', dropout=0.3)
        net.train()
        log, out = _recorded(lambda: net.sample(frames, regions, n=3, seed=9, **kw), net)
        slogs.append(log)
        draws.append(out)
    assert slogs[0] == slogs[1] and 'rows_repeat' not in slogs[0] and 'clip_fold' not in slogs[0]
    assert all(torch.equal(a, b) for a, b in zip(*draws))
    # the shared forms differ from them by exactly the new launches being present
    net, sd, args, vocab, frames, regions = case_net('small_msvd', dropout=0.3)
    net.train()
    log, _ = _recorded(lambda: net.sample(frames, regions, n=3, seed=9, share_encoder=True), net)
    assert log.count('rows_repeat') == 2 and 'clip_fold' not in log
    caps, lens = captions_for(args, vocab, 9, 45)
    log, _ = _recorded(lambda: dlsg_amd.Trainer(net, lr=1e-3).step(frames, regions, caps, lens, 1.0, seq_per_clip=3), net)
    assert log.count('rows_repeat') == 2 and log.count('clip_fold') == 2 and 'mean_rows_bwd' not in log


# ---------------------------------------------------------------- 3. row counts
def test_encoder_runs_on_clip_rows_and_bad_row_counts_raise():
    n = 4
    net, sd, args, vocab, frames, regions = case_net('small_msvd')
    B = frames.shape[0]
    caps, lens = captions_for(args, vocab, B * n, 47)
    L = caps.shape[1]
    seen = []
    inner = net._encode
    net._encode = lambda f, r, *a: seen.append((f.shape[0], r.shape[0])) or inner(f, r, *a)
    with torch.no_grad():
        logits, obj, mot, alpha = net(frames, regions, caps, L, 1.0, seq_per_clip=n)
    assert seen == [(B, B)]
    P, H = args.num_proposals, args.visual_hidden_size
    assert logits.shape == (B * n, L, len(vocab)) and alpha.shape[:2] == (B * n, L)
    assert obj.shape == (B, P, H) and mot.shape == (B, P, H)
    # the n = 1 call on the repeated clips gives the same logits (eval: no masks), and its proposals are these, repeated
    with torch.no_grad():
        l1, o1, m1, a1 = net(frames.repeat_interleave(n, 0), regions.repeat_interleave(n, 0), caps, L, 1.0)
    assert torch.allclose(logits, l1, atol=1e-5) and torch.equal(o1, obj.repeat_interleave(n, 0)) and torch.allclose(alpha, a1, atol=1e-6)
    ids, logp, lens_s = net.sample(frames, regions, n=n, seed=5, share_encoder=True)
    assert seen[-1] == (B, B) and ids.shape == (B * n, L) and logp.shape == (B * n, L) and lens_s.shape == (B * n,)
    for bad in (caps[:B * n - 1], caps[:B], torch.cat([caps, caps[:1]], 0)):
        with pytest.raises(ValueError):
            net(frames, regions, bad, L, 1.0, seq_per_clip=n)
        with pytest.raises(ValueError):
            dlsg_amd.Trainer(net, lr=0.0).step(frames, regions, bad, lens[:bad.shape[0]], 1.0, seq_per_clip=n)
    with pytest.raises(ValueError):
        net(frames, regions, caps, L, 1.0, seq_per_clip=0)
    with pytest.raises(ValueError):
        net(frames, regions, None, seq_per_clip=n)


@pytest.mark.parametrize('cls', ['CapBaseline1', 'CapBaselineModel'])
def test_baseline_models_refuse_several_captions_per_clip(cls):
    args, vocab = small_args(), dlsg_amd.make_vocab(50)
    net = getattr(dlsg_amd, cls)(args, vocab).eval().set_ops(SeqEmul())
    frames, regions = torch.zeros(2, 26, 112), torch.zeros(2, 26, 16, 32)
    caps = torch.full((4, 26), 5, dtype=torch.int64)
    with pytest.raises(ValueError, match='CapGnnModel only'):
        net(frames, regions, caps, 26, 1.0, seq_per_clip=2)
    with pytest.raises(ValueError, match='CapGnnModel only'):
        dlsg_amd.Trainer(net, lr=0.0).step(frames, regions, caps, [5, 5, 5, 5], 1.0, seq_per_clip=2)


def test_scst_trainer_shared_step_is_the_policy_gradient_of_the_shared_draw():
    n = 3
    net, sd, args, vocab, frames, regions = case_net('small_msvd')
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=n, lr=0.0, share_encoder=True)
    seen = []
    inner = tr.trainer.step
    tr.trainer.step = lambda *a, **k: seen.append((a, k)) or inner(*a, **k)
    expanded = []
    tr._expanded_inputs = lambda *a: expanded.append(a)
    tr.step(frames, regions, ['0', '1', '2'])
    (fx, rx, ids, lens, tf), kw = seen[0]
    assert fx is frames and rx is regions and kw['seq_per_clip'] == n and tf == 1.0 and not expanded
    want_ids, _, want_lens = net.sample(frames, regions, n=n, seed=kw['seed'], share_encoder=True)
    assert torch.equal(ids, want_ids) and torch.equal(lens, want_lens) and ids.shape[0] == 3 * n
    A = kw['seq_weights']
    assert float(A.abs().max()) > 0
    _, want = oracle_step_grads(args, vocab, sd, frames, regions, ids, lens, n, weights=A)
    compare_grads(net.grad_views(), want, 'emulated shared SCST step')


# ---------------------------------------------------------------- 4. two gloo ranks against one process
# Each rank's CrossEntropy is a mean over its own shard's words and the ranks' gradients are averaged: that equals one process
# on all clips when both shards hold the same number of words, which these lengths do (24 + 24).
GLOO_LENS = [5, 7, 6, 6, 8, 4, 6, 6]


def _gloo_build():
    net, sd, args, vocab, frames, regions = case_net('small_msrvtt')           # 4 clips -> two shards of 2
    assert frames.shape[0] == 4
    caps, _ = captions_for(args, vocab, 8, 49)
    return net, frames, regions, caps, torch.tensor(GLOO_LENS)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    net, frames, regions, caps, lens = _gloo_build()
    clips, rows = slice(rank * 2, rank * 2 + 2), slice(rank * 4, rank * 4 + 4)
    tr = dlsg_amd.Trainer(net, lr=0.0, world_size=world)
    tr.step(frames[clips], regions[clips], caps[rows], lens[rows], 1.0, seq_per_clip=2)
    np.save(os.path.join(out_dir, 'gflat%d.npy' % rank), net._gflat.numpy())
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_of_two_clips_equal_one_process_on_four():
    import tempfile
    with tempfile.TemporaryDirectory() as out:
        mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
        g0, g1 = np.load(os.path.join(out, 'gflat0.npy')), np.load(os.path.join(out, 'gflat1.npy'))
    assert np.array_equal(g0, g1)                               # every rank holds the same summed gradient
    net, frames, regions, caps, lens = _gloo_build()
    dlsg_amd.Trainer(net, lr=0.0).step(frames, regions, caps, lens, 1.0, seq_per_clip=2)
    one = net.grad_views()
    unused = net.unused_parameters
    mean = {}
    for k, p in net.named_parameters():
        o = net._offsets[k]
        mean[k] = torch.from_numpy(g0[o:o + p.numel()]).view(p.shape) / 2.0          # (Adam divides by the world size)
    compare_grads(mean, {k: (None if k in unused else one[k]) for k in mean}, 'two ranks x (2 clips x 2) against 4 clips x 2')


# ---------------------------------------------------------------- 5. the loader
def synthetic_set(tmp_path, sentences_per_clip, L=26, seed=0):
    """a CaptionSet with sentences_per_clip[v] sentences of clip v, interleaved, each caption's first word naming its row"""
    rng = np.random.RandomState(seed)
    vids = [v for v, k in enumerate(sentences_per_clip) for _ in range(k)]
    rng.shuffle(vids)
    lens = rng.randint(3, L + 1, size=len(vids)).tolist()
    caps = [torch.from_numpy(np.pad(np.r_[1000 + i, rng.randint(4, 50, size=n - 1)], (0, L - n))).long() for i, n in enumerate(lens)]
    tags = [torch.from_numpy(np.pad(rng.randint(1, 9, size=n), (0, L - n))).long() for n in lens]
    path = str(tmp_path / 'caps.pkl')
    with open(path, 'wb') as f:
        pickle.dump((caps, tags, lens, vids), f)
    N = len(sentences_per_clip)
    feats = torch.arange(N, dtype=torch.float32).view(N, 1, 1).expand(N, 2, 3).contiguous()
    store = D.ResidentFeatures.from_arrays(feats, feats.view(N, 2, 1, 3).expand(N, 2, 4, 3).contiguous(), 4, 'cpu')
    return D.CaptionSet(path), store


@pytest.mark.parametrize('world', [1, 2])
def test_clipwise_loader(tmp_path, world):
    per_clip = [5, 1, 3, 7, 2, 4, 3, 6, 3, 9, 4]                # 11 clips, some with fewer than 3 sentences
    caps, store = synthetic_set(tmp_path, per_clip)
    n, bs = 3, 4
    for epoch in (0, 1):
        clips_seen, draws = [], {}
        for rank in range(world):
            ld = D.TrainLoader(caps, store, bs, world_size=world, rank=rank, seed=7, captions_per_clip=n)
            ld.set_epoch(epoch)
            batches = list(ld)
            assert len(batches) == len(ld) == -(-(-(-len(per_clip) // world)) // bs)
            for f, r, none, c, t, lens, vids in batches:
                B = len(vids)
                assert none is None and f.shape[0] == r.shape[0] == B and c.shape == (B * n, 26) and t.shape == (B * n, 26)
                assert len(lens) == B * n and list(vids) == sorted(vids, reverse=True) and len(set(vids)) == B
                assert f[:, 0, 0].tolist() == [float(v) for v in vids]
                for b, v in enumerate(vids):
                    rows = [int(x) - 1000 for x in c[b * n:b * n + n, 0]]
                    assert all(caps.video_ids[i] == v for i in rows)                     # adjacent, and this clip's sentences
                    assert [caps.lengths[i] for i in rows] == list(lens[b * n:b * n + n])
                    assert all(torch.equal(t[b * n + j], caps.pos_tags[i]) for j, i in enumerate(rows))
                    k = per_clip[v]
                    assert len(set(rows)) == min(n, k)                                   # distinct where the clip has n
                    if k < n:
                        assert rows == (rows[:k] * n)[:n] and len(set(rows[:k])) == k    # else it cycles through its own
                    draws[v] = rows
                clips_seen += list(vids)
        if world == 1:
            assert sorted(clips_seen) == list(range(len(per_clip)))                      # an epoch covers every clip once
        else:
            assert set(clips_seen) == set(range(len(per_clip))) and len(clips_seen) == 12   # (padded by wrapping, as the sampler does)
        if epoch == 0:
            first = (list(clips_seen), dict(draws))
    assert first[0] != clips_seen and first[1] != draws                                 # another epoch, another order and draw
    # the same seed and epoch reproduce the batches
    a = D.TrainLoader(caps, store, bs, seed=7, captions_per_clip=n)
    b = D.TrainLoader(caps, store, bs, seed=7, captions_per_clip=n)
    for x, y in zip(a, b):
        assert torch.equal(x[3], y[3]) and x[5] == y[5] and x[6] == y[6]
    with pytest.raises(ValueError):
        D.TrainLoader(caps, store, bs, captions_per_clip=0)


@pytest.mark.parametrize('seed', [None, 11])
def test_one_caption_per_clip_is_the_existing_loader(tmp_path, seed):
    caps, store = synthetic_set(tmp_path, [5, 1, 3, 7, 2, 4, 3])
    outs = []
    for kw in ({}, {'captions_per_clip': 1}):
        torch.manual_seed(123)
        ld = D.TrainLoader(caps, store, 4, seed=seed, **kw)
        outs.append((len(ld), [x for ep in (0, 1) for x in (ld.set_epoch(ep) or list(ld))]))
    assert outs[0][0] == outs[1][0] == 7 and len(outs[0][1]) == len(outs[1][1]) == 14
    for x, y in zip(*[o[1] for o in outs]):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] is None and y[2] is None
        assert torch.equal(x[3], y[3]) and torch.equal(x[4], y[4]) and x[5] == y[5] and x[6] == y[6]

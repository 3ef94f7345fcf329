"""GPU: CIDEr-D on the MI355X (`dlsg_cider_d` over `scoring.DeviceCiderD`'s tables) against the host scorer, its determinism
on relaunch and graph replay, the advantages kernel (`dlsg_scst_advantage`), SCSTTrainer on a device reward against the host
reward, and a device-reward step that makes no host synchronisation.  The CPU side is tests/test_cider_device_host.py."""
import contextlib
import json
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.hip import HipOps
from test_cider_device_host import GOLD, OOV, emul_scst_advantage, encode, host_words, vocab_of
from test_gpu_scst import gpu_net

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    return HipOps()


def zipf_corpus(vocab, clips, refs_per_clip, seed):
    """reference sentences of 5..12 words drawn with a heavy head (as in captions: 'a man is ...'), so n-grams repeat"""
    rng = random.Random(seed)
    V = len(vocab)
    words = [vocab.idx2word[i] for i in range(4, V)]
    pick = lambda: words[min(int(rng.paretovariate(0.8)) - 1, len(words) - 1)]
    refs = {'v%d' % c: [' '.join(pick() for _ in range(rng.randint(5, 12))) for _ in range(refs_per_clip)] for c in range(clips)}
    return refs, rng


def sampled_rows(vocab, refs, vids, rng, L=26):
    """hypotheses like a sampler's: a reference of the clip with some words replaced, or random head words; <end>, then
    whatever the decoder wrote after it; a few rows without <end>"""
    V, end = len(vocab), vocab('<end>')
    rows = []
    for i, v in enumerate(vids):
        ws = [vocab(w) for w in rng.choice(refs[v]).split()]
        if i % 3 == 2:
            ws = [min(int(rng.paretovariate(0.8)) + 3, V - 1) for _ in range(rng.randint(1, 14))]
        ws = [rng.randrange(4, V) if rng.random() < 0.2 else w for w in ws]
        if i % 11 == 5:
            row = (ws * L)[:L]
        else:
            row = (ws + [end] + [rng.randrange(V) for _ in range(L)])[:L]
        rows.append(row)
    return rows


def check(dc, vids, rows, rtol=1e-12, atol=1e-12):
    ids = torch.tensor(rows, dtype=torch.int64, device=DEV)
    got = dc.scores_device(ids, dc.index(vids)).cpu().numpy()
    want = dc.cider.scores(vids, [host_words(dc.vocab, r, dc.end_id) for r in rows])
    assert np.allclose(got, want, rtol=rtol, atol=atol), (np.abs(got - want).max(), int(np.abs(got - want).argmax()))
    return got, want


def test_golden_cases():
    for case in json.load(open(GOLD)):
        gts, res = case['gts'], case['res']
        vids = sorted(gts)
        ref_words = sorted(set(w for v in vids for c in gts[v] for w in c.split()))
        hyp_words = sorted(set(w for v in vids[:2] for w in res[v][0].split()))
        vocab = vocab_of(hyp_words + ref_words[::3])
        dc = S.DeviceCiderD(gts, vocab)
        got, _ = check(dc, vids, [encode(vocab, res[v][0], 26) for v in vids])
        full = vocab_of(hyp_words + ref_words + [w for v in vids for w in res[v][0].split()])
        dc = S.DeviceCiderD(gts, full)
        got, _ = check(dc, vids, [encode(full, res[v][0], 26) for v in vids])
        assert np.allclose(got, case['cider_per'], rtol=0, atol=1e-9)


@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_msvd_sized_corpus(n):
    """1 200 clips x ~40 references, V = 10 000, 320 rows (64 clips x 5 samples)"""
    vocab = dlsg_amd.make_vocab(10000)
    rng = random.Random(n)
    refs, rng = zipf_corpus(vocab, 1200, 40, 11)
    for v in list(refs)[::7]:
        refs[v] = refs[v][:rng.randint(30, 40)]
    dc = S.DeviceCiderD(refs, vocab, n=n)
    clips = rng.sample(sorted(refs), 64)
    vids = [v for v in clips for _ in range(5)]
    got, want = check(dc, vids, sampled_rows(vocab, refs, vids, rng))
    assert (want > 0).mean() > 0.3


def test_msrvtt_sized_corpus():
    """6 513 clips x 20 references, V = 10 000"""
    vocab = dlsg_amd.make_vocab(10000)
    refs, rng = zipf_corpus(vocab, 6513, 20, 12)
    dc = S.DeviceCiderD(refs, vocab)
    vids = [v for v in rng.sample(sorted(refs), 64) for _ in range(5)]
    got, want = check(dc, vids, sampled_rows(vocab, refs, vids, rng))
    assert (want > 0).mean() > 0.3


def test_ids_outside_the_vocabulary_and_row_layouts(ops):
    """ids outside [0, V) (negative, V, huge) read nothing out of bounds and score as one word outside the vocabulary; rows at
    a row stride (a view of a wider buffer); L = 64; an empty batch"""
    vocab = dlsg_amd.make_vocab(3000)
    refs, rng = zipf_corpus(vocab, 50, 20, 13)
    dc = S.DeviceCiderD(refs, vocab)
    V = len(vocab)
    vids = [rng.choice(sorted(refs)) for _ in range(96)]
    rows = sampled_rows(vocab, refs, vids, rng, L=64)
    for i, r in enumerate(rows):
        for _ in range(i % 4):
            r[rng.randrange(12)] = rng.choice([-1, V, V + 1, 1 << 40, -(1 << 62), (1 << 63) - 1])
    ids = torch.tensor(rows, dtype=torch.int64)
    got = dc.scores_device(ids.to(DEV), dc.index(vids)).cpu().numpy()
    want = dc.cider.scores(vids, [host_words(vocab, r, dc.end_id) for r in rows])
    assert OOV in ' '.join(host_words(vocab, r, dc.end_id) for r in rows)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    wide = torch.full((96, 80), 7, dtype=torch.int64)
    wide[:, 3:3 + 26] = ids[:, :26]
    got2 = dc.scores_device(wide.to(DEV)[:, 3:3 + 26], dc.index(vids)).cpu().numpy()
    want2 = dc.cider.scores(vids, [host_words(vocab, r[:26], dc.end_id) for r in rows])
    assert np.allclose(got2, want2, rtol=1e-12, atol=1e-12)
    assert dc.scores_device(torch.zeros(0, 26, dtype=torch.int64, device=DEV), dc.index([])).numel() == 0
    with pytest.raises(RuntimeError):
        dc.scores_device(torch.zeros(2, 65, dtype=torch.int64, device=DEV), dc.index(vids[:2]))
    torch.cuda.synchronize()


def test_relaunch_and_graph_replay_are_bit_identical():
    vocab = dlsg_amd.make_vocab(10000)
    refs, rng = zipf_corpus(vocab, 300, 20, 14)
    dc = S.DeviceCiderD(refs, vocab)
    vids = [v for v in rng.sample(sorted(refs), 64) for _ in range(5)]
    ids = torch.tensor(sampled_rows(vocab, refs, vids, rng), dtype=torch.int64, device=DEV)
    cidx = dc.index(vids)
    first = dc.scores_device(ids, cidx)
    again = [dc.scores_device(ids, cidx) for _ in range(5)]
    torch.cuda.synchronize()
    assert all(torch.equal(first, x) for x in again)
    out = torch.empty(ids.shape[0], dtype=torch.float64, device=DEV)
    ops = dc._ops()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.cider_d(ids, cidx, dc.end_id, dc, out)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.cider_d(ids, cidx, dc.end_id, dc, out)
    for _ in range(3):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)


@pytest.mark.parametrize('greedy', [False, True])
def test_scst_advantage_kernel(ops, greedy):
    rng = np.random.default_rng(3)
    B, n = 64, 5
    r = rng.random(B * n) * 4
    r[::7] = 0.0
    lens = rng.integers(1, 27, B * n)
    g = rng.random(B) * 4 if greedy else None
    adv = torch.empty(B * n, dtype=torch.float32, device=DEV)
    stats = torch.empty(3, dtype=torch.float64, device=DEV)
    ops.scst_advantage(torch.from_numpy(r).to(DEV), torch.from_numpy(lens).to(DEV), None if g is None else torch.from_numpy(g).to(DEV),
                       n, adv, stats)
    want_adv, want_st = emul_scst_advantage(r, lens, g, n)
    torch.cuda.synchronize()
    got = adv.cpu().numpy()
    if greedy:
        assert np.array_equal(got, want_adv)
    else:
        assert np.allclose(got, want_adv, rtol=0, atol=1e-6)
    assert np.allclose(stats.cpu().numpy(), want_st, rtol=1e-12, atol=1e-12)


def scst_corpus(vocab, clips=3):
    rng = random.Random(9)
    words = [vocab.idx2word[i] for i in range(4, len(vocab))] + ['never-sampled']
    return {str(b): [' '.join(rng.choice(words) for _ in range(rng.randint(2, 8))) for _ in range(5)] for b in range(clips)}


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_scst_on_device_reward_equals_host_reward(baseline):
    """three graph-replayed SCST steps, same seed and weights, one with CiderD and one with DeviceCiderD: the same samples,
    advantages within 1e-6, loss and weights within the graphs-vs-eager tolerance of tests/test_gpu_scst.py"""
    res = []
    for device_reward in (False, True):
        net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
        host = S.CiderD(scst_corpus(vocab))
        reward = host.to_device(vocab) if device_reward else host
        tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, baseline=baseline, lr=1e-3, use_graphs=True)
        seen = []
        inner = tr.trainer.step
        tr.trainer.step = lambda *a, **k: seen.append((a[2].clone(), k['seq_weights'].clone())) or inner(*a, **k)
        random.seed(1)
        outs = [tr.step(frames, regions, ['0', '1', '2']) for _ in range(3)]
        torch.cuda.synchronize()
        res.append(([float(o['loss']) for o in outs], [[float(o[k]) for k in ('reward_mean', 'baseline_mean', 'mean_len')] for o in outs],
                    seen, net._flat.clone()))
    (lh, sh, eh, fh), (ld, sdv, ed, fd) = res
    for a, b in zip(eh, ed):
        assert torch.equal(a[0], b[0])
        assert (a[1].to(DEV) - b[1]).abs().max().item() <= 1e-6
    assert any(a[1].abs().max().item() > 0 for a in eh)
    assert np.allclose(sh, sdv, rtol=1e-12, atol=1e-12)
    assert np.allclose(lh, ld, rtol=1e-5, atol=1e-6), (lh, ld)
    assert (fh - fd).abs().max().item() <= 3e-5


@contextlib.contextmanager
def no_host_sync():
    """torch's sync debug mode 'error', and the host reads of a device tensor (.cpu, .item, .tolist, float) raising as well"""
    names = ('cpu', 'item', 'tolist', '__float__')
    saved = {k: torch.Tensor.__dict__.get(k) for k in names}
    orig = {k: getattr(torch.Tensor, k) for k in names}

    def guard(name):
        def f(self, *a, **k):
            if self.is_cuda:
                raise RuntimeError('host read of a device tensor (%s) inside a step that must not synchronise' % name)
            return orig[name](self, *a, **k)
        return f
    for k in names:
        setattr(torch.Tensor, k, guard(k))
    torch.cuda.set_sync_debug_mode('error')
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode('default')
        for k in names:
            if saved[k] is None:
                delattr(torch.Tensor, k)
            else:
                setattr(torch.Tensor, k, saved[k])


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_device_reward_step_makes_no_host_synchronisation(baseline):
    for device_reward in (True, False):
        net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
        host = S.CiderD(scst_corpus(vocab))
        reward = host.to_device(vocab) if device_reward else host
        tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, baseline=baseline, lr=1e-3, use_graphs=True, check_every=0)
        vids = ['0', '1', '2']
        for _ in range(2):
            tr.step(frames, regions, vids)                      # captures
        torch.cuda.synchronize()
        if device_reward:
            with no_host_sync():
                out = tr.step(frames, regions, vids)
            torch.cuda.synchronize()
            assert all(torch.is_tensor(out[k]) and out[k].is_cuda and out[k].dim() == 0 for k in ('reward_mean', 'baseline_mean', 'mean_len'))
            assert np.isfinite(float(out['loss'])) and float(out['mean_len']) >= 1.0
        else:
            with pytest.raises(RuntimeError):
                with no_host_sync():
                    tr.step(frames, regions, vids)
            torch.cuda.synchronize()

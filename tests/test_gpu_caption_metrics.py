"""GPU: BLEU-1..4 / ROUGE_L on the MI355X (`dlsg_caption_metrics`, `dlsg_caption_corpus` over `scoring.DeviceCaptionMetrics`'s
tables) against the host functions and the reference-made fixture, the LDS staging paths, determinism on relaunch and graph
replay, SCSTTrainer on a `DeviceMixedReward` against the host `MixedReward`, and a mixed-reward step that makes no host
synchronisation.  The CPU side is tests/test_caption_metrics_host.py."""
import contextlib
import json
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import hip
from dlsg_amd import scoring as S
from test_caption_metrics_host import MIX, check_edge_rows, check_golden_case, check_rows, outside_ids_case, unk_case
from test_cider_device_host import GOLD, OOV, encode, host_words
from test_gpu_cider_device import sampled_rows, scst_corpus, zipf_corpus
from test_gpu_scst import gpu_net

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_golden_cases():
    for case in json.load(open(GOLD)):
        check_golden_case(case, S.DeviceCaptionMetrics, device=DEV)


def test_edge_rows_over_a_random_corpus():
    check_edge_rows(S.DeviceCaptionMetrics, device=DEV)


def test_msvd_like_corpus():
    """300 clips x 40 references, V = 10 000, 320 rows (64 clips x 5 samples)"""
    vocab = dlsg_amd.make_vocab(10000)
    refs, rng = zipf_corpus(vocab, 300, 40, 21)
    dm = S.DeviceCaptionMetrics(refs, vocab)
    vids = [v for v in rng.sample(sorted(refs), 64) for _ in range(5)]
    got, stats, _ = check_rows(dm, vids, sampled_rows(vocab, refs, vids, rng), device=DEV)
    assert (got[:, 0] > 0).mean() > 0.3
    assert (stats[:, 0] > 0).mean() > 0.3 and (got[:, 3] > 1e-3).mean() > 0.3      # BLEU's `tiny` keeps even a row without a match above 0


def test_references_beyond_one_lds_stage():
    """a clip whose references total more words than one stage and number more than one pass takes (63); a single reference
    longer than the stage, between short ones, read from global memory"""
    stage = hip.METRICS_STAGE
    vocab = dlsg_amd.make_vocab(400)
    rng = random.Random(31)
    words = [vocab.idx2word[i] for i in range(4, 60)]
    sent = lambda n: ' '.join(rng.choice(words) for _ in range(n))
    per = stage // 20
    refs = {'many': [sent(per) for _ in range(25)] + [sent(rng.randint(3, 9)) for _ in range(70)],
            'long': [sent(7), sent(stage + 37), sent(9), sent(stage), sent(5)],
            'plain': [sent(8), sent(6)]}
    assert sum(len(r.split()) for r in refs['many']) > stage and len(refs['many']) > 63
    dm = S.DeviceCaptionMetrics(refs, vocab)
    vids, rows = [], []
    for v in sorted(refs):
        for i in range(6):
            src = refs[v][(7 * i) % len(refs[v])].split()
            at = rng.randrange(max(1, len(src) - 12))
            hyp = [w if rng.random() < 0.8 else rng.choice(words) for w in src[at:at + rng.randint(3, 14)]]
            vids.append(v)
            rows.append(encode(vocab, ' '.join(hyp), 26, rng))
    got, stats, _ = check_rows(dm, vids, rows, device=DEV)
    assert (got[:, 3] > 0.05).sum() >= 6 and (got[:, 4] > 0).all()


def test_ids_outside_the_vocabulary_row_layouts_and_refusals():
    """ids outside [0, V) read nothing out of bounds and count as words that match nothing; a reference word outside the
    vocabulary against a sampled <unk>; rows at a row stride (a view of a wider buffer); L = 64; an empty batch; L = 65 is
    refused; a clip index outside the tables gives NaN (a bound the kernel checks) and zero statistics"""
    refs, vocab, vids, rows = outside_ids_case()
    dm = S.DeviceCaptionMetrics(refs, vocab)
    _, _, hyps = check_rows(dm, vids, rows, device=DEV)
    assert OOV in ' '.join(hyps)
    urefs, uvocab, uvids, urows = unk_case()
    _, ustats, _ = check_rows(S.DeviceCaptionMetrics(urefs, uvocab), uvids, urows, device=DEV)
    assert ustats[1, 0] == 4 and ustats[1, 8] == 5

    vocab = dlsg_amd.make_vocab(3000)
    refs, rng = zipf_corpus(vocab, 50, 20, 13)
    dm = S.DeviceCaptionMetrics(refs, vocab)
    V = len(vocab)
    vids = [rng.choice(sorted(refs)) for _ in range(96)]
    rows = sampled_rows(vocab, refs, vids, rng, L=64)
    for i, r in enumerate(rows):
        for _ in range(i % 4):
            r[rng.randrange(12)] = rng.choice([-1, V, V + 1, 1 << 40, -(1 << 62), (1 << 63) - 1])
    check_rows(dm, vids, rows, device=DEV)
    ids = torch.tensor(rows, dtype=torch.int64)
    wide = torch.full((96, 80), 7, dtype=torch.int64)
    wide[:, 3:3 + 26] = ids[:, :26]
    view = wide.to(DEV)[:, 3:3 + 26]
    cidx = dm.index(vids)
    assert view.stride(0) == 80
    got = dm.scores_device(view, cidx).cpu().numpy()
    want = dm.scores(vids, [host_words(vocab, r[:26], dm.end_id) for r in rows])
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    none = torch.zeros(0, 26, dtype=torch.int64, device=DEV)
    assert dm.scores_device(none, dm.index([])).shape == (0, 5) and dm.stats_device(none, dm.index([])).shape == (0, 10)
    with pytest.raises(RuntimeError):
        dm.scores_device(torch.zeros(2, 65, dtype=torch.int64, device=DEV), dm.index(vids[:2]))
    with pytest.raises(RuntimeError):
        dm.corpus_device(none, dm.index([]))
    off = torch.tensor([0, dm.n_clips, -1, 1 << 30, 3], dtype=torch.int32, device=DEV)
    five = ids[:5, :26].to(DEV)
    sc, st = dm.scores_device(five, off).cpu(), dm.stats_device(five, off).cpu()
    rw = torch.empty(5, dtype=torch.float64, device=DEV)
    dm._ops().caption_metrics(five, off, dm.end_id, dm, reward=rw, weights=[0, 1, 0, 0, 0, 1])
    torch.cuda.synchronize()
    assert torch.isnan(sc[1:4]).all() and torch.isfinite(sc[[0, 4]]).all() and not st[1:4].any() and st[[0, 4]].any()
    assert torch.isnan(rw[1:4]).all().item() and torch.equal(rw[[0, 4]].cpu(), sc[[0, 4]][:, 0] + sc[[0, 4]][:, 4])


def test_relaunch_and_graph_replay_are_bit_identical():
    vocab = dlsg_amd.make_vocab(10000)
    refs, rng = zipf_corpus(vocab, 300, 20, 14)
    dm = S.DeviceCaptionMetrics(refs, vocab)
    vids = [v for v in rng.sample(sorted(refs), 64) for _ in range(5)]
    ids = torch.tensor(sampled_rows(vocab, refs, vids, rng), dtype=torch.int64, device=DEV)
    cidx = dm.index(vids)
    R = ids.shape[0]
    base = torch.rand(R, dtype=torch.float64, device=DEV) * 3
    weights = [1.0, 0.0, 0.5, 0.0, 2.0, 1.0]
    ops = dm._ops()

    def launch():
        out = (torch.full((R, 5), -1.0, dtype=torch.float64, device=DEV), torch.full((R, 10), -1, dtype=torch.int32, device=DEV),
               torch.full((R,), -1.0, dtype=torch.float64, device=DEV))
        ops.caption_metrics(ids, cidx, dm.end_id, dm, scores=out[0], stats=out[1], reward=out[2], weights=weights, base=base)
        return out
    first = launch()
    again = [launch() for _ in range(5)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for run in again for a, b in zip(first, run))
    want = (base + 0.5 * first[0][:, 1]) + 2.0 * first[0][:, 3]
    assert torch.equal(first[2], want + first[0][:, 4]) and (first[1][:, 0] > 0).float().mean().item() > 0.3
    out = tuple(torch.empty_like(x) for x in first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                           # warm-up outside the capture
        ops.caption_metrics(ids, cidx, dm.end_id, dm, scores=out[0], stats=out[1], reward=out[2], weights=weights, base=base)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.caption_metrics(ids, cidx, dm.end_id, dm, scores=out[0], stats=out[1], reward=out[2], weights=weights, base=base)
    for _ in range(3):
        for x in out:
            x.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, out))


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_scst_on_device_mixed_reward_equals_host_mixed_reward(baseline):
    """three graph-replayed SCST steps, same seed and weights, one with MixedReward and one with DeviceMixedReward: the same
    samples, advantages within 1e-6, loss and weights within the tolerances of test_scst_on_device_reward_equals_host_reward"""
    res = []
    for device_reward in (False, True):
        net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
        host = S.MixedReward(scst_corpus(vocab), MIX)
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
def test_mixed_reward_step_makes_no_host_synchronisation(baseline):
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    reward = S.DeviceMixedReward(scst_corpus(vocab), vocab, MIX)
    tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, baseline=baseline, lr=1e-3, use_graphs=True, check_every=0)
    vids = ['0', '1', '2']
    for _ in range(2):
        tr.step(frames, regions, vids)                      # captures
    torch.cuda.synchronize()
    with no_host_sync():
        out = tr.step(frames, regions, vids)
    torch.cuda.synchronize()
    assert all(torch.is_tensor(out[k]) and out[k].is_cuda and out[k].dim() == 0 for k in ('reward_mean', 'baseline_mean', 'mean_len'))
    assert np.isfinite(float(out['loss'])) and float(out['mean_len']) >= 1.0 and float(out['reward_mean']) > 0

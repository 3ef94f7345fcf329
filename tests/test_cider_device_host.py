"""CPU: CIDEr-D on the device's tables (`scoring.DeviceCiderD`) and the device-reward form of the SCST step.  The two new
kernels (`dlsg_cider_d`, `dlsg_scst_advantage`) are emulated in numpy, following the kernel's algorithm over the very tables
DeviceCiderD builds (`emul_cider_d`, `CiderEmul` below), and checked against the host scorer `CiderD.scores`.  The GPU side is
tests/test_gpu_cider_device.py."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.config import Vocabulary
from emul_ngram import find as _find, np_tables, row_ngrams
from test_scst_host import ScstEmul, small_net

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scoring.json')
OOV = '<out-of-range-id>'               # the string an id outside [0, V) stands for in the host reference


def emul_cider_d(tb, ids, clip_idx, end_id):
    """numpy restatement of cider_d_kernel (csrc/cider.hip): per row the words before the first end_id; per order k the n-grams
    at every position, kept at their first position with their count; idf from the corpus table (log_n when absent, and for an
    n-gram holding an id outside [0, V), which is never looked up); per reference min(w_h, w_r) w_r, divided by the norms when
    both are nonzero, times the length penalty, summed per position over the references and then over positions."""
    a = np_tables(tb)
    ids = ids.cpu().numpy()
    clip_idx = clip_idx.cpu().numpy()
    R, L = ids.shape
    n, V = tb.n, tb.V
    out = np.empty(R, dtype=np.float64)
    for r in range(R):
        c = int(clip_idx[r])
        if not 0 <= c < tb.n_clips or a['clip_off'][c + 1] <= a['clip_off'][c]:
            out[r] = float('nan')
            continue
        rb, re = int(a['clip_off'][c]), int(a['clip_off'][c + 1])
        tot = np.zeros(n)
        for k in range(n):
            ln, _, _, keys, kbad, first, tf = row_ngrams(ids[r], end_id, V, k)
            lh = max(ln - 1, 0) if n >= 2 else 0
            m = len(keys)
            if m == 0:
                continue
            wh = np.zeros(m)
            for i in range(m):
                if first[i]:
                    p = -1 if kbad[i] else _find(a['gram_keys'], keys[i])
                    wh[i] = tf[i] * (a['gram_idf'][p] if p >= 0 else tb.log_n)
            nh = math.sqrt(float((wh * wh).sum()))
            acc = np.zeros(m)
            for q in range(rb, re):
                e0, e1 = int(a['ref_off'][q]), int(a['ref_off'][q + 1])
                nr = a['ref_norm'][q, k]
                pen = math.exp(-float(lh - int(a['ref_len'][q])) ** 2 / (2 * tb.sigma * tb.sigma))
                for i in range(m):
                    cq = 0.0
                    if first[i] and not kbad[i]:
                        p = _find(a['ent_keys'][e0:e1], keys[i])
                        wr = a['ent_w'][e0 + p] if p >= 0 else 0.0
                        cq = min(wh[i], wr) * wr
                    if nh != 0 and nr != 0:
                        cq /= nh * nr
                    acc[i] += cq * pen
            tot[k] = acc.sum()
        out[r] = tot.sum() / n / (re - rb) * 10.0
    return out


def emul_scst_advantage(r, lens, greedy, n):
    r = np.asarray(r, dtype=np.float64)
    if greedy is not None:
        b = np.repeat(np.asarray(greedy, dtype=np.float64), n)
    else:
        R = r.reshape(-1, n)
        b = ((R.sum(1, keepdims=True) - R) / (n - 1)).reshape(-1)
    return (r - b).astype(np.float32), np.array([r.mean(), b.mean(), np.asarray(lens, dtype=np.float64).mean()])


class CiderEmul(ScstEmul):
    """ScstEmul + the two reward kernels"""

    def cider_d(self, ids, clip_idx, end_id, tables, out):
        assert ids.dtype == torch.int64 and clip_idx.dtype == torch.int32 and out.dtype == torch.float64
        out.copy_(torch.from_numpy(emul_cider_d(tables, ids, clip_idx, end_id)))

    def scst_advantage(self, rewards, lens, greedy, n, adv, stats):
        a, s = emul_scst_advantage(rewards.numpy(), lens.numpy(), None if greedy is None else greedy.numpy(), n)
        adv.copy_(torch.from_numpy(a))
        stats.copy_(torch.from_numpy(s))


def host_words(vocab, row, end_id):
    """decode_tokens' string of an id row, an id outside [0, V) standing for the word OOV"""
    words = []
    for t in row:
        t = int(t)
        if t == end_id:
            break
        words.append(vocab.idx2word[t] if 0 <= t < len(vocab) else OOV)
    return ' '.join(words)


def vocab_of(words):
    v = Vocabulary()
    for w in words:
        v.add_word(w)
    return v


def encode(vocab, hyp, L, rng=None, end=True):
    """a hypothesis string as an id row of length L: the words (<unk> outside the vocabulary), <end> (when it fits and `end`),
    then filler ids"""
    ids = [vocab(w) for w in hyp.split()]
    if end and len(ids) < L:
        ids.append(vocab('<end>'))
    while len(ids) < L:
        ids.append(rng.randrange(len(vocab)) if rng is not None else 0)
    return ids[:L]


def check_rows(dc, vids, rows, atol=1e-12):
    """emulated device scores of id rows == CiderD.scores of their decoded strings"""
    vocab = dc.vocab
    ids = torch.tensor(rows, dtype=torch.int64)
    got = emul_cider_d(dc, ids, dc.index(vids), dc.end_id)
    want = dc.cider.scores(vids, [host_words(vocab, r, dc.end_id) for r in rows])
    assert np.allclose(got, want, rtol=0, atol=atol), np.abs(got - want).max()
    return got, want


def random_corpus(rng, clips, refs_per_clip, words, lo=1, hi=12):
    return {'c%d' % c: [' '.join(rng.choice(words) for _ in range(rng.randint(lo, hi))) for _ in range(refs_per_clip)]
            for c in range(clips)}


# ------------------------------------------------------------------------------------------------ tables and scores
def test_golden_cases_with_out_of_vocabulary_reference_words():
    """the three golden cases.  The vocabulary holds the hypothesis words of two clips and every third reference word: the
    remaining reference words are out of vocabulary (their n-grams leave the device tables, but not the norms), and the other
    hypotheses' words outside it become <unk>, as a model would emit them."""
    for case in json.load(open(GOLD)):
        gts, res = case['gts'], case['res']
        vids = sorted(gts)
        ref_words = sorted(set(w for v in vids for c in gts[v] for w in c.split()))
        hyp_words = sorted(set(w for v in vids[:2] for w in res[v][0].split()))
        vocab = vocab_of(hyp_words + ref_words[::3])
        dc = S.DeviceCiderD(gts, vocab, device='cpu')
        assert len(set(ref_words) - set(vocab.word2idx)) > 0
        rows = [encode(vocab, res[v][0], 26) for v in vids]
        got, want = check_rows(dc, vids, rows)
        whole = [i for i, v in enumerate(vids) if all(w in vocab.word2idx for w in res[v][0].split())]
        assert len(whole) >= 2 and len(whole) < len(vids)
        assert np.allclose(got[whole], np.array(case['cider_per'])[whole], rtol=0, atol=1e-9)
        # every table n-gram is made of vocabulary words; every reference's entries are sorted and a subset of the corpus table
        a = np_tables(dc)
        assert np.all(np.diff(a['gram_keys'].astype(object)) > 0)
        for q in range(len(a['ref_len'])):
            e = a['ent_keys'][a['ref_off'][q]:a['ref_off'][q + 1]]
            assert np.all(np.diff(e.astype(object)) > 0) and np.isin(e, a['gram_keys']).all()


def test_out_of_vocabulary_reference_word_does_not_match_a_sampled_unk():
    refs = {'a': ['a dog runs zebroid fast', 'a dog runs'], 'b': ['the cat sits']}
    vocab = vocab_of(['a', 'dog', 'runs', 'fast', 'the', 'cat', 'sits'])         # 'zebroid' is not a word of the vocabulary
    dc = S.DeviceCiderD(refs, vocab, device='cpu')
    unk = vocab('<unk>')
    assert vocab('zebroid') == unk and 'zebroid' not in vocab.word2idx
    rows = [encode(vocab, 'a dog runs', 8), encode(vocab, 'a dog runs', 8)]
    rows[1][3:5] = [unk, vocab.word2idx['fast']]                                   # "a dog runs <unk> fast"
    got, want = check_rows(dc, ['a', 'a'], rows)
    # with <unk> matching 'zebroid' the 'runs zebroid' / 'zebroid fast' n-grams would have raised the score
    cheat = dc.cider.scores(['a'], ['a dog runs zebroid fast'])[0]
    assert got[1] < cheat - 1e-3


@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_random_corpora_and_edge_rows(n):
    rng = random.Random(100 + n)
    words = ['w%d' % i for i in range(14)]
    refs = random_corpus(rng, 9, 5, words)
    vocab = vocab_of(words[:11])                          # w11..w13 appear in references only
    dc = S.DeviceCiderD(refs, vocab, n=n, device='cpu')
    end, unk, pad = vocab('<end>'), vocab('<unk>'), vocab('<pad>')
    inv = [vocab.word2idx[w] for w in words[:11]]
    vids, rows = [], []
    L = 20
    for c in sorted(refs):
        for kind in range(8):
            if kind == 0:
                row = [end] + [rng.choice(inv) for _ in range(L - 1)]                   # empty hypothesis
            elif kind == 1:
                row = [rng.choice(inv), end] + [rng.randrange(len(vocab)) for _ in range(L - 2)]    # one word
            elif kind == 2:
                row = [rng.choice(inv[:3]) for _ in range(L)]                          # no <end>, many repeats
            elif kind == 3:
                row = [rng.choice(inv + [unk, pad]) for _ in range(9)] + [end] + [0] * (L - 10)
            elif kind == 4:
                row = encode(vocab, ' '.join(w for w in refs[c][0].split() if w in vocab.word2idx), L, rng)   # a reference
            else:
                row = [rng.choice(inv) for _ in range(rng.randint(2, 12))]
                row = (row + [end] + [rng.randrange(len(vocab)) for _ in range(L)])[:L]
            vids.append(c)
            rows.append(row)
    got, want = check_rows(dc, vids, rows)
    assert (want > 0).sum() > len(rows) // 3 and (want == 0).any()


def test_ids_outside_the_vocabulary_match_nothing():
    rng = random.Random(5)
    words = ['w%d' % i for i in range(8)]
    refs = random_corpus(rng, 4, 4, words, 3, 9)
    vocab = vocab_of(words)
    dc = S.DeviceCiderD(refs, vocab, device='cpu')
    V, end = len(vocab), vocab('<end>')
    inv = [vocab.word2idx[w] for w in words]
    rows, vids = [], []
    for c in sorted(refs):
        for bad in (-1, V, V + 7, 1 << 40, -(1 << 62)):
            row = [rng.choice(inv) for _ in range(10)]
            row[rng.randrange(10)] = bad
            row[rng.randrange(10)] = bad
            rows.append(row + [end] + [bad] * 5)
            vids.append(c)
    # the last word of an n-gram out of range must not turn its key into the shorter n-gram's (0xFFFF past the order)
    rows.append([inv[0], V, end] + [0] * 13)
    vids.append('c0')
    check_rows(dc, vids, rows)


def test_to_device_reuses_the_host_scorer_and_builds_the_same_tables():
    rng = random.Random(2)
    words = ['w%d' % i for i in range(10)]
    refs = random_corpus(rng, 5, 3, words)
    vocab = vocab_of(words[:8])
    cd = S.CiderD(refs)
    a, b = cd.to_device(vocab, device='cpu'), S.DeviceCiderD(refs, vocab, device='cpu')
    assert a.cider is cd and a.df is cd.df and a.log_n == cd.log_n
    for k in ('gram_keys', 'gram_idf', 'clip_off', 'ref_off', 'ref_norm', 'ref_len', 'ent_keys', 'ent_w'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    hyps = ['w1 w2 w3', 'w9 w1']
    assert np.array_equal(a.scores(['c0', 'c1'], hyps), cd.scores(['c0', 'c1'], hyps))
    idx = a.index(['c3', 'c0', 'c3'])
    assert idx.dtype == torch.int32 and idx.tolist() == [3, 0, 3]


def test_refusals():
    refs = {'a': ['x y z']}
    with pytest.raises(ValueError):
        S.DeviceCiderD(refs, dlsg_amd.make_vocab(65536), device='cpu')
    S.DeviceCiderD(refs, dlsg_amd.make_vocab(65535), device='cpu')
    for n in (0, 5):
        with pytest.raises(ValueError):
            S.DeviceCiderD(refs, vocab_of(['x', 'y', 'z']), n=n, device='cpu')
    with pytest.raises(ValueError):
        S.CiderD(refs, n=5).to_device(vocab_of(['x']), device='cpu')
    dc = S.DeviceCiderD(refs, vocab_of(['x', 'y', 'z']), device='cpu')
    with pytest.raises(KeyError):
        dc.index(['a', 'b'])


def test_pack_ngram():
    assert S.pack_ngram([1]) == 1 | 0xFFFF << 16 | 0xFFFF << 32 | 0xFFFF << 48
    assert S.pack_ngram([1, 2, 3, 4]) == 1 | 2 << 16 | 3 << 32 | 4 << 48
    assert S.pack_ngram([7, 0]) != S.pack_ngram([7])


# ------------------------------------------------------------------------------------------------ SCST on a device reward
def corpus_for(vocab, clips, seed=0):
    rng = random.Random(seed)
    words = [vocab.idx2word[i] for i in range(4, len(vocab))] + ['zzz-unseen']
    return {str(b): [' '.join(rng.choice(words) for _ in range(rng.randint(2, 7))) for _ in range(4)] for b in range(clips)}


def _spy(tr):
    seen = []
    inner = tr.trainer.step

    def step(*a, **k):
        seen.append((a, k))
        return inner(*a, **k)
    tr.trainer.step = step
    return seen


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_scst_step_on_a_device_reward_equals_the_host_reward_step(baseline):
    res = []
    for device_reward in (False, True):
        net, sd, args, vocab, frames, regions, _, _ = small_net()
        net.set_ops(CiderEmul())
        host = S.CiderD(corpus_for(vocab, 3))
        reward = host.to_device(vocab, device='cpu') if device_reward else host
        if device_reward:
            reward.ops = net.ops
        tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, baseline=baseline, lr=1e-3)
        seen = _spy(tr)
        outs = [tr.step(frames, regions, ['0', '1', '2']) for _ in range(2)]
        res.append((outs, seen, net._flat.clone()))
    (oh, sh, fh), (od, sd_, fd) = res
    for a, b in zip(sh, sd_):
        assert torch.equal(a[0][2], b[0][2]) and torch.equal(a[0][3], b[0][3])          # the same sampled words and lengths
        wh, wd = a[1]['seq_weights'], b[1]['seq_weights']
        assert wd.dtype == torch.float32 and (wh - wd).abs().max().item() <= 1e-6
        assert wh.abs().max().item() > 0
    for a, b in zip(oh, od):
        assert isinstance(a['reward_mean'], float) and torch.is_tensor(b['reward_mean']) and b['reward_mean'].dim() == 0
        for k in ('reward_mean', 'baseline_mean', 'mean_len'):
            assert abs(a[k] - float(b[k])) <= 1e-12, k
        assert abs(float(a['loss']) - float(b['loss'])) <= 1e-6
    assert (fh - fd).abs().max().item() <= 1e-6


@pytest.mark.parametrize('baseline', ['mean', 'greedy'])
def test_host_reward_step_issues_the_same_launches(baseline):
    """a reward with `scores` only takes the host path: no reward kernel, and the device-reward step issues the host step's
    launches plus the reward's (1 or 2 CIDEr-D launches and the advantages) right before the train step"""
    logs = []
    for device_reward in (False, True):
        net, sd, args, vocab, frames, regions, _, _ = small_net()
        net.set_ops(CiderEmul())
        host = S.CiderD(corpus_for(vocab, 3))
        reward = host.to_device(vocab, device='cpu') if device_reward else host
        if device_reward:
            reward.ops = net.ops
        tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=3, baseline=baseline, lr=1e-3)
        random.seed(4)
        net.ops.recording = []
        tr.step(frames, regions, ['0', '1', '2'])
        logs.append(net.ops.recording)
        net.ops.recording = None
    host_log, dev_log = logs
    new = ('cider_d', 'scst_advantage')
    assert not any(c in new for c in host_log)
    assert [c for c in dev_log if c not in new] == host_log
    assert dev_log.count('cider_d') == (2 if baseline == 'greedy' else 1) and dev_log.count('scst_advantage') == 1


def test_advantage_emulation_is_the_step_formula():
    rng = np.random.default_rng(0)
    r = rng.random(12) * 3
    lens = rng.integers(1, 27, 12)
    adv, st = emul_scst_advantage(r, lens, None, 4)
    R = r.reshape(3, 4)
    b = np.array([(R[i].sum() - R[i, j]) / 3 for i in range(3) for j in range(4)])
    assert np.allclose(adv, (r - b).astype(np.float32), rtol=0, atol=1e-6)
    assert np.allclose(st, [r.mean(), b.mean(), lens.mean()], rtol=0, atol=1e-12)

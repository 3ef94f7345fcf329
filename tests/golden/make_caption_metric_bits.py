"""Records tests/golden/caption_metric_bits.npz: the outputs of the caption-metric kernels (dlsg_cider_d, _caption_metrics,
_caption_corpus, _scst_advantage, _cider_consensus) and of the gradient-clipping pair (dlsg_grad_sumsq + _clip_coef) on seeded
cases, as computed on an MI355X by the commit BEFORE the three row kernels were rebuilt from the shared front end of
csrc/ngram.hpp and the reductions moved to csrc/common.hpp.  tests/test_gpu_caption_metric_bits.py runs the same launches on
the tree and compares every bit, so the fixture is recorded once from that parent build and never from the tree under test:
check the parent out into a scratch worktree, `make` its csrc/, and run this file under one `timeout` with that worktree's
d-lsg-video-caption_amd on PYTHONPATH (the case list comes from this file, the kernels, `HipOps` and the tables from the parent).

The inputs are built here from seeds, so only outputs are stored: per kernel and output one array, the launches' results
concatenated in the order of `cases()`; float64 as its int64 bit pattern, float32 as int32.  None of the kernels uses an
atomic: every element of every output is compared, the ones a launch leaves alone included."""
import functools
import math
import os
import random
import sys

import numpy as np
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.hip import GRAD_SUMSQ_SLOTS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'caption_metric_bits.npz')
KERNELS = ('cider_d', 'caption_metrics', 'caption_corpus', 'scst_advantage', 'cider_consensus', 'grad_clip')
V = 300
LS = (1, 2, 3, 4, 5, 26, 63, 64)
ORDERS = (1, 2, 3, 4)
PAD = 3                                  # columns behind the L of a row in its buffer: the launches on a view have a row stride of L + 3
LONG_REF = 2100                          # words of the long reference: over the 2048 of either kernel's LDS stage
LONG_CLIP, EMPTY_CLIP = 'c05', 'c12'
CONS_NS, CONS_LS, CONS_B = (1, 2, 5, 32), (1, 26, 64), 2
SCORE_KINDS = (None, 'finite', 'special')
TEMPERATURES = (0.5, 1.0, math.inf)
CORPUS_ROWS = (1, 15, 350)
ADV_SHAPES = ((3, 5), (70, 5))
GRAD_NS = (1, 5, 1027, 70001)


@functools.lru_cache(maxsize=None)
def corpus():
    """(refs, vocab): 12 clips of 1-6 references of 1-12 words over the 40 most frequent of the 296 words (and one word outside
    the vocabulary), one of them with a reference of LONG_REF words over all 296, and a 13th clip without references"""
    rng = random.Random(2024)
    vocab = dlsg_amd.make_vocab(V)
    words = ['w%d' % i for i in range(V - 4)]
    common = words[:40] + ['not-a-word']
    weights = [1.0 / (i + 1) for i in range(len(common) - 1)] + [0.05]
    refs = {}
    for c in range(12):
        refs['c%02d' % c] = [' '.join(rng.choices(common, weights, k=rng.randint(1, 12))) for _ in range(rng.randint(1, 6))]
    refs[LONG_CLIP] = refs[LONG_CLIP][:2] + [' '.join(rng.choice(words) for _ in range(LONG_REF))] + refs[LONG_CLIP][2:4]
    refs[EMPTY_CLIP] = []
    return refs, vocab


@functools.lru_cache(maxsize=None)
def tables(kind, n=4, device='cuda'):
    """the device tables, built once per (kind, n, device) and never written"""
    refs, vocab = corpus()
    return S.DeviceCiderD(refs, vocab, n=n, device=device) if kind == 'cider' else S.DeviceCaptionMetrics(refs, vocab, device=device)


BAD_IDS = (-1, V, 1 << 40)
ROW_KINDS = ('end0', 'end1', 'end2', 'end3', 'end4', 'noend', 'ref', 'ref_fifth', 'rep1', 'per2', 'per3', 'random') + tuple(
    '%s%d' % (k, b) for k in ('oov_first', 'oov_last', 'oov_adjacent', 'oov_alone', 'oov_after_end') for b in range(len(BAD_IDS))) + (
    'clip_below', 'clip_above')


@functools.lru_cache(maxsize=None)
def rows(L):
    """(ids (R, L + PAD) int64 host tensor, clip_idx (R,) int32 host tensor): one row per ROW_KINDS in [:, :L], the clips dealt
    round-robin (the one without references included), the words drawn from the clip's references.  Behind a row's <end> come
    seeded ids, <end> among them; the PAD columns hold <end> (a scan that ran past L would end the row there)"""
    refs, vocab = corpus()
    rng = random.Random(500 + L)
    end = vocab('<end>')
    vids = sorted(refs)
    ids = torch.full((len(ROW_KINDS), L + PAD), end, dtype=torch.int64)
    clip_idx = torch.zeros(len(ROW_KINDS), dtype=torch.int32)
    for r, kind in enumerate(ROW_KINDS):
        c = r % len(vids)
        ref = (refs[vids[c]] or refs[vids[0]])[0]
        ref = [vocab(w) for w in ref.split()]
        pool = [w for w in ref if w != vocab('<unk>')] or [4]
        draw = [rng.choice(pool) for _ in range(L)]
        closed = True
        if kind.startswith('end'):
            words = draw[:int(kind[3:])]
        elif kind == 'noend':
            words, closed = draw, False
        elif kind == 'ref':
            words = ref
        elif kind == 'ref_fifth':
            words = [rng.randrange(4, V) if i % 5 == 2 else w for i, w in enumerate(ref)]
        elif kind == 'rep1':
            words, closed = [pool[0]] * L, False
        elif kind in ('per2', 'per3'):
            p = int(kind[3:])
            words, closed = [list(dict.fromkeys(pool + [5, 6, 7]))[i % p] for i in range(L)], False
        elif kind.startswith('oov'):
            bad = BAD_IDS[int(kind[-1])]
            words = draw[:min(7, max(L - 2, 1))]
            if kind.startswith('oov_first') and words:
                words[0] = bad
            elif kind.startswith('oov_last') and words:
                words[-1] = bad
            elif kind.startswith('oov_adjacent') and len(words) >= 3:
                words[1] = words[2] = bad
            elif kind.startswith('oov_alone'):
                words = [bad]
        else:
            words = draw[:rng.randint(2, 12)]
        row = list(words)[:L]
        if closed and len(row) < L:
            row.append(end)
            fill = BAD_IDS[int(kind[-1])] if kind.startswith('oov_after_end') else None
            row += [fill if fill is not None else rng.randrange(V) for _ in range(L - len(row))]
        ids[r, :L] = torch.tensor(row, dtype=torch.int64)
        clip_idx[r] = -1 if kind == 'clip_below' else len(vids) if kind == 'clip_above' else c
    return ids, clip_idx


@functools.lru_cache(maxsize=None)
def candidates(n, L):
    """(CONS_B, n, L + PAD) int64 host tensor: per clip, variations of one reference; candidate 1 repeats candidate 0,
    candidates 2 and 3 share an id outside the vocabulary at position 1, candidate 4 has no <end>"""
    refs, vocab = corpus()
    rng = random.Random(9000 + 100 * n + L)
    end = vocab('<end>')
    vids = sorted(refs)
    ids = torch.full((CONS_B, n, L + PAD), end, dtype=torch.int64)
    for b in range(CONS_B):
        ref = [vocab(w) for w in refs[vids[b + 1]][0].split()]
        base = (ref * 3)[:max(6, len(ref))]
        made = []
        for i in range(n):
            words = [rng.choice(base) if rng.random() < 0.25 else w for w in base][:rng.randint(3, len(base))]
            if i == 1:
                words = list(made[0])
            elif i in (2, 3):
                words = list(base)
                words[1] = BAD_IDS[b]
                words = words[:-1] if i == 3 else words
            elif i == 4:
                words = (base * L)[:L]
            made.append(words)
            row = list(words)[:L]
            if len(row) < L:
                row.append(end)
                row += [rng.randrange(V) for _ in range(L - len(row))]
            ids[b, i, :L] = torch.tensor(row, dtype=torch.int64)
    return ids


def candidate_scores(n, kind):
    """(CONS_B, n) float32 log-scores; 'special': one -inf and one NaN among them"""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(70 + n)
    sc = -3 * torch.rand(CONS_B, n, generator=g)
    if kind == 'special':
        sc[0, min(1, n - 1)] = -math.inf
        sc[1, n - 1] = math.nan
    return sc


def cases():
    """(kernel, options) of every launch, in the order the fixture stores them"""
    c = []

    def add(kernel, **o):
        c.append((kernel, o))

    for n in ORDERS:
        for L in LS:
            add('cider_d', n=n, L=L, view=False)
    for L in LS:
        add('cider_d', n=4, L=L, view=True)

    for L in LS:
        for view in (False, True):
            add('caption_metrics', L=L, view=view, outputs=('scores', 'stats', 'reward'), w0=0.5)
    for L in (5, 64):
        for out in ('scores', 'stats'):
            add('caption_metrics', L=L, view=False, outputs=(out,), w0=0.0)
        for w0 in (0.0, 0.5):
            add('caption_metrics', L=L, view=False, outputs=('reward',), w0=w0)

    for R in CORPUS_ROWS:
        for base in (False, True):
            add('caption_corpus', rows=R, base=base)

    for B, n in ADV_SHAPES:
        for greedy in (True, False):
            add('scst_advantage', B=B, n=n, greedy=greedy)

    for n in CONS_NS:
        for L in CONS_LS:
            for i, kind in enumerate(SCORE_KINDS):
                add('cider_consensus', n=n, L=L, scores=kind, temperature=TEMPERATURES[(i + 1) % 3], util=i != 1, view=i == 2)
    for kind in SCORE_KINDS:
        for temperature in TEMPERATURES:
            for util in (True, False):
                add('cider_consensus', n=5, L=26, scores=kind, temperature=temperature, util=util, view=False)

    for n in GRAD_NS:
        add('grad_clip', n=n, inf=False)
    add('grad_clip', n=1027, inf=True)
    return c


def run_launch(ops, i, kernel, o):
    """launch number i on fresh output arrays -> {output: CPU tensor}"""
    f64 = dict(dtype=torch.float64, device='cuda')
    g = torch.Generator().manual_seed(4100 + i)
    if kernel in ('cider_d', 'caption_metrics'):
        ids, clip_idx = rows(o['L'])
        R = ids.shape[0]
        ids = ids.cuda()[:, :o['L']] if o['view'] else ids[:, :o['L']].contiguous().cuda()
        assert ids.is_contiguous() != o['view']
        clip_idx = clip_idx.cuda()
        if kernel == 'cider_d':
            tb = tables('cider', o['n'])
            out = torch.full((R,), -7.0, **f64)
            ops.cider_d(ids, clip_idx, tb.end_id, tb, out)
            return {'scores': out.cpu()}
        tb = tables('metrics')
        res = {}
        if 'scores' in o['outputs']:
            res['scores'] = torch.full((R, 5), -7.0, **f64)
        if 'stats' in o['outputs']:
            res['stats'] = torch.full((R, 10), -7, dtype=torch.int32, device='cuda')
        weights = base = None
        if 'reward' in o['outputs']:
            res['reward'] = torch.full((R,), -7.0, **f64)
            weights = [o['w0'], 0.25, 0.0, 0.5, 2.0, 1.0]
            base = torch.rand(R, generator=g, dtype=torch.float64).cuda() if o['w0'] else None
        ops.caption_metrics(ids, clip_idx, tb.end_id, tb, weights=weights, base=base, **res)
        return {n: v.cpu() for n, v in res.items()}
    if kernel == 'caption_corpus':
        R = o['rows']
        stats = torch.randint(0, 60, (R, 10), generator=g, dtype=torch.int32).cuda()
        scores = torch.rand(R, 5, generator=g, dtype=torch.float64).cuda()
        base = torch.rand(R, generator=g, dtype=torch.float64).cuda() * 3 if o['base'] else None
        out = torch.full((6,), -7.0, **f64)
        ops.caption_corpus(stats, scores, base, out)
        return {'out': out.cpu()}
    if kernel == 'scst_advantage':
        B, n = o['B'], o['n']
        rewards = torch.rand(B * n, generator=g, dtype=torch.float64).cuda() * 3
        lens = torch.randint(1, 27, (B * n,), generator=g).cuda()
        greedy = torch.rand(B, generator=g, dtype=torch.float64).cuda() * 3 if o['greedy'] else None
        adv = torch.full((B * n,), -7.0, device='cuda')
        stats = torch.full((3,), -7.0, **f64)
        ops.scst_advantage(rewards, lens, greedy, n, adv, stats)
        return {'adv': adv.cpu(), 'stats': stats.cpu()}
    if kernel == 'cider_consensus':
        n, L = o['n'], o['L']
        tb = tables('cider', 4)
        ids = candidates(n, L)
        ids = ids.cuda()[:, :, :L] if o['view'] else ids[:, :, :L].contiguous().cuda()
        sc = candidate_scores(n, o['scores'])
        res = {'expected': torch.full((CONS_B, n), -7.0, **f64), 'order': torch.full((CONS_B, n), -7, dtype=torch.int64, device='cuda')}
        if o['util']:
            res['util'] = torch.full((CONS_B, n, n), -7.0, **f64)
        ops.cider_consensus(ids, tb.end_id, tb, None if sc is None else sc.cuda(), o['temperature'], res.get('util'), res['expected'],
                            res['order'])
        return {k: v.cpu() for k, v in res.items()}
    assert kernel == 'grad_clip'
    n = o['n']
    x = torch.randn(n, generator=g) * 3e-2
    if o['inf']:
        x[n // 2] = math.inf
    buf = torch.zeros(n + 12, device='cuda')
    view = buf[5:5 + n]                                          # one float past a 16-byte boundary
    assert view.data_ptr() % 16 == 4
    view.copy_(x)
    slots = torch.full((GRAD_SUMSQ_SLOTS,), math.nan, **f64)
    record = torch.full((4,), -1.0, device='cuda')
    skipped = torch.zeros(1, dtype=torch.int64, device='cuda')
    ops.grad_sumsq(view, slots)
    ops.clip_coef(slots, 0.25, 1.0, record, skipped)
    return {'slots': slots.cpu(), 'record': record.cpu(), 'skipped': skipped.cpu()}


def run_all(ops):
    """every launch of `cases()` -> {kernel: [(label, {output: CPU tensor})]}"""
    res = {kn: [] for kn in KERNELS}
    for i, (kernel, o) in enumerate(cases()):
        res[kernel].append(('%d: %s %r' % (i, kernel, sorted(o.items(), key=str)), run_launch(ops, i, kernel, o)))
    return res


def as_stored(x):
    """the array of one output as the fixture keeps it: floats as their bits, so that -inf and NaN compare as well"""
    x = x.contiguous().view(-1)
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def stored_arrays(res):
    """{'<kernel>.<output>': the launches that have the output, concatenated in case order}"""
    arrays = {}
    for kn, runs in res.items():
        for _, o in runs:
            for n, x in o.items():
                arrays.setdefault('%s.%s' % (kn, n), []).append(as_stored(x))
    return {n: torch.cat(xs) for n, xs in arrays.items()}


def main():
    from dlsg_amd.hip import HipOps
    print('recording with', os.path.dirname(dlsg_amd.__file__))
    res = run_all(HipOps())
    for kn, runs in res.items():
        print(kn, len(runs), 'launches')
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, **{n: x.numpy() for n, x in stored_arrays(res).items()})


if __name__ == '__main__':
    main()

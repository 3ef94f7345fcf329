"""Records tests/golden/word_choice_bits.npz: the outputs of the five kernels that pick a word from a row of logits and write its
embedding (dlsg_argmax, _embed_fwd, _select_embed, _sample_embed, _sample_filter_embed) on seeded cases, as computed on an
MI355X by the commit BEFORE the kernels were rebuilt from shared phases (csrc/wordpick.hpp).  tests/test_gpu_word_choice_bits.py
runs the same launches on the tree and compares every bit, so the fixture is recorded once from that parent build and never from
the tree under test: check the parent out into a scratch worktree, `make` its csrc/, and run this file under one `timeout` with
that worktree's d-lsg-video-caption_amd on PYTHONPATH (the case list comes from this file, the kernels and `HipOps` from the
parent).

The inputs are built here from seeds, so only outputs are stored: per kernel and output one array, the launches' results
concatenated in the order of `cases()`; float32 as its int32 bit pattern.  None of the kernels uses an atomic: every element
of every output buffer is compared, the padding of a strided `out` and the rows a launch leaves alone included."""
import functools
import os
import sys

import numpy as np
import torch

from dlsg_amd.hip import SAMPLE_FILTER_MAXV

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'word_choice_bits.npz')
KERNELS = ('argmax', 'embed_fwd', 'select_embed', 'sample_embed', 'sample_filter_embed')
VS = (1, 40, 64, 257, 1000, 10007)      # one word, below a wave, a wave, one past the workgroup's stride, ..., no multiple of anything
ROW_KINDS = ('random', 'nan', 'neg_inf', 'equal', 'tie', 'some_nan', 'some_neg_inf', 'signed_zero', 'random_again')
L = 26                                   # caption length the `lens` of a sampled step start from
SITE_WORD, SITE_SAMPLE = 3, 5


@functools.lru_cache(maxsize=None)
def logits_block(V):
    """(9, V + 3) host logits (cached: read only), one row per ROW_KINDS; the launches read [:, :V], so the row stride is larger
    than V, and the three columns behind hold a value above every logit (a scan that ran past V would choose it)"""
    g = torch.Generator().manual_seed(1000 + V)
    x = torch.randn(len(ROW_KINDS), V + 3, generator=g) * 3
    x[1] = float('nan')
    x[2] = float('-inf')
    x[3] = 0.25
    x[4, min(3, V - 1)] = x[4, max(V - 2, 0)] = 50.0           # the maximum twice, at a low and a high index
    x[5, 2::7] = float('nan')
    x[6, 1::5] = float('-inf')
    x[7] = -x[7].abs() - 0.5                                    # the maximum is 0: -0.0 first, +0.0 behind it
    a = max(V // 2 - 1, 0)
    x[7, a] = -0.0
    x[7, min(a + 1, V - 1)] = 0.0 if V > 1 else -0.0
    x[8] = x[0]                                                 # row 0 again: the same choice at tau = 0, another `lens` preset
    x[:, V:] = 100.0
    return x


def end_word(V):
    """<end> = the first maximum of row 0 (and of row 8): a greedy step ends those rows"""
    return int(torch.argmax(logits_block(V)[0, :V]))


def table(n, W):
    """(n, W) embedding table of exact sixteenths, no two alike in a row or a column"""
    i, j = torch.arange(n)[:, None], torch.arange(W)[None, :]
    return ((i * 131 + j * 7) % 4093 - 2046).float() / 16


def history(V, rows):
    """(8, rows) time-major earlier words: even rows a, b, a, b, ... with a, b the row's two best words (so bigrams and trigrams
    repeat, and the ban hits the words the row would choose), odd rows seeded words that differ from row to row"""
    x = torch.nan_to_num(logits_block(V)[:, :V], nan=float('-inf'))
    top = torch.topk(x, min(2, V), dim=1).indices
    g = torch.Generator().manual_seed(77 + V)
    h = torch.randint(0, V, (8, len(ROW_KINDS)), generator=g)
    for r in range(0, len(ROW_KINDS), 2):
        h[0::2, r] = top[r, 0]
        h[1::2, r] = top[r, -1]
    return h[:, list(rows)].contiguous()


def cases():
    """(kernel, options) of every launch, in the order the fixture stores them"""
    c = []

    def add(kernel, **o):
        c.append((kernel, o))

    for V in VS:
        add('argmax', V=V)

    for p in (0.0, 0.3):
        for row0 in (0, 128):
            for W, ldo, rows in ((8, 8, 8), (20, 24, 8), (300, 300, 2)):   # (W = 300: past the workgroup's stride, two rows do)
                add('embed_fwd', W=W, ldo=ldo, rows=rows, p=p, row0=row0, seed_on_device=False)
    add('embed_fwd', W=20, ldo=24, rows=8, p=0.3, row0=128, seed_on_device=True)

    for coin in (0, 1):
        for prefilled in (0, 1):
            for t in (0, 2):
                for p in (0.0, 0.3):
                    add('select_embed', V=1000, coin=coin, prefilled=prefilled, t=t, p=p)
    for V in VS:
        if V != 1000:
            add('select_embed', V=V, coin=0, prefilled=0, t=2, p=0.3)

    plain = [dict(V=V, tau=tau, p=p) for V in VS for tau in (0.0, 0.7, 1.0) for p in (0.0, 0.3)]
    for o in plain:
        add('sample_embed', row0=64, t=2, **o)
    add('sample_embed', V=1000, tau=0.7, p=0.3, row0=0, t=2)

    def filt(**o):
        add('sample_filter_embed', **dict(dict(tau=0.7, p=0.0, row0=64, t=2, top_k=0, top_p=1.0, min_len=0, g=0, kept=True, rows=None), **o))

    for i, o in enumerate(plain):                                # every control off: sample_embed's cases
        filt(kept=i % 2 == 0, **o)
    for V in VS:
        for k in (1, 5, 50, V + 10):
            filt(V=V, top_k=k, p=0.3 if k == 5 else 0.0, kept=k != 50)
    for V in VS:
        for top_p in (0.9, 0.5, 1e-6):
            filt(V=V, tau=1.0, top_p=top_p)
    for V in VS:
        for k, top_p in ((50, 0.9), (5, 0.5)):
            filt(V=V, top_k=k, top_p=top_p, p=0.3)
    filt(V=1000, tau=0.0, top_k=5, top_p=0.5)                    # greedy: the thresholds are not searched
    for k, top_p in ((50, 1.0), (0, 0.9), (50, 0.9)):
        filt(V=SAMPLE_FILTER_MAXV, rows=(0, 4), top_k=k, top_p=top_p)
    for V in (1, 40, 1000):                                      # <end> is the maximum of rows 0 and 8: banned at t = 2, not at t = 3
        for tau in (0.0, 1.0):
            for t in (2, 3):
                filt(V=V, tau=tau, t=t, min_len=3)
    for V in (40, 1000):
        for g in (1, 2, 3):
            for t in (0, 2, 5):
                for tau, k in ((0.0, 0), (0.7, 0), (0.7, 5)):
                    filt(V=V, g=g, t=t, tau=tau, top_k=k)
    return c


_cache = {}


def _dev(name, make, *a):
    """a host-built input on the device, made once and never written"""
    if (name,) + a not in _cache:
        _cache[(name,) + a] = make(*a).cuda()
    return _cache[(name,) + a]


def run_launch(ops, i, kernel, o):
    """launch number i on fresh output arrays -> {output: CPU tensor}"""
    seed = 20261 + i
    f32 = dict(dtype=torch.float32, device='cuda')
    i64 = dict(dtype=torch.int64, device='cuda')
    if kernel == 'embed_fwd':
        rows, W = o['rows'], o['W']
        ids = torch.randint(0, 50, (rows,), generator=torch.Generator().manual_seed(seed)).cuda()
        out = torch.full((rows, o['ldo']), -7.0, **f32)
        sd = torch.tensor([seed], **i64) if o['seed_on_device'] else seed
        ops.embed_fwd(_dev('table', table, 50, W), ids, out[:, :W], p=o['p'], seed=sd, site=SITE_WORD, row0=o['row0'])
        return {'out': out.cpu()}
    V = o['V']
    x = _dev('logits', logits_block, V)
    if o.get('rows'):
        x = x[list(o['rows'])]
    x, rows = x[:, :V], x.shape[0]
    ids = torch.full((rows,), -1, **i64)
    if kernel == 'argmax':
        ops.argmax(x, ids)
        return {'ids': ids.cpu()}
    E = _dev('table', table, V, 8)
    out = torch.full((rows, 12), -7.0, **f32)                    # W = 8 in rows of 12
    if kernel == 'select_embed':
        caps = torch.randint(0, V, (rows, 3), generator=torch.Generator().manual_seed(seed)).cuda()
        coins = torch.zeros(3, dtype=torch.int32)
        coins[o['t']] = o['coin']
        ops.select_embed(x, caps, o['t'], coins.cuda(), E, ids, out[:, :8], p=o['p'], seed=seed, site=SITE_WORD, row0=32,
                         prefilled=o['prefilled'])
        return {'ids': ids.cpu(), 'out': out.cpu()}
    t = o['t']
    lens = torch.tensor([L, 1, L, 2, L, 0, L, 3, t])             # both sides of lens[r] > t; row 8 ends where row 0 does, and stays
    lens = (lens[list(o['rows'])] if o.get('rows') else lens).cuda()
    logp = torch.full((rows,), -7.0, **f32)
    res = {'ids': ids, 'out': out, 'logp': logp, 'lens': lens}
    common = dict(temperature=o['tau'], p=o['p'], seed=seed, site=SITE_WORD, site_sample=SITE_SAMPLE, row0=o['row0'])
    if kernel == 'sample_embed':
        ops.sample_embed(x, E, ids, out[:, :8], logp, lens, t, end_word(V), **common)
    else:
        if o['kept']:
            res['kept'] = torch.full((rows,), -1, dtype=torch.int32, device='cuda')
        hist = _dev('history', history, V, tuple(o['rows'] or range(len(ROW_KINDS)))) if o['g'] else None
        ops.sample_filter_embed(x, E, ids, out[:, :8], logp, lens, t, end_word(V), top_k=o['top_k'], top_p=o['top_p'],
                                min_len=o['min_len'], no_repeat_ngram=o['g'], hist=hist, kept=res.get('kept'), **common)
    return {n: v.cpu() for n, v in res.items()}


def run_all(ops):
    """every launch of `cases()` -> {kernel: [(label, {output: CPU tensor})]}"""
    res = {kn: [] for kn in KERNELS}
    for i, (kernel, o) in enumerate(cases()):
        res[kernel].append(('%d: %s %r' % (i, kernel, sorted(o.items())), run_launch(ops, i, kernel, o)))
    return res


def as_stored(x):
    """the array of one output as the fixture keeps it: float32 as its bits, so that -inf and NaN compare as well"""
    x = x.contiguous().view(-1)
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def stored_arrays(res):
    """{'<kernel>_<output>': the launches that have the output, concatenated in case order}"""
    arrays = {}
    for kn, runs in res.items():
        for _, o in runs:
            for n, x in o.items():
                arrays.setdefault('%s_%s' % (kn, n), []).append(as_stored(x))
    return {n: torch.cat(xs) for n, xs in arrays.items()}


def main():
    from dlsg_amd.hip import HipOps
    import dlsg_amd
    print('recording with', os.path.dirname(dlsg_amd.__file__))
    res = run_all(HipOps())
    for kn, runs in res.items():
        print(kn, len(runs), 'launches')
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, **{n: x.numpy() for n, x in stored_arrays(res).items()})


if __name__ == '__main__':
    main()

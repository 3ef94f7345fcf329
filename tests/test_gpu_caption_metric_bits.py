"""GPU (-m gpu): the caption-metric kernels (dlsg_cider_d, _caption_metrics, _caption_corpus, _scst_advantage, _cider_consensus)
and the gradient-clipping pair return, bit for bit, what they returned before the three row kernels were rebuilt from the shared
front end of csrc/ngram.hpp and the fixed-order reductions moved to csrc/common.hpp.  tests/golden/caption_metric_bits.npz was
recorded on an MI355X from the parent of that change by tests/golden/make_caption_metric_bits.py, whose case list and launches
this file runs again.  A mismatch is a fault of the kernels: the fixture is not re-recorded from the tree.  The CPU test checks
that the case list covers what the front end and the reductions can get wrong, and that the rows are not trivial."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from emul_ngram import row_ngrams
from test_cider_device_host import emul_cider_d

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_caption_metric_bits', os.path.join(HERE, 'golden', 'make_caption_metric_bits.py'))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def test_the_cases_cover_the_front_end_and_the_reductions():
    by = {kn: [o for k, o in rec.cases() if k == kn] for kn in rec.KERNELS}

    def seen(kn, *names):
        return {tuple(o[n] for n in names) for o in by[kn]}

    # ---- the corpus
    refs, vocab = rec.corpus()
    V, end = len(vocab), vocab('<end>')
    assert V == rec.V == 300 and len(refs) == 13 and refs[rec.EMPTY_CLIP] == []
    scorable = [v for v in sorted(refs) if v != rec.EMPTY_CLIP]
    assert {len(refs[v]) for v in scorable} <= set(range(1, 7)) and len({len(refs[v]) for v in scorable}) >= 4
    lens = [len(r.split()) for v in scorable for r in refs[v]]
    assert min(lens) == 1 and sorted(lens)[-2] <= 12 and max(lens) == rec.LONG_REF > dlsg_stage()
    assert lens.count(rec.LONG_REF) == 1 and max(len(r.split()) for r in refs[rec.LONG_CLIP]) == rec.LONG_REF
    for n in rec.ORDERS:
        tb = rec.tables('cider', n, 'cpu')
        assert tb.n == n
        c = tb.vids.index(rec.LONG_CLIP)
        per_ref = tb.ref_off[tb.clip_off[c] + 1:tb.clip_off[c + 1] + 1] - tb.ref_off[tb.clip_off[c]:tb.clip_off[c + 1]]
        assert n == 1 or per_ref.max() > 2048                    # alone over one LDS stage of cider_d_kernel (not with 296 unigrams)
        e = tb.vids.index(rec.EMPTY_CLIP)
        assert tb.clip_off[e] == tb.clip_off[e + 1]
    # ---- the rows of every length
    assert rec.LS == (1, 2, 3, 4, 5, 26, 63, 64)
    stats = dict(tf=0, unfirst=0, kbad=0)
    for L in rec.LS:
        ids, clip_idx = rec.rows(L)
        assert ids.shape == (len(rec.ROW_KINDS), L + rec.PAD) and ids[:, :L].stride(0) > L
        rows = dict(zip(rec.ROW_KINDS, ids[:, :L].tolist()))
        length = {k: (r.index(end) if end in r else L) for k, r in rows.items()}
        assert length['end0'] == 0 and length['noend'] == L and all(length['end%d' % p] == min(p, L) for p in range(1, 5))
        assert len(set(rows['rep1'])) == 1 and length['rep1'] == L
        assert row_ngrams(ids[rec.ROW_KINDS.index('rep1'), :L], end, V, 0).tf == [L] * L
        for p in (2, 3):
            r = rows['per%d' % p]
            assert length['per%d' % p] == L and r[p:] == r[:max(L - p, 0)] and (L < p or len(set(r[:p])) == p)
        for b, bad in enumerate(rec.BAD_IDS):
            assert rows['oov_alone%d' % b][0] == bad and length['oov_alone%d' % b] == min(1, L) or L == 1
            if L >= 5:
                r = rows['oov_first%d' % b]
                assert r[0] == bad and all(0 <= x < V for x in r[1:length['oov_first%d' % b]])
                r = rows['oov_last%d' % b]
                assert r[length['oov_last%d' % b] - 1] == bad and r[length['oov_last%d' % b]] == end
                r = rows['oov_adjacent%d' % b]
                assert r[1] == r[2] == bad
                r, n = rows['oov_after_end%d' % b], length['oov_after_end%d' % b]
                assert all(0 <= x < V for x in r[:n]) and n < L - 1 and set(r[n + 1:]) == {bad}
        vids = sorted(refs)
        ref = [vocab(w) for w in refs[vids[clip_idx[rec.ROW_KINDS.index('ref')]]][0].split()]
        assert rows['ref'][:length['ref']] == ref[:L]
        if L >= 26:
            fifth = rows['ref_fifth']
            ref = [vocab(w) for w in refs[vids[clip_idx[rec.ROW_KINDS.index('ref_fifth')]]][0].split()]
            changed = sum(a != b for a, b in zip(fifth, ref))
            assert length['ref_fifth'] == len(ref) and (len(ref) < 3 or 0 < changed <= (len(ref) + 4) // 5)
        assert clip_idx[-2] == -1 and clip_idx[-1] == len(vids) and (clip_idx == vids.index(rec.EMPTY_CLIP)).any()
        assert set(clip_idx[:-2].tolist()) == set(range(len(vids)))
        for r in ids[:, :L]:
            for k in range(4):
                g = row_ngrams(r, end, V, k)
                stats['tf'] += any(t > 1 for t in g.tf)
                stats['unfirst'] += not all(g.first)
                stats['kbad'] += any(g.kbad)
    assert min(stats.values()) >= 10, stats                          # repeats, positions that are not first, keys with a bad word
    # ---- not trivially zero: CIDEr-D of the rows by the emulator
    tb = rec.tables('cider', 4, 'cpu')
    for L in (5, 26, 64):
        ids, clip_idx = rec.rows(L)
        sc = emul_cider_d(tb, ids[:, :L], clip_idx, tb.end_id)
        assert np.isnan(sc).sum() >= 3 and (sc > 0).sum() * 3 >= np.isfinite(sc).sum(), (L, sc)
    # ---- the launches
    assert seen('cider_d', 'n', 'L') >= {(n, L) for n in (1, 2, 3, 4) for L in rec.LS}
    assert {L for (L, v) in seen('cider_d', 'L', 'view') if v} == set(rec.LS)
    whole = ('scores', 'stats', 'reward')
    assert {(L, v) for (L, v, o) in seen('caption_metrics', 'L', 'view', 'outputs') if o == whole} == {(L, v) for L in rec.LS for v in (False, True)}
    assert {o for (o,) in seen('caption_metrics', 'outputs')} == {whole, ('scores',), ('stats',), ('reward',)}
    assert {w0 for (o, w0) in seen('caption_metrics', 'outputs', 'w0') if o == ('reward',)} == {0.0, 0.5}
    assert seen('caption_corpus', 'rows', 'base') == {(R, b) for R in (1, 15, 350) for b in (False, True)}
    assert seen('scst_advantage', 'B', 'n', 'greedy') == {(B, 5, g) for B in (3, 70) for g in (False, True)}
    assert all((B * n) % 256 for B, n in rec.ADV_SHAPES)
    assert seen('cider_consensus', 'n', 'L') == {(n, L) for n in (1, 2, 5, 32) for L in (1, 26, 64)}
    for names, values in (('scores', rec.SCORE_KINDS), ('temperature', (0.5, 1.0, math.inf)), ('util', (True, False))):
        assert {v for (v,) in seen('cider_consensus', names)} == set(values)
    assert seen('cider_consensus', 'scores', 'temperature', 'util') == {(s, t, u) for s in rec.SCORE_KINDS for t in rec.TEMPERATURES
                                                                        for u in (True, False)}
    assert any(o['view'] for o in by['cider_consensus'])
    for n in (5, 32):
        for L in (26, 64):
            c = rec.candidates(n, L)[:, :, :L]
            for b in range(rec.CONS_B):
                w = [r[:r.index(end)] if end in r else r for r in c[b].tolist()]     # the candidates' words
                assert w[0] == w[1] and w[0] != w[2] and w[2][1] == w[3][1] == rec.BAD_IDS[b] and w[2] != w[3]
            assert (c[:, 4] != end).all()
    sp = rec.candidate_scores(5, 'special')
    assert sp.isneginf().sum() == 1 and sp.isnan().sum() == 1 and rec.candidate_scores(5, 'finite').isfinite().all()
    assert seen('grad_clip', 'n', 'inf') == {(1, False), (5, False), (1027, False), (70001, False), (1027, True)}
    assert os.path.getsize(rec.FIXTURE) < 256 * 1024


def dlsg_stage():
    from dlsg_amd import abi
    return abi.defines['DLSG_METRICS_STAGE']


@pytest.fixture(scope='module')
def tree_results():
    from dlsg_amd.hip import HipOps
    return rec.run_all(HipOps())


@gpu
@pytest.mark.parametrize('kernel', rec.KERNELS)
def test_the_caption_metric_kernels_keep_their_recorded_bits(tree_results, kernel):
    runs = tree_results[kernel]
    with np.load(rec.FIXTURE) as f:                                  # (each array is decompressed once)
        want = {n[len(kernel) + 1:]: f[n] for n in f.files if n.startswith(kernel + '.')}
    assert set(want) == {n for _, got in runs for n in got}
    at = {n: 0 for n in want}
    for label, got in runs:
        for n, x in got.items():
            w = torch.from_numpy(want[n][at[n]:at[n] + x.numel()])
            at[n] += x.numel()
            assert torch.equal(rec.as_stored(x), w), (label, n)
    for n, end in at.items():
        assert end == want[n].size, (kernel, n)

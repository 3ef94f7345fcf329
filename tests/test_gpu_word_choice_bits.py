"""GPU (-m gpu): the five kernels that pick a word from a row of logits and write its embedding return, bit for bit, what they
returned before they were rebuilt from the shared phases of csrc/wordpick.hpp.  tests/golden/word_choice_bits.npz was recorded on
an MI355X from the parent of that change by tests/golden/make_word_choice_bits.py, whose case list and launches this file runs
again.  The tests that compare the filtered sampler with the plain one, and both with argmax, now compare code with itself; this
fixture is what ties the kernels to their earlier results.  A mismatch is a fault of the kernels: the fixture is not re-recorded
from the tree."""
import importlib.util
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_word_choice_bits', os.path.join(HERE, 'golden', 'make_word_choice_bits.py'))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def test_the_cases_cover_every_size_row_kind_and_option():
    by = {kn: [o for k, o in rec.cases() if k == kn] for kn in rec.KERNELS}

    def seen(kn, *names):
        return {tuple(o[n] for n in names) for o in by[kn]}

    # ---- the rows of every logits block, and its stride
    for V in rec.VS + (rec.SAMPLE_FILTER_MAXV,):
        x = rec.logits_block(V)
        assert x.stride(0) > V
        x = x[:, :V]
        assert x[1].isnan().all() and (x[2] == float('-inf')).all() and (x[3] == x[3, 0]).all()
        top = (x[4] == x[4].max()).nonzero().view(-1).tolist()
        assert top == sorted({min(3, V - 1), max(V - 2, 0)})
        assert torch.equal(x[8], x[0]) and x[0].isfinite().all()
        if V >= 40:
            assert len(top) == 2
            assert x[5].isnan().any() and x[5].isfinite().any() and (x[6] == float('-inf')).any() and x[6].isfinite().any()
            z = (x[7] == 0).nonzero().view(-1).tolist()
            assert len(z) == 2 and z[1] == z[0] + 1 and x[7].max() == 0
            assert torch.signbit(x[7, z[0]]) and not torch.signbit(x[7, z[1]])
    # ---- vocabulary sizes
    assert rec.VS == (1, 40, 64, 257, 1000, 10007)
    for kn in ('argmax', 'select_embed', 'sample_embed', 'sample_filter_embed'):
        assert seen(kn, 'V') >= {(V,) for V in rec.VS}, kn
    assert {o['V'] for kn in by if kn != 'embed_fwd' for o in by[kn] if o['V'] > 10007} == {rec.SAMPLE_FILTER_MAXV}
    assert all(len(o['rows']) == 2 for o in by['sample_filter_embed'] if o['V'] == rec.SAMPLE_FILTER_MAXV)
    assert seen('sample_embed', 'V') == {(V,) for V in rec.VS}
    # ---- embed_fwd
    assert seen('embed_fwd', 'p', 'row0', 'W') >= {(p, r0, W) for p in (0.0, 0.3) for r0 in (0, 128) for W in (8, 20, 300)}
    assert all(o['ldo'] > o['W'] for o in by['embed_fwd'] if o['W'] == 20)
    assert sum(o['seed_on_device'] for o in by['embed_fwd']) == 1
    # ---- select_embed
    assert seen('select_embed', 'coin', 'prefilled', 't', 'p') >= {(c, f, t, p) for c in (0, 1) for f in (0, 1) for t in (0, 2)
                                                                   for p in (0.0, 0.3)}
    # ---- sample_embed, and the same cases through the filtered kernel with every control off
    plain = {(V, tau, p) for V in rec.VS for tau in (0.0, 0.7, 1.0) for p in (0.0, 0.3)}
    assert seen('sample_embed', 'V', 'tau', 'p') >= plain
    assert all(o['row0'] != 0 for o in by['sample_embed'][:len(plain)])
    off = [o for o in by['sample_filter_embed'] if (o['top_k'], o['top_p'], o['min_len'], o['g']) == (0, 1.0, 0, 0)]
    assert {(o['V'], o['tau'], o['p']) for o in off} >= plain
    assert {o['kept'] for o in off} == {True, False}
    for V in rec.VS:                                                         # lens is written: a greedy step ends rows 0 and 8
        assert rec.end_word(V) == int(torch.argmax(rec.logits_block(V)[8, :V]))
    # ---- sample_filter_embed's controls
    for V in rec.VS:
        assert {k for (v, k, tp) in seen('sample_filter_embed', 'V', 'top_k', 'top_p') if v == V and tp == 1.0} >= {1, 5, 50, V + 10}
        assert {tp for (v, k, tp) in seen('sample_filter_embed', 'V', 'top_k', 'top_p') if v == V and k == 0} >= {0.9, 0.5, 1e-6}
        assert any(k > 0 and tp < 1.0 for (v, k, tp) in seen('sample_filter_embed', 'V', 'top_k', 'top_p') if v == V)
    assert seen('sample_filter_embed', 'min_len', 't') >= {(3, 2), (3, 3)}
    assert seen('sample_filter_embed', 'g', 't') >= {(g, t) for g in (1, 2, 3) for t in (0, 2, 5)}
    h = rec.history(1000, range(len(rec.ROW_KINDS)))
    assert torch.equal(h[0::2, 0], h[0, 0].expand(4)) and torch.equal(h[1::2, 0], h[1, 0].expand(4)) and h[0, 0] != h[1, 0]
    assert len({tuple(h[:, r].tolist()) for r in range(h.shape[1])}) > 5
    assert os.path.getsize(rec.FIXTURE) < 256 * 1024


@pytest.fixture(scope='module')
def tree_results():
    from dlsg_amd.hip import HipOps
    return rec.run_all(HipOps())


@gpu
@pytest.mark.parametrize('kernel', rec.KERNELS)
def test_the_word_choice_kernels_keep_their_recorded_bits(tree_results, kernel):
    runs = tree_results[kernel]
    with np.load(rec.FIXTURE) as f:                                  # (each array is decompressed once)
        want = {n[len(kernel) + 1:]: f[n] for n in f.files if n.startswith(kernel + '_')}
    assert set(want) == {n for _, got in runs for n in got}
    at = {n: 0 for n in want}
    for label, got in runs:
        for n, x in got.items():
            w = torch.from_numpy(want[n][at[n]:at[n] + x.numel()])
            at[n] += x.numel()
            assert torch.equal(rec.as_stored(x), w), (label, n)
    for n, end in at.items():
        assert end == want[n].size, (kernel, n)

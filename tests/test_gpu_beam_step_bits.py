"""GPU (-m gpu): the eight beam-search step kernels return, bit for bit, what they returned before they were rebuilt from the shared
phases of csrc/beam.hpp.  tests/golden/beam_step_bits.npz (select, hist, ens, groups) was recorded on an MI355X from the parent of
that change by tests/golden/make_beam_step_bits.py; tests/golden/beam_step_bits2.npz (gumbel, cons) from the parent of the change
that gave the history searches one loop and one emitter, by tests/golden/make_beam_step_bits2.py; tests/golden/beam_step_bits3.npz
(excl, gumbel_excl) from the parent of the change that gave the steps under exclusions shared argument checks and wrappers (and
tried to fold the two kernels into their parents), by tests/golden/make_beam_step_bits3.py.  This file runs the recorders' case
lists and launches again.  The chain tests (hist without bans against plain, one member against hist, one group against ens, no constraints against hist, one beam against sample_embed) compare kernels that share their code with each other; these
fixtures are what ties them to the earlier results.  A mismatch is a fault of the kernels: a fixture is not re-recorded from the
tree."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _recorder(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = sys.modules[name] = importlib.util.module_from_spec(spec)   # (the sibling imports the first one by its name)
    spec.loader.exec_module(mod)
    return mod


rec = _recorder('make_beam_step_bits')
rec2 = _recorder('make_beam_step_bits2')
rec3 = _recorder('make_beam_step_bits3')
RECORDER = dict([(kn, rec) for kn in rec.KERNELS] + [(kn, rec2) for kn in rec2.KERNELS] + [(kn, rec3) for kn in rec3.KERNELS])


def test_the_cases_cover_every_dispatch_and_variant():
    """every K of the dispatch, every kernel at every K (groups: every K that has a divisor above 1), both history lengths; the
    stochastic step at both temperatures with both forms of the seed, the constrained one at all four (C, W); the two steps under
    exclusions at every K under all four kinds of table, the stochastic one with both forms of the seed"""
    seen = {(kn, key[0][1]) for key in rec.step_keys() for kn, _ in rec.launches(key)}
    for k in range(1, 9):
        assert {('select', k), ('hist', k), ('ens', k)} <= seen
        assert (('groups', k) in seen) == (k > 1)
    assert {key[1] for key in rec.step_keys()} == {26, 64}
    assert os.path.getsize(rec.FIXTURE) < 256 * 1024
    # (kernel, option, K, L, g, min_len == 0): every option of both kernels at every K with and without the n-gram ban and a minimum
    # length (L = 64 is trimmed to the steps with the ban, as in the first fixture)
    seen2 = {(kn, opt, key[0][1], key[1], key[2], key[4] == 0) for key in rec2.step_keys() for kn, opt in rec2.launches(key)}
    options = [('gumbel', (temp, form)) for temp in (1.0, 0.7) for form in ('int', 'word')] + \
              [('cons', cw) for cw in ((0, 1), (1, 1), (3, 2), (8, 8))]
    for k in range(1, 9):
        for L, g in ((26, 0), (26, 3), (64, 3)) if k == 8 else ((26, 0), (26, 3)):
            assert {(kn, opt, k, L, g, plain) for kn, opt in options for plain in (True, False)} <= seen2, (k, L, g)
    assert os.path.getsize(rec2.FIXTURE) < 256 * 1024
    # the same for the steps under exclusions: every table kind, and every (M, mode) of the ensemble step
    assert rec3.KERNELS == ('excl', 'gumbel_excl') and rec3.step_keys() == rec.step_keys()
    seen3 = {(kn, opt[:1] if kn == 'excl' else opt, key[0][1], key[1], key[2], key[4] == 0)
             for key in rec3.step_keys() for kn, opt in rec3.launches(key)}
    options = [('excl', (tab,)) for tab in ('empty', 'one', 'mixed', 'full')] + \
              [('gumbel_excl', (tab, form)) for tab in ('empty', 'one', 'mixed', 'full') for form in ('int', 'word')]
    for k in range(1, 9):
        for L, g in ((26, 0), (26, 3), (64, 3)) if k == 8 else ((26, 0), (26, 3)):
            assert {(kn, opt, k, L, g, plain) for kn, opt in options for plain in (True, False)} <= seen3, (k, L, g)
    assert {opt[1:] for key in rec3.step_keys() for kn, opt in rec3.launches(key) if kn == 'excl'} == {(1, 0), (3, 0), (3, 1)}
    assert os.path.getsize(rec3.FIXTURE) < 256 * 1024


@pytest.fixture(scope='module')
def tree_results():
    from dlsg_amd.hip import HipOps
    ops = HipOps()
    return dict(rec.run_all(ops), **rec2.run_all(ops), **rec3.run_all(ops))


@gpu
@pytest.mark.parametrize('kernel', rec.KERNELS + rec2.KERNELS + rec3.KERNELS)
def test_the_step_kernels_keep_their_recorded_bits(tree_results, kernel):
    runs = tree_results[kernel]
    stored = RECORDER[kernel].as_stored
    with np.load(RECORDER[kernel].FIXTURE) as f:                     # (each array is decompressed once)
        want = {n: f['%s_%s' % (kernel, n)] for n in runs[0][1]}
    at = {n: 0 for n in runs[0][1]}
    for label, got in runs:
        for n, x in got.items():
            w = torch.from_numpy(want[n][at[n]:at[n] + x.numel()])
            at[n] += x.numel()
            assert torch.equal(torch.from_numpy(stored(n, x)), w), (label, n)
    for n, end in at.items():
        assert end == want[n].size, (kernel, n)

"""GPU (-m gpu): the four beam-search step kernels return, bit for bit, what they returned before they were rebuilt from the shared
phases of csrc/beam.hpp.  tests/golden/beam_step_bits.npz was recorded on an MI355X from the parent of that change by
tests/golden/make_beam_step_bits.py, whose case list and launches this file runs again.  The chain tests (hist without bans
against plain, one member against hist, one group against ens) compare kernels that now share their code with each other; this
fixture is what ties them to the earlier results.  A mismatch is a fault of the kernels: the fixture is not re-recorded from the
tree."""
import importlib.util
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_beam_step_bits', os.path.join(HERE, 'golden', 'make_beam_step_bits.py'))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def test_the_cases_cover_every_dispatch_and_variant():
    """every K of the dispatch, every kernel at every K (groups: every K that has a divisor above 1), both history lengths"""
    seen = {(kn, key[0][1]) for key in rec.step_keys() for kn, _ in rec.launches(key)}
    for k in range(1, 9):
        assert {('select', k), ('hist', k), ('ens', k)} <= seen
        assert (('groups', k) in seen) == (k > 1)
    assert {key[1] for key in rec.step_keys()} == {26, 64}
    assert os.path.getsize(rec.FIXTURE) < 256 * 1024


@pytest.fixture(scope='module')
def tree_results():
    from dlsg_amd.hip import HipOps
    return rec.run_all(HipOps())


@gpu
@pytest.mark.parametrize('kernel', rec.KERNELS)
def test_the_step_kernels_keep_their_recorded_bits(tree_results, kernel):
    runs = tree_results[kernel]
    with np.load(rec.FIXTURE) as f:                                  # (each array is decompressed once)
        want = {n: f['%s_%s' % (kernel, n)] for n in runs[0][1]}
    at = {n: 0 for n in runs[0][1]}
    for label, got in runs:
        for n, x in got.items():
            w = torch.from_numpy(want[n][at[n]:at[n] + x.numel()])
            at[n] += x.numel()
            x = x.contiguous().view(-1)
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, w), (label, n)
    for n, end in at.items():
        assert end == want[n].size, (kernel, n)

"""CPU: the element-wise gradient comparator of tests/helpers.py (`compare_grads`) on real oracle gradients.

The bench-size parity tests used to hold each gradient only to its NORM (within 5e-3 relative).  A dropped, doubled or swapped
32 x 32 tile of a large weight gradient barely moves a norm.  Here the oracle's gradients of a small CapGnnModel are mutated the
ways a GEMM tile schedule goes wrong; the comparator must flag each of them, pass a 1-ulp noise field, and the zeroed tile is
shown to slip through the old norm criterion."""
import functools

import pytest
import torch

import dlsg_amd
from helpers import load_case, weights_and_inputs, compare_grads, oracle_grads

OLD_NORM_REL = 5e-3                   # the norm criterion of the bench parity tests: |  ||g|| - ||g_ref|| | <= 5e-3 ||g_ref||


@functools.lru_cache(maxsize=None)
def _oracle_grads():
    from oracle import torch_ref as R
    args, vocab, g, kind = load_case('small_msvd')
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd, frames, regions, caps, lens = weights_and_inputs(net, g, args)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    out = orc(frames, regions, caps, 26, 1.0)
    R.ragged_ce(out[0], caps, lens).backward()
    return oracle_grads(orc)


def _want():
    return dict(_oracle_grads())


def _got():
    return {k: (None if v is None else v.clone()) for k, v in _oracle_grads().items()}


def _largest_weight(want):
    """name of the largest 2-d gradient with room for two 32-row blocks and a 32 x 32 tile"""
    cands = [(v.numel(), k) for k, v in want.items() if v is not None and v.dim() == 2 and v.shape[0] >= 64 and v.shape[1] >= 32]
    return max(cands)[1]


def _old_norm_ok(got, want):
    for k, ref in want.items():
        if ref is None:
            continue
        n, r = float(got[k].double().norm()), float(ref.double().norm())
        if abs(n - r) > OLD_NORM_REL * max(r, 1e-12):
            return False
    return True


def test_oracle_gradients_equal_themselves():
    want = _want()
    rep = compare_grads(_got(), want, 'identity')
    assert rep['checked'] > 20 and rep['max_ratio'] == 0.0 and rep['norm_ratio'] == 0.0


def test_zeroed_tile_passes_the_norm_check_and_fails_the_comparator():
    """The quietest aligned 32 x 32 tile of the largest weight gradient (the one a norm notices least) set to zero."""
    want = _want()
    k = _largest_weight(want)
    ref = want[k]
    R_, C_ = ref.shape[0] // 32, ref.shape[1] // 32
    tiles = ref[:R_ * 32, :C_ * 32].reshape(R_, 32, C_, 32).double().pow(2).sum((1, 3))
    i, j = divmod(int(tiles.argmin()), C_)
    got = _got()
    got[k][32 * i:32 * i + 32, 32 * j:32 * j + 32] = 0
    assert not torch.equal(got[k], ref)
    assert _old_norm_ok(got, want), 'the old norm criterion was meant to miss this tile'
    rep = compare_grads(got, want, 'zeroed tile', check=False)
    assert rep['failures'] and {f[0] for f in rep['failures']} == {k}, rep['failures']
    with pytest.raises(AssertionError):
        compare_grads(got, want, 'zeroed tile')


def test_swapped_row_blocks_fail_the_comparator():
    """Two 32-row blocks written to each other's place: the norm does not move at all."""
    want = _want()
    k = _largest_weight(want)
    got = _got()
    got[k][0:32], got[k][32:64] = want[k][32:64].clone(), want[k][0:32].clone()
    assert _old_norm_ok(got, want)
    rep = compare_grads(got, want, 'swapped blocks', check=False)
    assert {f[0] for f in rep['failures']} == {k}, rep['failures']
    assert rep['max_ratio'] > 1.0 and rep['norm_ratio'] > 1.0


def test_scaled_row_fails_the_comparator():
    """The row holding the largest element of the largest weight gradient scaled by 1.01."""
    want = _want()
    k = _largest_weight(want)
    got = _got()
    row = int(want[k].abs().argmax()) // want[k].shape[1]
    got[k][row] *= 1.01
    rep = compare_grads(got, want, 'scaled row', check=False)
    assert {f[0] for f in rep['failures']} == {k}, rep['failures']
    assert rep['max_param'] == k and rep['max_ratio'] > 1.0


def test_one_ulp_noise_passes():
    """Every element moved by about one float32 ulp of itself (rounding noise of another summation order)."""
    want = _want()
    got = _got()
    gen = torch.Generator().manual_seed(0)
    for k, v in got.items():
        if v is not None:
            v += v * (2.0 ** -23) * torch.randn(v.shape, generator=gen)
    rep = compare_grads(got, want, 'ulp noise')
    assert 0.0 < rep['max_ratio'] < 0.01 and 0.0 < rep['norm_ratio'] < 0.01, rep


def test_parameter_without_an_oracle_gradient_must_be_zero():
    want = _want()
    k = _largest_weight(want)
    want[k] = None
    got = _got()
    got[k].zero_()
    compare_grads(got, want, 'absent, zero')
    got[k][3, 5] = 1e-30
    rep = compare_grads(got, want, 'absent, nonzero', check=False)
    assert [f[0] for f in rep['failures']] == [k]


def test_nan_fails():
    want = _want()
    k = _largest_weight(want)
    got = _got()
    got[k][1, 1] = float('nan')
    rep = compare_grads(got, want, 'nan', check=False)
    assert rep['failures'] and all(f[0] == k for f in rep['failures'])
    assert rep['max_param'] == k and rep['max_ratio'] == float('inf')

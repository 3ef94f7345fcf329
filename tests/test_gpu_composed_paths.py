"""GPU (-m gpu): the composed paths (gemm + softmax + gemm + rowln) the engine takes where a fused kernel does not cover the shape,
and the mixed ones (LatentPSL forward fused, backward composed), on the real kernels against the float64 oracle; then scheduled
sampling on both sides of the fused in-kernel argmax's limit V * D = 2^21.  Every case first asserts the predicate values that
define it, so a later change of a limit cannot silently move it to another branch."""
import random

import pytest
import torch

import dlsg_amd
from dlsg_amd import limits
from dlsg_amd.synth import synth_state_dict, synth_batch
from helpers import small_args
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-4          # tests/test_gpu_parity.py


def models(args, V, seed):
    """-> (HIP model on the host, float64 oracle) on the same seeded weights"""
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    return net, orc.double()


# frames, P, H, B -> (o2v, LatentPSL forward, LatentPSL backward, self-attention core) fused?
CASES = [
    ((33, 8, 64, 3), (False, False, False, False)),    # everything composed
    ((26, 9, 64, 3), (True, True, False, True)),       # forward fused, backward composed: P > 8
    ((26, 33, 64, 3), (True, False, False, True)),     # both composed, the decoder attends 33 proposals
    ((32, 8, 1024, 1), (True, True, False, True)),     # backward composed by its LDS limit; o2v and self-attention fused at T = 32
    ((26, 32, 1024, 1), (True, False, False, True)),   # 128 KB of theta: the forward is composed (it used to be refused)
]


@pytest.mark.parametrize('shape,fused', CASES)
def test_composed_and_mixed_paths_against_the_float64_oracle(shape, fused):
    T, P, H, B = shape
    args = small_args(visual_hidden_size=H, region_projected_size=H, num_proposals=P, num_obj=16, max_frames=T, train_batch_size=B)
    net, orc = models(args, 50, 41)
    frames, regions, caps, lens = synth_batch(args, 50, B, 42)
    assert frames.shape[1] == T and regions.shape[2] == 16
    want = orc(frames.double(), regions.double(), caps, 26, 1.0)[0]
    loss_ref = R.ragged_ce(want, caps, lens)
    loss_ref.backward()
    net = net.cuda()
    ops = net.ops
    assert (bool(ops.o2v_supported(T, H)), bool(ops.latent_psl_supported(T, P, H)), bool(ops.latent_psl_bwd_supported(T, P, H)),
            bool(ops.sa_core_supported(T, 2 * H))) == fused
    with torch.no_grad():
        got = net(frames.cuda(), regions.cuda(), caps.cuda(), 26, 1.0)[0].cpu()
    err = (got.double() - want.detach()).abs().max().item()
    print('%s: max|dlogit| %.3g' % (shape, err))
    assert err <= LOGIT_TOL, err
    tr = dlsg_amd.Trainer(net, lr=0.0)
    loss = float(tr.step(frames.cuda(), regions.cuda(), caps.cuda(), lens, 1.0))
    print('%s: loss %.6f, oracle %.6f' % (shape, loss, loss_ref.item()))
    assert abs(loss - loss_ref.item()) <= 1e-3
    G = net.grad_views()
    worst, checked = 0.0, 0
    for k, p in orc.named_parameters():
        if p.grad is None:
            continue
        ref = p.grad
        e = (G[k].cpu().double() - ref).abs().max().item()
        bound = 2e-5 + 2e-3 * ref.abs().max().item()
        worst = max(worst, e / bound)
        assert e <= bound, (k, e, bound)
        checked += 1
    print('%s: %d gradients, worst error / bound %.3f' % (shape, checked, worst))
    assert checked >= 60


# vocabulary, batch seed: 96 x 21845 = 2^21 - 64 weights (in-kernel argmax), 96 x 21846 = 2^21 + 32 (separate path).  The batch
# seeds were chosen on the host so that no position is a near-tie (asserted below on the oracle alone).
@pytest.mark.parametrize('V,seed,fused', [(21845, 22, True), (21846, 23, False)])
def test_scheduled_sampling_on_both_sides_of_the_in_kernel_argmax_limit(V, seed, fused):
    from emul_ops import EmulOps
    D = 96
    args = small_args(decode_hidden_size=D)
    net, orc = models(args, V, 21)
    assert limits.dec_tail_sample(21845, D) and not limits.dec_tail_sample(21846, D)
    frames, regions, caps, lens = synth_batch(args, V, 3, seed)
    with torch.no_grad():
        random.seed(12)
        want = orc(frames.double(), regions.double(), caps, 26, 0.6)[0]
        random.seed(12)
        emu = net.set_ops(EmulOps())(frames, regions, caps, 26, 0.6)[0]
    # a near-tie at a sampled position would let the two sides feed different words legitimately: the oracle's own margin first
    top2 = want.topk(2, dim=-1)[0]
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    emu_err = (emu.double() - want).abs().max().item()
    print('V = %d: smallest top-2 logit gap of the oracle %.3g, float32 emulation against float64 %.3g' % (V, gap, emu_err))
    assert gap >= 100 * emu_err and gap >= 2e-4, (gap, emu_err)
    net.set_ops(None)
    net = net.cuda()
    assert bool(net.ops.dec_tail_sample_supported(V, D)) == fused
    random.seed(12)
    with torch.no_grad():
        got = net(frames.cuda(), regions.cuda(), caps.cuda(), 26, 0.6)[0].cpu()
    err = (got.double() - want).abs().max().item()
    print('V = %d: max|dlogit| %.3g' % (V, err))
    assert err <= LOGIT_TOL, err

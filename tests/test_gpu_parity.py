"""GPU (-m gpu): the HIP model against the golden vectors of the reference (tests/golden, produced by
tests/golden/make_goldens.py from the imported reference) and against the oracle on fresh seeded inputs.

north_star tolerance: logits within 1e-3 (fp32) of the reference, argmax-decoded token ids bit-exact.
We assert 2e-4 on logits (fp32 MFMA keeps ~1e-5), ids identical, gradients within 2e-3 of their scale."""
import os
import random

import numpy as np
import pytest
import torch

import dlsg_amd
from helpers import load_case, weights_and_inputs

pytestmark = pytest.mark.gpu

SMALL = ['small_msvd', 'small_msrvtt', 'small_noobj', 'small_baseline1', 'small_baselinemodel']
MODELS = {'capgnn': dlsg_amd.CapGnnModel, 'baseline1': dlsg_amd.CapBaseline1, 'baselinemodel': dlsg_amd.CapBaselineModel}
LOGIT_TOL = 2e-4


def build(tag, fused=True):
    args, vocab, g, kind = load_case(tag)
    torch.manual_seed(0)
    net = MODELS[kind](args, vocab).eval()
    sd, frames, regions, caps, lens = weights_and_inputs(net, g, args)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.fused_o2v = fused
    return net, g, frames.cuda(), regions.cuda(), caps.cuda(), lens, kind


def test_native_library_is_what_runs():
    from dlsg_amd.hip import HipOps, LIB_PATH, ABI_VERSION
    ops = HipOps()
    assert ops.lib.dlsg_abi_version() == ABI_VERSION == 8
    with open('/proc/self/maps') as f:
        assert 'libdlsg_hip.so' in f.read(), LIB_PATH


@pytest.mark.parametrize('tag', SMALL)
@pytest.mark.parametrize('fused', [True, False])
def test_forward_logits_and_intermediates(tag, fused):
    net, g, frames, regions, caps, lens, kind = build(tag, fused)
    with torch.no_grad():
        out = net(frames, regions, caps, 26, 1.0)
    err = np.abs(out[0].cpu().numpy() - g['logits']).max()
    assert err <= LOGIT_TOL, err
    if kind == 'capgnn':
        assert np.abs(out[1].cpu().numpy() - g['obj_psl']).max() <= LOGIT_TOL
        assert np.abs(out[2].cpu().numpy() - g['mot_psl']).max() <= LOGIT_TOL
        assert np.abs(out[3].cpu().numpy() - g['alpha']).max() <= LOGIT_TOL
        # every intermediate the reference fixture holds (models/layer.py:46-61,172-201), read out of the HIP schedule's own
        # activation store: frame nodes, normalised object nodes, graph output, BiLSTM / self-attention stages
        sv = {}
        with torch.no_grad():
            net._engine_forward(frames, regions, caps, 26, [True] * 26, False, net.next_seed(), sv)
        B, T = frames.shape[0], frames.shape[1]
        enc = net.encoder
        got = {}
        for key, pfx, m in (('obj', 'encoder.obj_encoder', enc.obj_encoder), ('mot', 'encoder.motion_encoder', enc.motion_encoder)):
            s_ = sv[pfx]
            got[key + '.v'] = s_['v'].view(B, T, -1)
            got[key + '.ov'] = s_['ov'].view(B, T, -1)
            if 'y' in s_:
                # o = LayerNorm(y): the fused graph kernel never materialises it -- rebuilt from what it saved (y, mean / rstd)
                st = s_['ostats']
                ln = m.obj_norm[1]
                o = (s_['y'] - st[:, :1]) * st[:, 1:2] * ln.weight.detach() + ln.bias.detach()
                got[key + '.o'] = o.view(B, -1, o.shape[-1])
        sp = sv['encoder.motion_pre_encoder']
        got['pre.embed'] = sp['e'].view(B, T, -1)
        got['pre.lstm'] = sp['out'].view(B, T, -1)
        got['pre.lstm_ln'] = (sp['x'].view(B, T, -1) - sp['pe'])          # the engine adds the positional table in the same launch
        got['pre.sa'] = sp['so'].view(B, T, -1)
        got['pre.out'] = sv['encoder.motion_encoder']['visual'].view(B, T, -1)
        checked = 0
        for k, v in got.items():
            if 'i.' + k in g:
                err = np.abs(v.detach().cpu().numpy() - g['i.' + k]).max()
                assert err <= LOGIT_TOL, (k, err)
                checked += 1
        assert checked >= 7, checked


@pytest.mark.parametrize('tag', SMALL)
def test_greedy_ids_bit_exact_and_scheduled_sampling(tag):
    net, g, frames, regions, caps, lens, kind = build(tag)
    net.update_beam_size(1)
    with torch.no_grad():
        ids = net(frames, regions, None)[0]
    assert ids.dtype == torch.int64
    assert np.array_equal(ids.cpu().numpy(), g['greedy_ids'])
    random.seed(12)
    with torch.no_grad():
        logits = net(frames, regions, caps, 26, 0.6)[0]
    assert np.abs(logits.cpu().numpy() - g['ss_logits']).max() <= LOGIT_TOL


def test_decoder_forward_with_step_feats():
    """models/layer.py:394,404-405: Decoder.forward called on its own with a given global feature (`step_feats`) -- logits and
    greedy ids of the reference's decoder on the weights / inputs of small_msvd (tests/golden/make_goldens_r5.py)"""
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'small_stepfeats.npz')))
    step = torch.from_numpy(fx['step_feats']).cuda()
    with torch.no_grad():
        obj, mot = net._encode(frames, regions, False, net.next_seed(), {})
        logits, alphas = net.decoder(obj, caps, 26, 1.0, cnn_feats_2=mot, step_feats=step)
        assert np.abs(logits.cpu().numpy() - fx['logits']).max() <= LOGIT_TOL
        assert len(alphas) == 26 and alphas[0].shape == (frames.shape[0], 16, 1)
        net.update_beam_size(1)
        ids, _ = net.decoder(obj, None, 26, 1.0, cnn_feats_2=mot, step_feats=step)
        assert np.array_equal(ids.cpu().numpy(), fx['greedy_ids'])
        # without step_feats the call is the model's own decoder pass
        logits2, _ = net.decoder(obj, caps, 26, 1.0, cnn_feats_2=mot)
        assert np.abs(logits2.cpu().numpy() - g['logits']).max() <= LOGIT_TOL


def test_decoder_forward_beam_branch_on_its_own():
    """models/layer.py:449-460: the decoder called on its own with beam_size != 1 searches itself -- best-beam ids of the
    reference's decoder from the encoder's proposals, with and without `step_feats` (tests/golden/small_decbeam.npz)"""
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    fx = dict(np.load(os.path.join(here, 'small_decbeam.npz')))
    step = torch.from_numpy(np.load(os.path.join(here, 'small_stepfeats.npz'))['step_feats']).cuda()
    with torch.no_grad():
        obj, mot = net._encode(frames, regions, False, net.next_seed(), {})
        for k in (3, 5):
            net.update_beam_size(k)
            ids, alphas = net.decoder(obj, None, None, 1.0, cnn_feats_2=mot)
            assert alphas == [] and np.array_equal(ids.cpu().numpy(), fx['beam%d_ids' % k])
            ids, _ = net.decoder(obj, None, None, 1.0, cnn_feats_2=mot, step_feats=step)
            assert np.array_equal(ids.cpu().numpy(), fx['beam%d_ids_stepfeats' % k])
            assert np.array_equal(net(frames, regions, None)[0].cpu().numpy(), fx['beam%d_ids' % k])


@pytest.mark.parametrize('tag', SMALL)
def test_beam5_ids_bit_exact(tag):
    net, g, frames, regions, caps, lens, kind = build(tag)
    net.update_beam_size(5)
    with torch.no_grad():
        ids = net(frames, regions, None)[0]
    assert np.array_equal(ids.cpu().numpy(), g['beam5_ids'])


@pytest.mark.parametrize('bias', [4.0, 7.0, 30.0])
@pytest.mark.parametrize('k', [5, 3])
def test_beam_early_exit_and_finished_beams(bias, k):
    """<end> made likely: beams finish at different steps and the search stops before max_words; the fused beam_select
    kernel + deferred early-exit test against the oracle's beam search (ids and output length)."""
    from oracle import torch_ref as R
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    sd = {kk: v.clone().cpu() for kk, v in net.state_dict().items()}
    sd['decoder.word_restore.bias'][net.decoder.vocab('<end>')] += bias
    net.load_state_dict(sd)
    args, vocab, _, _ = load_case('small_msvd')
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    orc.update_beam_size(k)
    net.update_beam_size(k)
    with torch.no_grad():
        want = orc(frames.cpu(), regions.cpu(), None)[0]
        got = net(frames, regions, None)[0].cpu()
    assert got.shape == want.shape and torch.equal(got, want), (got.shape, want.shape)
    if bias >= 30.0:
        assert got.shape[1] < 26


@pytest.mark.parametrize('tag', SMALL)
def test_autograd_gradients(tag):
    net, g, frames, regions, caps, lens, kind = build(tag)
    outs = net(frames, regions, caps, 26, 1.0)[0]
    rows = torch.cat([outs[j][:lens[j]] for j in range(outs.shape[0])], 0)
    tgt = torch.cat([caps[j][:lens[j]] for j in range(outs.shape[0])], 0)
    loss = torch.nn.functional.cross_entropy(rows, tgt)
    loss.backward()
    assert abs(loss.item() - float(g['loss'])) <= 1e-4
    for k, p in net.named_parameters():
        if 'gnone.' + k in g:
            assert p.grad is None, k
        else:
            ref = g['g.' + k]
            err = np.abs(p.grad.cpu().numpy() - ref).max()
            assert err <= 2e-5 + 2e-3 * np.abs(ref).max(), (k, err, np.abs(ref).max())


@pytest.mark.parametrize('tag', SMALL)
def test_trainer_step_loss_and_adam(tag):
    net, g, frames, regions, caps, lens, kind = build(tag)
    tr = dlsg_amd.Trainer(net)
    loss = tr.step(frames, regions, caps, lens, 1.0)
    assert abs(float(loss) - float(g['loss'])) <= 1e-4
    for k, p in net.named_parameters():
        s, a = g['post.' + k]
        assert abs(float(p.detach().double().sum()) - s) <= 1e-4 * max(1.0, a), k


def test_full_size_msvd_shape():
    """BASELINE config 0/1 shape: 26 x (2048+4096) frames, 16 x 2048 regions, vocab 1000."""
    net, g, frames, regions, caps, lens, kind = build('full_msvd_b2')
    with torch.no_grad():
        logits = net(frames, regions, caps, 26, 1.0)[0]
        err = np.abs(logits.cpu().numpy() - g['logits']).max()
        assert err <= 1e-3, err
        net.update_beam_size(1)
        ids = net(frames, regions, None)[0].cpu().numpy()
    bad = ids != g['greedy_ids']
    # a mismatch is only tolerable as a near-tie of the reference's own top-2 logits (none expected)
    assert not bad.any(), (np.argwhere(bad)[:5], g['logit_margin'].min())
    tr = dlsg_amd.Trainer(net)
    loss = tr.step(frames, regions, caps, lens, 1.0)
    assert abs(float(loss) - float(g['loss'])) <= 1e-3
    G = net.grad_views()
    for k, p in net.named_parameters():
        if 'gnorm.' + k in g:
            ref = float(g['gnorm.' + k])
            got = float(G[k].double().norm())
            assert abs(got - ref) <= 5e-3 * max(ref, 1e-6) + 1e-6, (k, got, ref)


def test_full_size_reference_default_feature_dims():
    """The reference's DEFAULT feature widths, `--a_feature_size 1536 --m_feature_size 1024` (utils/opt.py:69-70; SURVEY.md
    section 0 row 3), full hidden sizes: the 2-D stream is the strided 1536-column slice of the 2560-wide frame block
    (models/model.py:70).  Top-8 logits, greedy and beam-5 ids, proposals, attention weights, loss, every gradient norm,
    post-Adam checksums of the reference (tests/golden/make_goldens_r3.py)."""
    net, g, frames, regions, caps, lens, kind = build('full_default_b2')
    assert frames.shape[-1] == 1536 + 1024 and net.encoder.a_feature_size == 1536
    with torch.no_grad():
        out = net(frames, regions, caps, 26, 1.0)
        logits = out[0].cpu()
        top = torch.topk(logits, 8, dim=-1)
        assert np.array_equal(top.indices[..., 0].numpy(), g['logits_top_idx'][..., 0])
        assert np.abs(top.values.numpy() - g['logits_top_val']).max() <= 1e-3
        assert np.abs(logits.double().sum(-1).numpy() - g['logits_sum']).max() <= 0.05
        assert np.abs(out[1].cpu().numpy() - g['obj_psl']).max() <= LOGIT_TOL
        assert np.abs(out[2].cpu().numpy() - g['mot_psl']).max() <= LOGIT_TOL
        assert np.abs(out[3].cpu().numpy() - g['alpha']).max() <= LOGIT_TOL
        net.update_beam_size(1)
        assert np.array_equal(net(frames, regions, None)[0].cpu().numpy(), g['greedy_ids']), g['logit_margin'].min()
        net.update_beam_size(5)
        assert np.array_equal(net(frames, regions, None)[0].cpu().numpy(), g['beam5_ids'])
    tr = dlsg_amd.Trainer(net)
    loss = tr.step(frames, regions, caps, lens, 1.0)
    assert abs(float(loss) - float(g['loss'])) <= 1e-3
    G = net.grad_views()
    n = 0
    for k, p in net.named_parameters():
        if 'gnorm.' + k in g:
            ref = float(g['gnorm.' + k])
            got = float(G[k].double().norm())
            assert abs(got - ref) <= 5e-3 * max(ref, 1e-6) + 1e-6, (k, got, ref)
            n += 1
    assert n >= 60
    for k, p in net.named_parameters():
        s_, a_ = g['post.' + k]
        assert abs(float(p.detach().double().sum()) - s_) <= 1e-4 * max(1.0, a_), k


@pytest.mark.parametrize('mode', ['fp32', 'x3_bwd', 'x3_all'])
def test_full_size_msrvtt_shape(mode):
    """BASELINE config 3 shape (run_gun.py:31-40: 36 objects -> 936 object nodes, 5 proposals, D = 1536, vocab 10k), every
    output the fixture holds: top-8 logits, greedy and beam-5 ids, loss, the norm of every parameter gradient (the
    6144-wide language cell, the 936-object fused graph backward, the 10k-vocab CE / beam_select)."""
    net, g, frames, regions, caps, lens, kind = build('full_msrvtt_b2')
    net.gemm_precision = mode
    with torch.no_grad():
        logits = net(frames, regions, caps, 26, 1.0)[0].cpu()
        top = torch.topk(logits, 8, dim=-1)
        assert np.array_equal(top.indices[..., 0].numpy(), g['logits_top_idx'][..., 0])
        assert np.abs(top.values.numpy() - g['logits_top_val']).max() <= 1e-3
        assert np.abs(logits.double().sum(-1).numpy() - g['logits_sum']).max() <= 0.5
        net.update_beam_size(1)
        ids = net(frames, regions, None)[0].cpu().numpy()
        assert np.array_equal(ids, g['greedy_ids']), g['logit_margin'].min()
        net.update_beam_size(5)
        bids = net(frames, regions, None)[0].cpu().numpy()
        assert np.array_equal(bids, g['beam5_ids'])
    tr = dlsg_amd.Trainer(net)
    loss = tr.step(frames, regions, caps, lens, 1.0)
    assert abs(float(loss) - float(g['loss'])) <= 1e-3
    G = net.grad_views()
    n = 0
    for k, p in net.named_parameters():
        if 'gnorm.' + k in g:
            ref = float(g['gnorm.' + k])
            got = float(G[k].double().norm())
            assert abs(got - ref) <= 5e-3 * max(ref, 1e-6) + 1e-6, (k, got, ref)
            n += 1
    assert n >= 60


@pytest.mark.parametrize('tag', ['small_msvd', 'small_msrvtt', 'small_baseline1', 'full_msvd_b2'])
@pytest.mark.parametrize('graphs', [False, True])
def test_gradients_under_scheduled_sampling_vs_reference(tag, graphs):
    """tf = 0.6, coin order of random.seed(12): 11 of the 26 steps are fed their own argmax (layer.py:432-439) -- the
    per-step vocab projection, `select_embed` / `skip_if` under hipGraph replay, the embedding-gradient scatter to sampled
    ids.  Loss and every gradient against the reference itself (tests/golden/*_ss.npz), eager and replayed."""
    from helpers import load_aux, check_grads
    net, _, frames, regions, caps, lens, kind = build(tag)
    g = load_aux(tag, 'ss')
    tr = dlsg_amd.Trainer(net, lr=0.0, use_graphs=graphs)
    for rep in range(2 if graphs else 1):          # second pass = a replay of the captured graphs
        random.seed(12)
        loss = tr.step(frames, regions, caps, lens, 0.6)
        assert abs(float(loss) - float(g['loss'])) <= (1e-4 if 'logits' in g else 1e-3)
        G = net.grad_views()
        check_grads(lambda k, p: G[k], net.named_parameters(), g, rel=2e-3)
    if graphs:
        assert tr._graphs is not None


@pytest.mark.parametrize('tag', ['small_msvd', 'small_msrvtt'])
@pytest.mark.parametrize('graphs', [False, True])
def test_dropout_placement_vs_reference(tag, graphs):
    """TRAIN mode against the reference (tests/golden/*_drop.npz: the reference's forward/backward with
    torch.nn.functional.dropout drawing its masks from this build's counter hash, keyed by call order -> site): pins the
    nine dropout sites, their tensors and their p (layer.py:28,53,310,320,328; sublayer.py:21-26,58-61,87,183-187)."""
    from helpers import load_aux, check_grads
    net, _, frames, regions, caps, lens, kind = build(tag)
    g = load_aux(tag, 'drop')
    net.train()
    tf = float(g['meta.tf'])
    tr = dlsg_amd.Trainer(net, lr=0.0, use_graphs=graphs)
    for rep in range(2 if graphs else 1):
        net.seed_counter = int(g['meta.counter']) - 1
        random.seed(4)
        loss = tr.step(frames, regions, caps, lens, tf)
        assert abs(float(loss) - float(g['loss'])) <= 1e-4
        G = net.grad_views()
        check_grads(lambda k, p: G[k], net.named_parameters(), g, rel=2e-3)
    net.seed_counter = int(g['meta.counter']) - 1
    random.seed(4)
    with torch.no_grad():
        logits = net(frames, regions, caps, 26, tf)[0]
    assert np.abs(logits.cpu().numpy() - g['logits']).max() <= LOGIT_TOL


def test_train_mode_matches_emulated_masks():
    """dropout on: the stateless masks of the HIP kernels equal the numpy restatement in tests/emul_ops.py, so a
    train-mode step must agree with the emulated engine on the same seed."""
    from emul_ops import EmulOps
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    args, vocab, _, _ = load_case('small_msvd')
    torch.manual_seed(0)
    ref = dlsg_amd.CapGnnModel(args, vocab)
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ref.set_ops(EmulOps())
    outs = []
    for m, dev in ((ref, 'cpu'), (net, 'cuda')):
        m.train()
        m.seed_counter = 7
        random.seed(4)
        tr = dlsg_amd.Trainer(m, lr=0.0)
        loss = tr.step(frames.to(dev), regions.to(dev), caps.to(dev), lens, 0.9)
        outs.append((float(loss), m._gflat.cpu().clone()))
    assert abs(outs[0][0] - outs[1][0]) <= 1e-4
    d = (outs[0][1] - outs[1][1]).abs().max().item()
    assert d <= 2e-5 + 2e-3 * outs[0][1].abs().max().item(), d


@pytest.mark.parametrize('shape', [dict(B=5, T=26, L=26, O=16, P=8), dict(B=1, T=26, L=26, O=16, P=8),
                                   dict(B=3, T=20, L=12, O=5, P=5), dict(B=2, T=32, L=7, O=9, P=3)])
def test_oracle_parity_on_fresh_inputs(shape):
    """Not fixtures: new seeds and odd shapes (batch 1, 20 or 32 frames, 5 or 9 regions, short captions); the oracle
    (CPU torch restatement, pinned by the goldens) against the HIP path: logits, greedy ids, loss and every gradient."""
    from oracle import torch_ref as R
    from dlsg_amd.synth import synth_state_dict, synth_batch
    from helpers import small_args
    B, T, L = shape['B'], shape['T'], shape['L']
    args = small_args(num_obj=shape['O'], num_proposals=shape['P'], max_frames=T, max_words=L)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), 99)
    net.load_state_dict(sd)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    frames, regions, caps, lens = synth_batch(args, 50, B, 123)
    lens = lens.clamp(max=L)
    want = orc(frames, regions, caps, L, 1.0)[0]
    loss_ref = R.ragged_ce(want, caps, lens)
    loss_ref.backward()
    orc.update_beam_size(1)
    with torch.no_grad():
        ids_ref = orc(frames, regions, None)[0]
    net = net.cuda()
    with torch.no_grad():
        got = net(frames.cuda(), regions.cuda(), caps.cuda(), L, 1.0)[0].cpu()
        net.update_beam_size(1)
        ids = net(frames.cuda(), regions.cuda(), None)[0].cpu()
    assert (want.detach() - got).abs().max().item() <= LOGIT_TOL
    assert torch.equal(ids, ids_ref)
    tr = dlsg_amd.Trainer(net, lr=0.0)
    loss = tr.step(frames.cuda(), regions.cuda(), caps.cuda(), lens, 1.0, max_len=L)
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-4
    G = net.grad_views()
    for (k, p) in orc.named_parameters():
        if p.grad is None:
            continue
        ref = p.grad
        err = (G[k].cpu() - ref).abs().max().item()
        assert err <= 2e-5 + 2e-3 * ref.abs().max().item(), (k, err, ref.abs().max().item())


@pytest.mark.parametrize('train_mode', [False, True])
def test_hipgraph_trainer_matches_eager_trainer(train_mode):
    """Three optimisation steps: the hipGraph-replayed schedule (device-side coins / seed / Adam step) must track the
    eager schedule (host-side branching)."""
    res = []
    for graphs in (False, True):
        net, g, frames, regions, caps, lens, kind = build('small_msvd')
        net.train(train_mode)
        tr = dlsg_amd.Trainer(net, use_graphs=graphs)
        random.seed(21)
        losses = [float(tr.step(frames, regions, caps, lens, 0.7)) for _ in range(3)]
        torch.cuda.synchronize()
        res.append((losses, net._flat.cpu().clone()))
    for a, b in zip(res[0][0], res[1][0]):
        assert abs(a - b) <= 2e-4, (res[0][0], res[1][0])
    assert (res[0][1] - res[1][1]).abs().max().item() <= 1e-4


X3_LOGIT_TOL = 1e-3     # north_star: logits within 1e-3 of the reference


@pytest.mark.parametrize('tag', ['small_msvd', 'small_msrvtt', 'small_baseline1', 'full_msvd_b2'])
@pytest.mark.parametrize('mode', ['x3_all', 'x3_bwd'])
def test_split_bf16_precision_modes_hold_parity(tag, mode):
    """gemm_precision x3_*: split-bf16 matrix products must keep the north_star tolerance (logits 1e-3, ids bit-exact)
    and gradients within 2e-3 of their scale."""
    net, g, frames, regions, caps, lens, kind = build(tag)
    net.gemm_precision = mode
    with torch.no_grad():
        logits = net(frames, regions, caps, 26, 1.0)[0]
        err = np.abs(logits.cpu().numpy() - g['logits']).max()
        net.update_beam_size(1)
        ids = net(frames, regions, None)[0].cpu().numpy()
        net.update_beam_size(5)
        bids = net(frames, regions, None)[0].cpu().numpy()
    print('%s %s max|dlogit| = %.3g (min top-2 margin of the reference %.3g)' % (tag, mode, err, g['logit_margin'].min()))
    assert err <= X3_LOGIT_TOL, err
    assert np.array_equal(ids, g['greedy_ids'])
    assert np.array_equal(bids, g['beam5_ids'])
    tr = dlsg_amd.Trainer(net)
    loss = tr.step(frames, regions, caps, lens, 1.0)
    assert abs(float(loss) - float(g['loss'])) <= 1e-3
    G = net.grad_views()
    for k, p in net.named_parameters():
        if 'g.' + k in g:
            ref = g['g.' + k]
            e = np.abs(G[k].cpu().numpy() - ref).max()
            assert e <= 2e-5 + 2e-3 * np.abs(ref).max(), (k, e, np.abs(ref).max())
        elif 'gnorm.' + k in g:
            ref = float(g['gnorm.' + k])
            assert abs(float(G[k].double().norm()) - ref) <= 5e-3 * max(ref, 1e-6) + 1e-6, k


def test_graph_trainer_takes_a_batch_of_another_shape():
    """The short last batch of an epoch: the captured graphs are for one shape, other shapes are launched kernel by kernel
    and must give the same update as an eager trainer fed the same sequence of batches."""
    res = []
    for use_graphs in (True, False):
        net, g, frames, regions, caps, lens, kind = build('small_msvd')
        tr = dlsg_amd.Trainer(net, use_graphs=use_graphs)
        random.seed(5)
        losses = []
        for sl in (slice(0, 3), slice(0, 3), slice(0, 2), slice(0, 3)):
            losses.append(float(tr.step(frames[sl].contiguous(), regions[sl].contiguous(), caps[sl].contiguous(), lens[sl], 1.0)))
        res.append((losses, net._flat.clone()))
    assert np.allclose(res[0][0], res[1][0], atol=2e-5), (res[0][0], res[1][0])
    assert (res[0][1] - res[1][1]).abs().max().item() <= 3e-5


def test_segmented_graph_capture_as_used_with_several_ranks():
    """With world_size > 1 the step is captured as one hipGraph per gradient bucket (the RCCL all-reduces run between
    replays).  N > 1 cannot run on this box, so the segmentation itself is forced on one GPU and compared with the
    single-graph schedule."""
    res = []
    for cuts in (False, True):
        net, g, frames, regions, caps, lens, kind = build('small_msvd')
        net.train()
        tr = dlsg_amd.Trainer(net, use_graphs=True)
        tr.force_graph_cuts = cuts
        random.seed(5)
        losses = [float(tr.step(frames, regions, caps, lens, 0.8)) for _ in range(3)]
        torch.cuda.synchronize()
        if cuts:
            # decoder | motion_pre_encoder | the graph modules without their obj_embed weights | motion obj_embed.weight |
            # object obj_embed.weight | tail (Adam)
            assert len(tr._graphs) == 6
        res.append((losses, net._flat.cpu().clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])


def test_hipgraph_greedy_inference_ids_bit_exact():
    """BASELINE configs[4]: the graph-captured greedy decode returns the reference's token ids."""
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    net.update_beam_size(1)
    gg = dlsg_amd.GreedyGraph(net, frames, regions)
    ids = gg(frames, regions)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), g['greedy_ids'])
    ids2 = gg(frames.flip(0).contiguous(), regions.flip(0).contiguous())        # new inputs through the static buffers
    torch.cuda.synchronize()
    assert np.array_equal(ids2.cpu().numpy(), g['greedy_ids'][::-1])


@pytest.mark.parametrize('tag', ['small_msvd', 'small_baselinemodel', 'full_msvd_b2'])
def test_hipgraph_beam_search_ids_bit_exact(tag):
    """BeamGraph (whole beam search replayed from a hipGraph, no host sync inside) == the eager beam search == the golden
    beam-5 ids of the reference; a second replay on other inputs follows the inputs."""
    net, g, frames, regions, caps, lens, kind = build(tag)
    net.update_beam_size(5)
    bg = dlsg_amd.BeamGraph(net, frames, regions)
    ids = bg(frames, regions)[0]
    assert np.array_equal(ids.cpu().numpy(), g['beam5_ids'])
    f2, r2 = torch.flip(frames, [0]).contiguous(), torch.flip(regions, [0]).contiguous()
    with torch.no_grad():
        want = net(f2, r2, None)[0]
    assert torch.equal(bg(f2, r2)[0], want)


@pytest.mark.parametrize('Bn', [64, 128])
def test_full_size_batch64_clips_are_independent_and_deterministic(Bn):
    """Size-independent properties at the bench configuration (MSVD-shaped, batch 64, and 128 = BASELINE
    config 4's per-GPU batch): the forward is deterministic
    (bit-identical on a second run) and a clip's logits / greedy ids do not depend on which other clips share its batch
    (same clip alone, in a batch of 3, in the full batch): catches any cross-clip indexing at full size."""
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(1000)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), 3))
    net = net.cuda()
    frames, regions, caps, lens = synth_batch(args, 1000, Bn, 5)
    frames, regions, caps = frames.cuda(), regions.cuda(), caps.cuda()
    with torch.no_grad():
        full = net(frames, regions, caps, 26, 1.0)[0]
        again = net(frames, regions, caps, 26, 1.0)[0]
        assert torch.equal(full, again)
        net.update_beam_size(1)
        ids_full = net(frames, regions, None)[0]
        for sel in ([0], [Bn - 1], [5, 17, 40]):
            idx = torch.tensor(sel, device='cuda')
            part = net(frames[idx].contiguous(), regions[idx].contiguous(), caps[idx].contiguous(), 26, 1.0)[0]
            assert (part - full[idx]).abs().max().item() <= 5e-5, sel
            ids_part = net(frames[idx].contiguous(), regions[idx].contiguous(), None)[0]
            assert torch.equal(ids_part, ids_full[idx]), sel


def test_full_size_train_step_gradients_are_bit_reproducible():
    """The whole gradient arena of a batch-64 MSVD-shaped step (eval mode: no dropout seed to vary) is bit-identical across
    runs, kernel by kernel and replayed: no float atomics are left on the path (word-embedding scatter, tall column sums)."""
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(1000)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), 3))
    net = net.cuda()
    frames, regions, caps, lens = [t.cuda() for t in synth_batch(args, 1000, 64, 5)]
    for graphs in (False, True):
        tr = dlsg_amd.Trainer(net, lr=0.0, use_graphs=graphs)
        ref = None
        for _ in range(4):
            tr.step(frames, regions, caps, lens, 1.0)
            cur = net._gflat.clone()
            if ref is None:
                ref = cur
                assert float(ref.abs().max()) > 0
            assert torch.equal(cur, ref), int((cur != ref).sum())


@pytest.mark.parametrize('mode,Bn,shape', [('fp32', 64, 'msvd'), ('x3_bwd', 64, 'msvd'), ('fp32', 128, 'msvd'),
                                           ('fp32', 64, 'msrvtt'), ('fp32', 90, 'msvd')])      # 90: 67-row shard, ragged 64-row tiles
def test_full_size_gradient_is_token_weighted_mean_of_shard_gradients(mode, Bn, shape):
    """Property at the bench configurations (batch 64 and 128 MSVD-shaped, batch 64 MSR-VTT-shaped = BASELINE configs 1, 4
    and 3 per GPU; dropout off): the ragged CrossEntropy is a mean over
    sum(cap_lens) rows, so grad(batch) = (n_A grad(A) + n_B grad(B)) / (n_A + n_B) for any split of the batch.  Exercises
    every backward kernel at full size with no oracle in the loop."""
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped() if shape == 'msvd' else dlsg_amd.msrvtt_shaped()
    V = 1000 if shape == 'msvd' else 10000
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), 4))
    net = net.cuda()
    net.gemm_precision = mode
    frames, regions, caps, lens = synth_batch(args, V, Bn, 6)
    frames, regions, caps = frames.cuda(), regions.cuda(), caps.cuda()
    tr = dlsg_amd.Trainer(net, lr=0.0)

    def grad(sl):
        loss = tr.step(frames[sl].contiguous(), regions[sl].contiguous(), caps[sl].contiguous(), lens[sl], 1.0)
        return float(loss), net._gflat.clone(), int(lens[sl].clamp(max=26).sum())
    lf, gf, nf = grad(slice(0, Bn))
    la, ga, na = grad(slice(0, 23))
    lb, gb, nb = grad(slice(23, Bn))
    assert na + nb == nf
    assert abs(lf - (na * la + nb * lb) / nf) <= 2e-5
    want = (na * ga + nb * gb) / nf
    scale = gf.abs().max().item()
    tol = 2e-5 if mode == 'fp32' else 3e-4
    assert (gf - want).abs().max().item() <= tol * scale + 1e-7, ((gf - want).abs().max().item(), scale)


def test_graph_trainer_follows_lr_changes_and_resumes_from_torch_adam_state():
    """The replayed graphs read the learning rate (and Adam's bias corrections) from device memory: changing
    `trainer.lr` between replays (MultiStepLR, run_gun.py:94-95) must act exactly as on an eager trainer; and a trainer
    resumed from an exported Adam state continues bit-for-bit like the one that exported it."""
    res = []
    for use_graphs in (True, False):
        net, g, frames, regions, caps, lens, kind = build('small_msvd')
        tr = dlsg_amd.Trainer(net, use_graphs=use_graphs)
        random.seed(7)
        for epoch in (0, 4, 7):
            tr.lr = dlsg_amd.multistep_lr(epoch)
            tr.step(frames, regions, caps, lens, 1.0)
        res.append((net._flat.clone(), tr.optimizer_state_dict()))
    assert (res[0][0] - res[1][0]).abs().max().item() <= 3e-6
    # resume: a fresh trainer + exported state == continuing the original
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    tr = dlsg_amd.Trainer(net)
    net._flat.copy_(res[1][0])
    tr.load_optimizer_state_dict(res[1][1])
    assert tr.t == 3 and abs(tr.lr - dlsg_amd.multistep_lr(7)) < 1e-12
    net2, *_ = build('small_msvd')
    tr2 = dlsg_amd.Trainer(net2)
    random.seed(7)
    for epoch in (0, 4, 7):
        tr2.lr = dlsg_amd.multistep_lr(epoch)
        tr2.step(frames, regions, caps, lens, 1.0)
    tr.step(frames, regions, caps, lens, 1.0)
    tr2.step(frames, regions, caps, lens, 1.0)
    assert torch.equal(net._flat, net2._flat)


@pytest.mark.parametrize('tag', SMALL)
def test_rank_schedule_equals_the_one_rank_schedule_on_every_model(tag):
    """`Trainer(rehearse_ranks=8)` -- the schedule of a data-parallel rank: per-bucket flush, buckets through the RCCL communicator
    inside the captured step (world 1), the all-rank Adam guard behind the last launch, BiLSTM backward step by step -- on every
    model family (CapGnnModel hands over five buckets, the baselines one): three train-mode steps with scheduled sampling land
    on the weights of the plain replayed trainer (the two BiLSTM backward forms differ in the last bits only)."""
    res = []
    for ranks in (0, 8):
        net, g, frames, regions, caps, lens, kind = build(tag)
        net.train()
        tr = dlsg_amd.Trainer(net, use_graphs=True, rehearse_ranks=ranks)
        random.seed(5)
        losses = [float(tr.step(frames, regions, caps, lens, 0.8)) for _ in range(3)]
        if ranks:
            info = tr.collectives_info()
            assert len(tr._graphs) == 1 and tr._adam_in_graph and info['where'] == "inside the step's hipGraph", info
            assert net.ops.persistent_bilstm_bwd is False and net.stream_k_in_backward and net.sk_backward_cu_budget == 0
        tr.check()
        res.append((losses, net._flat.clone()))
        tr.close()
    assert np.allclose(res[0][0], res[1][0], rtol=0, atol=2e-6), (res[0][0], res[1][0])
    assert (res[0][1] - res[1][1]).abs().max().item() <= 2e-6


def test_graph_trainer_with_an_extra_logit_gradient_matches_eager():
    """Trainer.step(extra_dlogits=...) in graph mode (forward + CrossEntropy | the caller's term | backward + Adam): the term
    sees the logits / loss / attention weights of THIS step and its result reaches the backward -- equal to the kernel-by-
    kernel step over several steps with scheduled sampling and changing terms; a step without the term falls back to eager."""
    res = []
    for use_graphs in (True, False):
        net, g, frames, regions, caps, lens, kind = build('small_msvd')
        net.train()
        tr = dlsg_amd.Trainer(net, use_graphs=use_graphs)
        random.seed(7)
        seen = []
        for k in range(4):
            def term(logits_tm, sv, k=k):
                seen.append((float(sv['loss_dev']), float(logits_tm.abs().sum()), float(sv['dec']['ALPHA'].sum())))
                return (0.02 * (k + 1)) * torch.tanh(logits_tm) / logits_tm.shape[1]
            loss = tr.step(frames, regions, caps, lens, 0.7, extra_dlogits=term)
            seen.append(float(loss))
        if use_graphs:
            assert tr._graphs is not None and [key for _, key in tr._graphs] == ['hook', None]
        tr.step(frames, regions, caps, lens, 0.7)                      # the other form of the step: eager on this trainer
        res.append((net._flat.clone(), seen))
    assert (res[0][0] - res[1][0]).abs().max().item() <= 3e-6
    for a, b in zip(res[0][1], res[1][1]):
        assert np.allclose(a, b, rtol=2e-5, atol=1e-6), (a, b)


def test_load_encoder_grafts_and_freezes_word_embedding(tmp_path):
    """models/model.py:45-53 on the GPU: graft + one optimisation step (eager and hipGraph) leaves the frozen word embedding
    bit-unchanged and equals the oracle doing the same with torch.optim.Adam."""
    from helpers import graft_and_step, OracleTrainer
    from oracle import torch_ref as R
    orc, _, loss_o = graft_and_step(R.CapGnnModelRef, 'cpu', tmp_path, OracleTrainer)
    want = dict(orc.named_parameters())
    for graphs in (False, True):
        net, emb0, loss = graft_and_step(dlsg_amd.CapGnnModel, 'cuda', tmp_path,
                                         lambda m: dlsg_amd.Trainer(m, use_graphs=graphs))
        assert abs(loss - loss_o) <= 1e-4
        assert torch.equal(net.decoder.word_embed.weight.detach().cpu(), emb0)
        for k, p in net.named_parameters():
            d = (p.detach().cpu() - want[k].detach()).abs()
            assert d.max().item() <= 3.3e-4 and (d > 2e-6).float().mean().item() <= 5e-3, (k, d.max().item())


def test_out_of_range_caption_id_poisons_the_loss():
    """torch's CrossEntropyLoss raises on a target >= V; the fused ragged CE cannot raise from the device, it must not read
    out of bounds and returns a NaN loss."""
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    bad = caps.clone()
    bad[0, 0] = net.decoder.vocab_size + 7
    L, Bn, V = 26, caps.shape[0], net.decoder.vocab_size
    logits = torch.randn(L, Bn, V, device='cuda')
    dl = torch.empty_like(logits); rl = torch.empty(L * Bn, device='cuda'); loss = torch.empty(1, device='cuda')
    net.ops.ce_ragged(logits, bad, torch.as_tensor(lens).cuda(), dl, rl, loss, time_major=True)
    assert torch.isnan(loss).item()
    net.ops.ce_ragged(logits, caps, torch.as_tensor(lens).cuda(), dl, rl, loss, time_major=True)
    assert torch.isfinite(loss).item() and torch.isfinite(dl).all().item()


def _oracle_hyp_logp(orc, frames, regions, hyp, end, upto):
    """the beam score of the hypothesis hyp[:upto + 1] of one clip under the oracle: the sum of its words' log-probabilities,
    teacher-forced, nothing added after the first <end> (allennlp_beamsearch.py: an ended beam only appends <end> at 0)"""
    with torch.no_grad():
        logits = orc(frames, regions, hyp[:upto + 1].unsqueeze(0), upto + 1, 1.0)[0][0].double()
    lp = torch.log_softmax(logits, -1).gather(1, hyp[:upto + 1].view(-1, 1)).view(-1)
    s = 0.0
    for t in range(upto + 1):
        s += float(lp[t])
        if int(hyp[t]) == end:
            break
    return s


@pytest.mark.parametrize('end_bias', [0.0, 9.0])
def test_beam5_at_batch128_config4_as_stated(end_bias):
    """BASELINE configs[4] as it is stated: allennlp-style beam search with beam 5 at batch 128, MSVD-shaped, one GPU
    (layer.py:449-460,489-567; allennlp_beamsearch.py:51-294).  640 beam rows go through `dec_mid` / `dec_tail`, the state
    gathers and `beam_select`.  Asserted: (1) the hipGraph-captured search (no host sync inside) returns exactly the ids
    of the eager search with its host-side early exit -- also when every beam ends early (`end_bias` lifts <end>'s logit so
    the whole batch stops after a few words and the cut of `beam_finish` is exercised); (2) a clip's beam ids do not depend on
    which other clips share its batch (alone, among 3, among 128) beyond the common length of the two results; (3) all 128 clips
    agree with the oracle's beam search (CPU restatement of the reference) token for token: the same common prefix and only <end>
    beyond it.  At most two clips other than 3, 64 and 127 may differ, and only at a demonstrated near-tie."""
    from dlsg_amd.synth import synth_state_dict, synth_batch
    from oracle import torch_ref as R
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(1000)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), 3)
    if end_bias:
        sd['decoder.word_restore.bias'] = sd['decoder.word_restore.bias'].clone()
        sd['decoder.word_restore.bias'][vocab('<end>')] += end_bias
    net.load_state_dict(sd)
    net = net.cuda()
    Bn = 128
    frames, regions, caps, lens = synth_batch(args, 1000, Bn, 5)
    fc, rc = frames.cuda(), regions.cuda()
    net.update_beam_size(5)
    with torch.no_grad():
        ids_eager = net(fc, rc, None)[0]
    assert ids_eager.shape[0] == Bn and 1 <= ids_eager.shape[1] <= 26
    if end_bias:
        assert ids_eager.shape[1] < 26, 'the biased <end> was meant to stop the whole batch early'
    bg = dlsg_amd.BeamGraph(net, fc, rc)
    ids_graph = bg(fc, rc)[0]
    assert torch.equal(ids_graph, ids_eager)
    ids_again = bg(fc, rc)[0]
    assert torch.equal(ids_again, ids_eager)
    end = vocab('<end>')
    with torch.no_grad():
        for sel in ([0], [Bn - 1], [5, 77, 100]):
            idx = torch.tensor(sel, device='cuda')
            part = net(fc[idx].contiguous(), rc[idx].contiguous(), None)[0]
            n = min(part.shape[1], ids_eager.shape[1])
            assert torch.equal(part[:, :n], ids_eager[idx][:, :n]), sel
            # past the shorter result the longer one only appends <end> (all beams of those clips had ended)
            assert bool((part[:, n:] == end).all()) and bool((ids_eager[idx][:, part.shape[1]:] == end).all()), sel
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    orc.update_beam_size(5)
    with torch.no_grad():
        want = orc(frames, regions, None)[0]
    got = ids_eager.cpu()
    L = max(want.shape[1], got.shape[1])
    pad = lambda x: torch.cat([x, torch.full((Bn, L - x.shape[1]), end, dtype=x.dtype)], 1)
    # exact common prefix, only <end> beyond it: the padded rows are equal
    differ = [b for b in range(Bn) if not torch.equal(pad(got)[b], pad(want)[b])]
    print('beam-5 at batch 128, end_bias %g: %d of %d clips differ from the oracle %s' % (end_bias, len(differ), Bn, differ))
    assert len(differ) <= 2 and not set(differ) & {3, 64, 127}, differ
    for b in differ:
        # the only excuse is a near-tie: at the first differing step the oracle's own cumulative log-probabilities of the two
        # competing hypotheses (teacher-forced through the oracle) agree within 1e-5 relative
        x, y = pad(got)[b], pad(want)[b]
        d = int((x != y).nonzero()[0])
        lp = [_oracle_hyp_logp(orc, frames[b:b + 1], regions[b:b + 1], h, end, d) for h in (x, y)]
        assert abs(lp[0] - lp[1]) <= 1e-5 * abs(lp[1]), (b, d, lp)


def test_single_long_clip_with_many_objects_stays_inside_the_graph_kernel_limits():
    """B = 1, T = 32 frames, 36 objects: 72 object tiles for one clip-stream used to ask the fused graph kernel for more
    chunks per clip (72) than it accepts (64) -> EINVAL (round-2 advisor).  Forward and a train step against the oracle."""
    from dlsg_amd.synth import synth_state_dict, synth_batch
    from dlsg_amd.engine import o2v_nsplit, O2V_MAX_NSPLIT
    from oracle import torch_ref as R
    assert o2v_nsplit(1, 32 * 36) == O2V_MAX_NSPLIT and o2v_nsplit(2, 29 * 36) <= O2V_MAX_NSPLIT
    args = dlsg_amd.make_args(visual_hidden_size=64, region_projected_size=64, query_hidden_size=48, decode_hidden_size=96,
                              a_feature_size=40, m_feature_size=72, region_feature_size=32, word_size=20, num_proposals=8,
                              num_obj=36, max_frames=32, train_batch_size=1)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), 11)
    net.load_state_dict(sd)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    frames, regions, caps, lens = synth_batch(args, 50, 1, 12)
    assert frames.shape[1] == 32 and regions.shape[2] == 36
    with torch.no_grad():
        want = orc(frames, regions, caps, 26, 1.0)[0]
    net = net.cuda()
    with torch.no_grad():
        got = net(frames.cuda(), regions.cuda(), caps.cuda(), 26, 1.0)[0].cpu()
    assert (got - want).abs().max().item() <= LOGIT_TOL
    tr = dlsg_amd.Trainer(net)
    loss = float(tr.step(frames.cuda(), regions.cuda(), caps.cuda(), lens, 1.0))
    assert abs(loss - R.ragged_ce(want, caps, lens).item()) <= 1e-3


@pytest.mark.parametrize('kind', ['baseline1', 'baselinemodel'])
def test_baseline_decoders_attend_over_clips_longer_than_32_frames(kind):
    """The baseline decoders attend over the frame nodes (models/model.py:76-107): clips of 33..72 frames are legal in the
    reference (positional-encoding table of 72 rows, sublayer.py:87) and used to be refused at construction because the fused
    word-step kernel held 32 attention rows.  40 frames: logits, greedy ids and a train step against the oracle."""
    from dlsg_amd.synth import synth_state_dict, synth_batch
    from oracle import torch_ref as R
    args = dlsg_amd.make_args(visual_hidden_size=64, region_projected_size=64, query_hidden_size=48, decode_hidden_size=96,
                              a_feature_size=40, m_feature_size=72, region_feature_size=32, word_size=20, num_proposals=8,
                              num_obj=16, max_frames=40, train_batch_size=3)
    vocab = dlsg_amd.make_vocab(50)
    torch.manual_seed(0)
    net = MODELS[kind](args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), 21)
    net.load_state_dict(sd)
    orc = {'baseline1': R.CapBaseline1Ref, 'baselinemodel': R.CapBaselineModelRef}[kind](args, vocab).eval()
    orc.load_state_dict(sd)
    frames, regions, caps, lens = synth_batch(args, 50, 3, 22)
    assert frames.shape[1] == 40
    with torch.no_grad():
        want = orc(frames, regions, caps, 26, 1.0)[0]
        orc.update_beam_size(1)
        want_ids = orc(frames, regions, None)[0]
    net = net.cuda()
    with torch.no_grad():
        got = net(frames.cuda(), regions.cuda(), caps.cuda(), 26, 1.0)[0].cpu()
        net.update_beam_size(1)
        ids = net(frames.cuda(), regions.cuda(), None)[0].cpu()
    assert (got - want).abs().max().item() <= LOGIT_TOL
    assert torch.equal(ids, want_ids)
    ref_tr = R.make_optimizer(orc)
    want_loss = R.train_step(orc.train(False), ref_tr, frames, regions, caps, lens, 1.0)
    tr = dlsg_amd.Trainer(net)
    loss = float(tr.step(frames.cuda(), regions.cuda(), caps.cuda(), lens, 1.0))
    assert abs(loss - float(want_loss)) <= 1e-3
    G = net.grad_views()
    for k, p in orc.named_parameters():
        if p.grad is None:
            continue
        ref = p.grad
        err = (G[k].cpu() - ref).abs().max().item()
        assert err <= 2e-5 + 2e-3 * ref.abs().max().item(), (k, err)

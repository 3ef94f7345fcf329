"""GPU (-m gpu): the shared capture-and-replay helper (dlsg_amd/graphs.py) where its seven users cannot show it: a capture whose
body raises on the host, a replay after the model re-packed its parameter arena, and the SCSTTrainer rebuilding its graphs after
such a re-pack.  All on the two-clip `small_msvd` case and its golden ids (bit-exact, as in tests/test_gpu_parity.py)."""
import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd.graphs import capture
from dlsg_amd.hip import HipOps
from test_gpu_parity import build

pytestmark = pytest.mark.gpu


def repack(net):
    """what load_encoder / load_state_dict into a copy / .to() lead to: the parameters move to a new arena"""
    old = net._flat
    net._flat = None
    net.flatten_parameters_()
    assert net._flat is not old and net._flat.data_ptr() != old.data_ptr()
    return old                                   # (kept alive by the caller: the new arena cannot reuse its address)


def test_host_exception_in_a_captured_body_leaves_the_capture_stream_usable():
    """A Python exception between two launches of a captured body (no device error): it propagates, the capture is ended -- every
    capture of the process shares this stream -- and the next graph captured on it is right."""
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    x = torch.zeros(64, device=frames.device)

    def body():
        net.ops.fill(x, 1.0)
        raise ValueError('host error between two launches')
    with pytest.raises(ValueError, match='host error between two launches'):
        capture(x.device, body, warmup=lambda: net.ops.fill(x, 0.0))
    with torch.cuda.stream(HipOps.capture_stream(x.device)):
        assert not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0           # the captured fill was recorded, never run
    ids = dlsg_amd.GreedyGraph(net, frames, regions)(frames, regions)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), g['greedy_ids'])


def test_replay_against_a_repacked_arena_is_refused():
    """A graph holds addresses into the arena it was captured on: after a re-pack a replay raises before it launches anything
    (it used to return captions computed from the old arena's weights); graphs built afterwards give the golden ids again."""
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    net.update_beam_size(5)

    def check(gg, bg):
        ids, beam = gg(frames, regions), bg(frames, regions)[0]
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), g['greedy_ids'])
        assert np.array_equal(beam.cpu().numpy(), g['beam5_ids'])
    gg, bg = dlsg_amd.GreedyGraph(net, frames, regions), dlsg_amd.BeamGraph(net, frames, regions)
    check(gg, bg)
    assert gg.valid_for(frames, regions) and bg.valid_for(frames, regions)
    old = repack(net)
    for graph in (gg, bg):
        assert not graph.valid_for(frames, regions)
        before = net.ops.launches
        with pytest.raises(RuntimeError, match='arena'):
            graph(frames, regions)
        assert net.ops.launches == before
    check(dlsg_amd.GreedyGraph(net, frames, regions), dlsg_amd.BeamGraph(net, frames, regions))
    del old


def test_scst_trainer_rebuilds_its_graphs_after_a_repack():
    net, g, frames, regions, caps, lens, kind = build('small_msvd')
    net.update_beam_size(1)
    net.train()
    words = [net.decoder.vocab.idx2word[i] for i in range(4, 12)]
    vids = [str(b) for b in range(frames.shape[0])]
    reward = dlsg_amd.CiderD({v: [' '.join(words[b:b + 4]), ' '.join(words[b + 1:b + 6])] for b, v in enumerate(vids)})
    scst = dlsg_amd.SCSTTrainer(net, reward, n_samples=2, baseline='greedy', use_graphs=True)
    scst.step(frames, regions, vids)
    sampler, greedy = scst._sampler, scst._greedy
    assert sampler.arena is net._flat and greedy.arena is net._flat and scst.trainer._graphs is not None
    old = repack(net)
    out = scst.step(frames, regions, vids)
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))
    assert scst._sampler is not sampler and scst._greedy is not greedy
    assert scst._sampler.arena is net._flat and scst._greedy.arena is net._flat
    assert scst.trainer._graphs is not None
    del old

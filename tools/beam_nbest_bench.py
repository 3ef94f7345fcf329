"""Beam search at batch 128, beam 5, MSVD-shaped, vocabulary 1000, as replayed hipGraphs, one JSON line:
  * `beam_graph`   -- BeamGraph: the reference's search (one caption per clip; the call ends in the host back-trace of `beam_finish`);
  * `nbest_off`    -- NBestBeamGraph with the options off (all 5 beams with scores, token history carried on the device);
  * `nbest_on`     -- NBestBeamGraph with no_repeat_ngram = 3, min_len = 4, length_penalty = 0.7.
The three graphs live in one process and are timed in alternating rounds (the order rotates from round to round); every figure is
ms per batch including the device synchronisation that makes the result readable.  `spread` of a graph is (max - min) / median over
its rounds: BeamGraph's own spread is the yardstick for the other two.
usage: python3 tools/beam_nbest_bench.py [rounds=9] [replays per round=5]
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def measure(rounds=9, reps=5, B=128, V=1000, k=5):
    import torch
    for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    net.load_state_dict(synth_state_dict(net.state_dict(), 0))
    net = net.to('cuda').eval()
    net.update_beam_size(k)
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    frames, regions = frames.cuda(), regions.cuda()
    graphs = [('beam_graph', dlsg_amd.BeamGraph(net, frames, regions)),
              ('nbest_off', dlsg_amd.NBestBeamGraph(net, frames, regions)),
              ('nbest_on', dlsg_amd.NBestBeamGraph(net, frames, regions, no_repeat_ngram=3, min_len=4, length_penalty=0.7))]
    ms = {name: [] for name, _ in graphs}
    for name, g in graphs:                                     # first replays outside the timing
        g(g.frames, g.regions)
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(graphs)):
            name, g = graphs[(i + r) % len(graphs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                g(g.frames, g.regions)
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'beam search as hipGraph replays: batch %d, beam %d, MSVD-shaped, vocabulary %d; %d alternating rounds of %d '
                   'replays, ms per batch' % (B, k, V, rounds, reps)}
    for name, _ in graphs:
        med = statistics.median(ms[name])
        out[name] = {'median_ms': round(med, 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3),
                     'spread': round((max(ms[name]) - min(ms[name])) / med, 4), 'rounds_ms': [round(x, 3) for x in ms[name]]}
    base = out['beam_graph']['median_ms']
    for name in ('nbest_off', 'nbest_on'):
        out[name]['over_beam_graph'] = round(out[name]['median_ms'] / base, 4)
    ids, scores, lens = graphs[1][1](frames, regions)
    top = graphs[0][1](frames, regions)[0]
    out['nbest_off_top1_equals_beam_graph'] = bool(torch.equal(ids[:, 0, :top.shape[1]], top))
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

"""Ensemble beam search at batch 128, beam 5, MSVD-shaped, vocabulary 1000, as replayed hipGraphs, one JSON line.  Options on in
every leg: no_repeat_ngram = 3, min_len = 4, length_penalty = 0.7.
  * `nbest_1`   -- (a) NBestBeamGraph of one member;
  * `ens_1`     -- (b) EnsembleBeamGraph of that one member: against (a), the third row read and the combine at M = 1;
  * `ens_3`     -- (c) EnsembleBeamGraph of three members (seeds 0, 1, 2), mode 'prob', uniform weights;
  * `nbest_x3`  -- (d) the three members' NBestBeamGraphs replayed back to back: against (c), one shared search or three.
The graphs live in one process and are timed in alternating rounds (the order rotates from round to round); every figure is ms
per batch including the device synchronisation that makes the result readable.  `spread` of a leg is (max - min) / median over its
rounds.
usage: python3 tools/ensemble_bench.py [rounds=7] [replays per round=5]
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def measure(rounds=7, reps=5, B=128, V=1000, k=5):
    import torch
    for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    nets = []
    for seed in range(3):
        torch.manual_seed(0)
        net = dlsg_amd.CapGnnModel(args, vocab)
        net.load_state_dict(synth_state_dict(net.state_dict(), seed))
        nets.append(net.to('cuda').eval())
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    frames, regions = frames.cuda(), regions.cuda()
    opts = dict(beam_size=k, no_repeat_ngram=3, min_len=4, length_penalty=0.7)
    singles = [dlsg_amd.NBestBeamGraph(net, frames, regions, **opts) for net in nets]
    ens1 = dlsg_amd.EnsembleBeamGraph(dlsg_amd.Ensemble(nets[:1]), frames, regions, **opts)
    ens3 = dlsg_amd.EnsembleBeamGraph(dlsg_amd.Ensemble(nets), frames, regions, **opts)
    legs = [('nbest_1', singles[:1]), ('ens_1', [ens1]), ('ens_3', [ens3]), ('nbest_x3', singles)]
    ms = {name: [] for name, _ in legs}
    for name, graphs in legs:                                  # first replays outside the timing
        for g in graphs:
            g(frames, regions)
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(legs)):
            name, graphs = legs[(i + r) % len(legs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                for g in graphs:
                    g(frames, regions)
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'ensemble beam search as hipGraph replays: batch %d, beam %d, MSVD-shaped, vocabulary %d, bans and length penalty '
                   'on; %d alternating rounds of %d replays, ms per batch' % (B, k, V, rounds, reps)}
    for name, _ in legs:
        med = statistics.median(ms[name])
        out[name] = {'median_ms': round(med, 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3),
                     'spread': round((max(ms[name]) - min(ms[name])) / med, 4), 'rounds_ms': [round(x, 3) for x in ms[name]]}
    out['ens_1_over_nbest_1'] = round(out['ens_1']['median_ms'] / out['nbest_1']['median_ms'], 4)
    out['ens_3_over_nbest_x3'] = round(out['ens_3']['median_ms'] / out['nbest_x3']['median_ms'], 4)
    one, same = singles[0](frames, regions), ens1(frames, regions)
    out['ens_1_equals_nbest_1'] = all(bool(torch.equal(a, b)) for a, b in zip(one, same))
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

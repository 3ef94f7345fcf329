"""Diverse beam search against the plain n-best search at batch 128, beam 6, MSVD-shaped, vocabulary 1000, as replayed hipGraphs
(`NBestBeamGraph`), no_repeat_ngram = 3, min_len = 4, length_penalty = 0.7 in all three, one JSON line:
  * `plain`     -- one group: `dlsg_beam_select_hist` at every word (the code that was there before the groups);
  * `groups3`   -- num_groups = 3, diversity_penalty = 0.5: `dlsg_beam_select_groups` at every word;
  * `groups6`   -- num_groups = 6, diversity_penalty = 0.5.
The three graphs live in one process and are timed in alternating rounds (the order rotates from round to round); every figure is
ms per batch including the device synchronisation that makes the result readable.  `spread` of a graph is (max - min) / median over
its rounds: the plain graph's own spread is the yardstick for the other two.  `distinct_stems` is the mean number of different three-word
openings among a clip's 6 captions.
usage: python3 tools/groups_bench.py [rounds=9] [replays per round=5]
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def measure(rounds=9, reps=5, B=128, V=1000, k=6):
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
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    frames, regions = frames.cuda(), regions.cuda()
    opts = dict(beam_size=k, no_repeat_ngram=3, min_len=4, length_penalty=0.7)
    graphs = [('plain', dlsg_amd.NBestBeamGraph(net, frames, regions, **opts)),
              ('groups3', dlsg_amd.NBestBeamGraph(net, frames, regions, num_groups=3, diversity_penalty=0.5, **opts)),
              ('groups6', dlsg_amd.NBestBeamGraph(net, frames, regions, num_groups=6, diversity_penalty=0.5, **opts))]
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
    out = {'what': 'plain and diverse beam search as hipGraph replays: batch %d, beam %d, MSVD-shaped, vocabulary %d; %d alternating '
                   'rounds of %d replays, ms per batch' % (B, k, V, rounds, reps)}
    for name, g in graphs:
        med = statistics.median(ms[name])
        ids = g(frames, regions)[0]
        torch.cuda.synchronize()
        distinct = sum(len({tuple(r[:3]) for r in clip}) for clip in ids.cpu().tolist()) / float(B)
        out[name] = {'median_ms': round(med, 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3),
                     'spread': round((max(ms[name]) - min(ms[name])) / med, 4), 'rounds_ms': [round(x, 3) for x in ms[name]],
                     'distinct_stems': round(distinct, 2)}
    base = out['plain']['median_ms']
    for name in ('groups3', 'groups6'):
        out[name]['over_plain'] = round(out[name]['median_ms'] / base, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

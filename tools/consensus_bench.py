"""Consensus reranking against the diverse n-best search it reranks, at batch 128, beam 6 in 3 groups (diversity_penalty 0.5),
MSVD-shaped, vocabulary 1000, no_repeat_ngram = 3, min_len = 4, length_penalty = 0.7, as replayed hipGraphs, one JSON line:
  * `nbest`      -- `NBestBeamGraph`: the search alone (its code is the parent commit's: this tree adds launches after it only);
  * `consensus`  -- `ConsensusBeamGraph`: the same search, `dlsg_cider_consensus`, the gathers that reorder the beams;
  * `launch`     -- a graph that holds the `dlsg_cider_consensus` launch alone, on the search's output (HIP events around a replay).
The first two are timed in alternating rounds (the order rotates); every figure is ms per batch including the device
synchronisation that makes the result readable.  `spread` is (max - min) / median over a graph's rounds.  Also: how often the
consensus's first caption is not the search's first, and the mean expected utility of both.  The model's weights and the reward's
corpus are synthetic (seeded noise; captions of 5..12 words drawn with a heavy head), so the last three say how the pieces behave,
not how captions improve.
usage: python3 tools/consensus_bench.py [rounds=11] [replays per round=5]
       python3 tools/consensus_bench.py launch [launches=30]        # the launch alone, eagerly: the target of a kernel trace
The measurement runs in a child process under `timeout`."""
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def setup(B=128, V=1000, k=6):
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
    rng = random.Random(0)
    words = [vocab.idx2word[i] for i in range(4, V)]
    pick = lambda: words[min(int(rng.paretovariate(0.8)) - 1, len(words) - 1)]
    refs = {'v%d' % c: [' '.join(pick() for _ in range(rng.randint(5, 12))) for _ in range(20)] for c in range(1200)}
    reward = dlsg_amd.DeviceCiderD(refs, vocab)
    opts = dict(beam_size=k, num_groups=3, diversity_penalty=0.5, no_repeat_ngram=3, min_len=4, length_penalty=0.7)
    return dlsg_amd, net, reward, frames.cuda(), regions.cuda(), opts


def measure(rounds=11, reps=5, B=128, V=1000, k=6):
    import torch
    dlsg_amd, net, reward, frames, regions, opts = setup(B, V, k)
    from dlsg_amd.graphs import capture
    graphs = [('nbest', dlsg_amd.NBestBeamGraph(net, frames, regions, **opts)),
              ('consensus', dlsg_amd.ConsensusBeamGraph(net, frames, regions, reward, n_best=k, **opts))]
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
    out = {'what': 'diverse n-best search alone and with consensus reranking as hipGraph replays: batch %d, beam %d in 3 groups, '
                   'MSVD-shaped, vocabulary %d; %d alternating rounds of %d replays, ms per batch; synthetic model and corpus'
                   % (B, k, V, rounds, reps)}
    for name, g in graphs:
        med = statistics.median(ms[name])
        out[name] = {'median_ms': round(med, 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3),
                     'spread': round((max(ms[name]) - min(ms[name])) / med, 4), 'rounds_ms': [round(x, 3) for x in ms[name]]}
    out['consensus']['over_nbest'] = round(out['consensus']['median_ms'] / out['nbest']['median_ms'], 4)
    out['consensus']['minus_nbest_ms'] = round(out['consensus']['median_ms'] - out['nbest']['median_ms'], 3)
    # the launch alone, on the search's output
    ids, scores, lens = (x.clone() for x in graphs[0][1](frames, regions))
    graph, (order, expected) = capture(frames.device, lambda: reward.consensus_device(ids))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5 + 30)]
    for a, b in ev:
        a.record()
        graph.replay()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev[5:]]
    out['launch'] = {'median_us': round(statistics.median(us), 2), 'min_us': round(min(us), 2), 'max_us': round(max(us), 2),
                     'replays': len(us), 'clips': B, 'candidates': k}
    out['search_ms_per_word'] = round(out['nbest']['median_ms'] / net.decoder.max_words, 3)
    # what the consensus chooses
    first = order[:, 0].cpu()
    e = expected.cpu()
    out['choice'] = {'first_differs': round(float((first != 0).float().mean()), 4),
                     'mean_expected_search_first': round(float(e[:, 0].mean()), 4),
                     'mean_expected_consensus_first': round(float(e.gather(1, first.view(-1, 1)).mean()), 4)}
    net.ops.check_persistent()
    print(json.dumps(out))


def launch_only(launches=30):
    import torch
    dlsg_amd, net, reward, frames, regions, opts = setup()
    ids = net.beam_search(frames, regions, **opts)[0]
    for _ in range(launches):
        reward.consensus_device(ids)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'dlsg_cider_consensus launched %d times on a batch-128, beam-6 search output' % launches}))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1:3] == ['run', 'launch']:
        launch_only(*[int(x) for x in sys.argv[3:4]])
    elif len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

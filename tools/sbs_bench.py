"""Stochastic beam search (sampling without replacement) against the n-best beam search of as many beams, at batch 128, MSVD-shaped,
vocabulary 1000, no_repeat_ngram = 3, min_len = 4, as replayed hipGraphs, one JSON line:
  * `sbs5`, `sbs5t`     -- `StochasticBeamGraph` with n = 5, and n = 5 with the threshold (6 beams);
  * `nbest5`, `nbest6`  -- `NBestBeamGraph` with 5 and 6 beams (length_penalty 0.7): the comparator, code this search does not touch.
The four are timed in alternating rounds (the order rotates); every figure is ms per batch including the device synchronisation
that makes the result readable.  `spread` is (max - min) / median over a graph's rounds.  Also, on the tool's synthetic corpus:
the mean number of distinct captions among 5 from `sample(n=5)` and from this search, and the mean CIDEr-D of the consensus
caption chosen from either list, at temperatures 1, 0.5 and 0.25.  The model's weights and the corpus are synthetic (seeded
noise), so the quality figures say how the pieces behave, not how captions improve.
usage: python3 tools/sbs_bench.py [rounds=11] [replays per round=5]
       python3 tools/sbs_bench.py steps [searches=3]        # both searches eagerly: the target of a kernel trace
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIMIT_S = 300
BANS = dict(no_repeat_ngram=3, min_len=4)


def measure(rounds=11, reps=5, B=128, V=1000):
    import torch
    from consensus_bench import setup
    dlsg_amd, net, reward, frames, regions, _ = setup(B, V)
    graphs = [('sbs5', dlsg_amd.StochasticBeamGraph(net, frames, regions, n=5, **BANS)),
              ('nbest5', dlsg_amd.NBestBeamGraph(net, frames, regions, beam_size=5, length_penalty=0.7, **BANS)),
              ('sbs5t', dlsg_amd.StochasticBeamGraph(net, frames, regions, n=5, return_threshold=True, **BANS)),
              ('nbest6', dlsg_amd.NBestBeamGraph(net, frames, regions, beam_size=6, length_penalty=0.7, **BANS))]

    def replay(name, g, seed):
        return g(g.frames, g.regions, seed) if name.startswith('sbs') else g(g.frames, g.regions)
    ms = {name: [] for name, _ in graphs}
    for name, g in graphs:                                     # first replays outside the timing
        replay(name, g, 1)
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(graphs)):
            name, g = graphs[(i + r) % len(graphs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(reps):
                replay(name, g, 2 + r * reps + j)
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'stochastic beam search and the n-best beam search as hipGraph replays: batch %d, MSVD-shaped, vocabulary %d; %d '
                   'alternating rounds of %d replays, ms per batch; synthetic model and corpus' % (B, V, rounds, reps)}
    for name, g in graphs:
        med = statistics.median(ms[name])
        out[name] = {'median_ms': round(med, 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3),
                     'spread': round((max(ms[name]) - min(ms[name])) / med, 4), 'rounds_ms': [round(x, 3) for x in ms[name]]}
    out['sbs5']['over_nbest5'] = round(out['sbs5']['median_ms'] / out['nbest5']['median_ms'], 4)
    out['sbs5t']['over_nbest6'] = round(out['sbs5t']['median_ms'] / out['nbest6']['median_ms'], 4)
    # what the candidate lists are worth: distinct captions among 5, and the consensus caption's CIDEr-D
    L = net.decoder.max_words
    clip = reward.index(['v%d' % b for b in range(B)])
    out['quality'] = {}
    for temp in (1.0, 0.5, 0.25):                              # the synthetic model is flat: a low temperature stands in for a peaked one
        drawn = net.sample(frames, regions, n=5, temperature=temp, seed=11, **BANS)[0].view(B, 5, L)
        ours = net.sample_without_replacement(frames, regions, n=5, temperature=temp, seed=11, **BANS)[0]
        quality = {}
        for name, ids in (('sample', drawn), ('without_replacement', ours)):
            best = dlsg_amd.consensus_rerank(reward, ids, n_best=1)[0][:, 0].contiguous()
            quality[name] = {'mean_distinct_of_5': round(sum(len({tuple(r) for r in c}) for c in ids.tolist()) / B, 3),
                             'consensus_ciderd': round(float(reward.scores_device(best, clip).mean()), 4)}
        out['quality']['temperature_%g' % temp] = quality
    net.ops.check_persistent()
    print(json.dumps(out))


def steps_only(searches=3, B=128, V=1000):
    import torch
    from consensus_bench import setup
    dlsg_amd, net, reward, frames, regions, _ = setup(B, V)
    for i in range(searches):
        net.sample_without_replacement(frames, regions, n=5, seed=i, **BANS)
        net.beam_search(frames, regions, beam_size=5, length_penalty=0.7, **BANS)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'sample_without_replacement(n=5) and beam_search(beam_size=5) run %d times each, eagerly, batch %d'
                              % (searches, B)}))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1:3] == ['run', 'steps']:
        steps_only(*[int(x) for x in sys.argv[3:4]])
    elif len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

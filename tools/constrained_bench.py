"""Lexically constrained beam search against the n-best beam search, at batch 128, beam 5, MSVD-shaped, vocabulary 1000,
no_repeat_ngram = 3, min_len = 4, length_penalty 0.7, as replayed hipGraphs, one JSON line:
  * `nbest`        -- `NBestBeamGraph`: the comparator, code this search does not touch;
  * `cons_CxW`     -- `ConstrainedBeamGraph` with C constraints per clip of W alternatives each: 0x1, 2x1, 2x8, 8x1, 8x8 (random words).
The graphs are timed in alternating rounds (the order rotates) after a warm-up replay each; every figure is ms per batch including
the device synchronisation that makes the result readable; the median over the rounds, min, max and `spread` = (max - min) / median.
Per constrained graph also: `all_met`, the share of clips whose best caption (row 0) meets every constraint -- 1.0 by the step's
guarantee, so the tool doubles as a check at the workload's size --, and the mean score of that caption beside the unconstrained
best caption's: the price of the constraints.  `step_us`: the select launch alone, `beam_select_hist` and `beam_select_cons` (8x8)
on the logits of a mid-caption step, 200 back-to-back launches between two events per round, microseconds per launch.
The model's weights are synthetic (seeded noise): the scores say how the pieces behave, not how captions improve.
usage: python3 tools/constrained_bench.py [rounds=11] [replays per round=5]
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
OPTS = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=3, min_len=4)
SHAPES = [(0, 1), (2, 1), (2, 8), (8, 1), (8, 8)]


def summary(xs, digits=3):
    med = statistics.median(xs)
    return {'median': round(med, digits), 'min': round(min(xs), digits), 'max': round(max(xs), digits),
            'spread': round((max(xs) - min(xs)) / med, 4)}


def step_times(torch, net, cons, rounds, launches=200, B=128, k=5, t=6):
    """the select launch alone on (B*k, V) logits of a model-like scale, microseconds per launch"""
    ops, V, L = net.ops, net.decoder.vocab_size, net.decoder.max_words
    end, R = net.decoder.vocab('<end>'), B * k
    gen = torch.Generator(device='cuda').manual_seed(1)
    logits = torch.randn(R, V, device='cuda', generator=gen)
    hist = torch.randint(4, V, (2, R, L), device='cuda', generator=gen)
    last, lp = hist[0][:, t - 1].contiguous(), -torch.rand(R, device='cuda', generator=gen) * 5
    pred, back, rows = (torch.empty(R, dtype=torch.int64, device='cuda') for _ in range(3))
    nlp = torch.empty(R, device='cuda')
    calls = {'beam_select_hist': lambda: ops.beam_select_hist(logits, last, lp, pred, nlp, back, rows, k, end, hist[0], hist[1], t, 3, 4),
             'beam_select_cons': lambda: ops.beam_select_cons(logits, last, lp, pred, nlp, back, rows, k, end, hist[0], hist[1], t, cons, 3, 4)}
    us = {name: [] for name in calls}
    for r in range(rounds + 1):                                # round 0 warms up
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                call()
            b.record()
            b.synchronize()
            if r:
                us[name].append(a.elapsed_time(b) / launches * 1e3)
    return {name: summary(v, 2) for name, v in us.items()}


def measure(rounds=11, reps=5, B=128, V=1000):
    import torch
    from consensus_bench import setup
    dlsg_amd, net, reward, frames, regions, _ = setup(B, V)
    gen = torch.Generator().manual_seed(3)
    cons = {cw: torch.randint(4, V, (B, cw[0], cw[1]), generator=gen).cuda() for cw in SHAPES}
    graphs = [('nbest', dlsg_amd.NBestBeamGraph(net, frames, regions, **OPTS))]
    graphs += [('cons_%dx%d' % cw, dlsg_amd.ConstrainedBeamGraph(net, frames, regions, cons[cw], return_met=True, **OPTS)) for cw in SHAPES]

    def replay(name, g):
        return g(g.frames, g.regions) if name == 'nbest' else g(g.frames, g.regions, g.cons)
    ms = {name: [] for name, _ in graphs}
    for name, g in graphs:                                     # first replays outside the timing
        replay(name, g)
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(graphs)):
            name, g = graphs[(i + r) % len(graphs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(reps):
                replay(name, g)
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'constrained beam search and the n-best beam search as hipGraph replays: batch %d, beam 5, MSVD-shaped, vocabulary '
                   '%d; %d alternating rounds of %d replays, ms per batch; synthetic model' % (B, V, rounds, reps)}
    free = replay(*graphs[0])[1][:, 0].clone()
    for name, g in graphs:
        out[name] = dict(summary(ms[name]), rounds_ms=[round(x, 3) for x in ms[name]])
        if name != 'nbest':
            out[name]['over_nbest'] = round(out[name]['median'] / out['nbest']['median'], 4)
            ids, scores, lens, met = replay(name, g)
            C = g.cons.shape[1]
            out[name]['all_met'] = round(float((met[:, 0] == C).double().mean()), 4)
            out[name]['mean_score'] = round(float(scores[:, 0].mean()), 4)
    out['nbest']['mean_score'] = round(float(free.mean()), 4)
    out['step_us'] = step_times(torch, net, cons[(8, 8)], rounds)
    net.ops.check_persistent()
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

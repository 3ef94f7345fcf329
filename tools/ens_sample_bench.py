"""Sampling from an ensemble at batch 128, n = 5, MSVD-shaped, vocabulary 1000, eval mode, as replayed hipGraphs, one JSON line.
  * `ens_sample_3` -- EnsembleSampleGraph of three members (seeds 0, 1, 2), mode 'prob', uniform weights, temperature 1;
  * `sample_x3`    -- the three members' own SampleGraph(n=5, share_encoder=True) replayed back to back: the work of the members'
                      own samplers, against which `ens_sample_3` adds the combine and replaces three draws and embeddings by one draw
                      and three embeddings;
  * `ens_beam_3`   -- EnsembleBeamGraph of the same ensemble at beam 5: the search on the same number of rows.
The graphs live in one process and are timed in alternating rounds (the order rotates from round to round) after a first replay
each; every figure is ms per batch including the device synchronisation that makes the result readable; `spread` of a leg is
(max - min) / median over its rounds.
`step_us`: the word-step launch alone on 640 rows of logits of a model-like scale, 200 back-to-back launches between two events per
round, microseconds per launch, for the settings `min_len` (min_len = 1: the cheapest control) and `top` (top_k = 50, top_p = 0.9):
`sample_filter_embed` on one row of logits, `sample_ens` with M = 1 and with M = 3 at the same rows and V.
The weights are synthetic (seeded noise): the figures say what the launches cost.
usage: python3 tools/ens_sample_bench.py [rounds=7] [replays per round=5]
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def summary(xs, digits=3):
    med = statistics.median(xs)
    return {'median': round(med, digits), 'min': round(min(xs), digits), 'max': round(max(xs), digits),
            'spread': round((max(xs) - min(xs)) / med, 4), 'rounds': [round(x, digits) for x in xs]}


def step_times(torch, net, rows, V, rounds, launches=200, t=6):
    from dlsg_amd import engine as E
    ops, L, end = net.ops, net.decoder.max_words, net.decoder.vocab('<end>')
    W = net.decoder.word_embed.weight.shape[1]
    gen = torch.Generator(device='cuda').manual_seed(1)
    xs = [torch.randn(rows, V, device='cuda', generator=gen) * 3 for _ in range(3)]
    Em = torch.randn(V, W, device='cuda', generator=gen)
    hist = torch.randint(4, V, (L, rows), device='cuda', generator=gen)
    ids, out = torch.empty(rows, dtype=torch.int64, device='cuda'), torch.empty(rows, W, device='cuda')
    logp, ln = torch.empty(rows, device='cuda'), torch.full((rows,), L, dtype=torch.int64, device='cuda')
    kept, comb = torch.empty(rows, dtype=torch.int32, device='cuda'), torch.empty(rows, V, device='cuda')
    calls = {}
    for tag, ctl in (('min_len', dict(min_len=1)), ('top', dict(top_k=50, top_p=0.9))):
        common = dict(temperature=1.0, seed=5, site_sample=E.SITE_SAMPLE, row0=rows, hist=hist, kept=kept, **ctl)
        calls[tag + '/sample_filter_embed'] = lambda c=common: ops.sample_filter_embed(xs[0], Em, ids, out, logp, ln, t, end, p=0.0,
                                                                                       site=E.SITE_WORD, **c)
        calls[tag + '/sample_ens_1'] = lambda c=common: ops.sample_ens(xs[:1], [1.0], 0, comb, ids, logp, ln, t, end, **c)
        calls[tag + '/sample_ens_3'] = lambda c=common: ops.sample_ens(xs, [1.0] * 3, 0, comb, ids, logp, ln, t, end, **c)
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


def measure(rounds=7, reps=5, B=128, V=1000, n=5):
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
    ens = dlsg_amd.Ensemble(nets)
    seeds = iter(range(1, 10 ** 6))
    ens_sample = dlsg_amd.EnsembleSampleGraph(ens, frames, regions, n, 1.0)
    singles = [dlsg_amd.SampleGraph(net, frames, regions, n=n, share_encoder=True) for net in nets]
    ens_beam = dlsg_amd.EnsembleBeamGraph(ens, frames, regions, beam_size=n)

    def own():
        s = next(seeds)
        for g in singles:
            g(frames, regions, s)
    legs = [('ens_sample_3', lambda: ens_sample(frames, regions, next(seeds))), ('sample_x3', own),
            ('ens_beam_3', lambda: ens_beam(frames, regions))]
    ms = {name: [] for name, _ in legs}
    for _, call in legs:                                       # first replays outside the timing
        call()
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(legs)):
            name, call = legs[(i + r) % len(legs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'sampling from an ensemble as hipGraph replays: batch %d, n = %d, MSVD-shaped, vocabulary %d, eval mode; %d alternating '
                   'rounds of %d replays, ms per batch; step_us: microseconds per word-step launch on %d rows' % (B, n, V, rounds, reps, B * n)}
    for name, _ in legs:
        out[name] = summary(ms[name])
    out['ens_sample_3/sample_x3'] = round(out['ens_sample_3']['median'] / out['sample_x3']['median'], 4)
    out['ens_sample_3/ens_beam_3'] = round(out['ens_sample_3']['median'] / out['ens_beam_3']['median'], 4)
    ids, _, lens = ens_sample(frames, regions, 3)
    out['ens_sample_3']['mean_len'] = round(float(lens.double().mean()), 3)
    out['step_us'] = step_times(torch, nets[0], B * n, V, rounds)
    nets[0].ops.check_persistent()
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

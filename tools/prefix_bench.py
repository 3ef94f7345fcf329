"""Decoding under a forced prefix against the decode without one, at batch 128, MSVD-shaped, vocabulary 1000, as replayed hipGraphs,
one JSON line:
  * `nbest`, `nbest_p3`, `nbest_p8` -- `NBestBeamGraph` at beam 5 (no_repeat_ngram = 3, min_len = 4, length_penalty 0.7) without the
                                        keyword and with a prefix of 3 and of 8 words for every clip;
  * `sample`, `sample_p3`           -- `SampleGraph` at n = 5 without the keyword and with a prefix of 3 words.
The graphs are timed in alternating rounds (the order rotates) after a warm-up replay each; every figure is ms per batch including
the device synchronisation that makes the result readable; the median over the rounds, min, max and `spread` = (max - min) /
median.  `step_us`: the launches alone on the logits of a mid-caption step -- `beam_select_hist` and `beam_force_prefix` behind it
(all clips forced, and no clip forced), `sample_embed` and `sample_force_prefix` -- 200 back-to-back launches between two events
per round, microseconds per launch.  The prefixes are random word ids and the model's weights seeded noise: the figures say what
the launches cost.
usage: python3 tools/prefix_bench.py [rounds=11] [replays per round=5]
       python3 tools/prefix_bench.py steps [launches=200]      the two force kernels alone, for a kernel trace of their own
       python3 tools/prefix_bench.py against PARENT [replays=20]   the decodes WITHOUT the keyword in a checkout of the parent commit
                                                                (its library built) and in this tree: parent, tree, parent, tree,
                                                                a process each, ms per batch (median of the replays)
The measurement runs in child processes under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420
OPTS = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=3, min_len=4)


def summary(xs, digits=3):
    med = statistics.median(xs)
    return {'median': round(med, digits), 'min': round(min(xs), digits), 'max': round(max(xs), digits),
            'spread': round((max(xs) - min(xs)) / med, 4)}


def setup(root, B=128, V=1000):
    """the package of the checkout at `root`, an MSVD-shaped model with seeded weights on the device, and B clips"""
    import torch
    sys.path[:0] = [root, os.path.join(root, 'd-lsg-video-caption_amd')]
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    net.load_state_dict(synth_state_dict(net.state_dict(), 0))
    net = net.to('cuda').eval()
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    return torch, dlsg_amd, net, frames.cuda(), regions.cuda()


def prefix(torch, B, P, V):
    return torch.randint(4, V, (B, P), generator=torch.Generator().manual_seed(P)).cuda()


def timed(torch, graph, reps, *extra):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        graph(graph.frames, graph.regions, *extra)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def step_calls(torch, net, B=128, k=5, t=2, P=8):
    """the launches on (B*k, V) logits of a model-like scale: the select launch and the force launch behind it, the plain sampled
    step and the force launch behind it"""
    from dlsg_amd import engine as E
    ops, V, L = net.ops, net.decoder.vocab_size, net.decoder.max_words
    end, R = net.decoder.vocab('<end>'), B * k
    gen = torch.Generator(device='cuda').manual_seed(1)
    logits = torch.randn(R, V, device='cuda', generator=gen)
    hist = torch.randint(4, V, (2, R, L), device='cuda', generator=gen)
    last, lp = hist[0][:, t - 1].contiguous(), -torch.rand(R, device='cuda', generator=gen) * 5
    pred, back, rows = (torch.empty(R, dtype=torch.int64, device='cuda') for _ in range(3))
    nlp = torch.empty(R, device='cuda')
    step = (last, lp, pred, nlp, back, rows, k, end, hist[0], hist[1], t)
    px = prefix(torch, B, P, V)
    none = torch.full_like(px, -1)
    emb = net.decoder.word_embed.weight
    ids, out = torch.empty(R, dtype=torch.int64, device='cuda'), torch.empty(R, emb.shape[1], device='cuda')
    logp, lens = torch.empty(R, device='cuda'), torch.full((R,), L, dtype=torch.int64, device='cuda')
    kw = dict(temperature=1.0, seed=5, site=E.SITE_WORD, row0=(t + 1) * R)
    return {'beam_select_hist': lambda: ops.beam_select_hist(logits, *step, 3, 4),
            'beam_force_prefix': lambda: ops.beam_force_prefix([logits], [1.0], 0, *step, px),
            'beam_force_prefix_no_clip': lambda: ops.beam_force_prefix([logits], [1.0], 0, *step, none),
            'sample_embed': lambda: ops.sample_embed(logits, emb, ids, out, logp, lens, t, end, site_sample=E.SITE_SAMPLE, **kw),
            'sample_force_prefix': lambda: ops.sample_force_prefix(logits, emb, ids, out, logp, lens, t, px, L, rows_per_clip=k, **kw),
            'sample_force_prefix_no_row': lambda: ops.sample_force_prefix(logits, emb, ids, out, logp, lens, t, none, L, rows_per_clip=k, **kw)}


def step_times(torch, calls, rounds, launches=200):
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


def steps_only(launches=200):
    torch, dlsg_amd, net, frames, regions = setup(ROOT)
    calls = step_calls(torch, net)
    for name in ('beam_force_prefix', 'sample_force_prefix'):
        for _ in range(launches):
            calls[name]()
        torch.cuda.synchronize()
    print(json.dumps({'launched': launches, 'kernels': ['beam_force_prefix_kernel', 'sample_force_prefix_kernel']}))


def measure(rounds=11, reps=5, B=128, V=1000):
    torch, dlsg_amd, net, frames, regions = setup(ROOT, B, V)
    graphs = [('nbest', dlsg_amd.NBestBeamGraph(net, frames, regions, **OPTS), ())]
    graphs += [('nbest_p%d' % P, dlsg_amd.NBestBeamGraph(net, frames, regions, prefix=prefix(torch, B, P, V), **OPTS), ()) for P in (3, 8)]
    graphs += [('sample', dlsg_amd.SampleGraph(net, frames, regions, n=5), (7,)),
               ('sample_p3', dlsg_amd.SampleGraph(net, frames, regions, n=5, prefix=prefix(torch, B, 3, V)), (7,))]
    for _, g, extra in graphs:                                 # first replays outside the timing
        timed(torch, g, 1, *extra)
    ms = {name: [] for name, _, _ in graphs}
    for r in range(rounds):
        for i in range(len(graphs)):
            name, g, extra = graphs[(i + r) % len(graphs)]
            ms[name].append(timed(torch, g, reps, *extra))
    out = {'what': 'decoding under a forced prefix as hipGraph replays: batch %d, beam 5 / n = 5, MSVD-shaped, vocabulary %d; %d '
                   'alternating rounds of %d replays, ms per batch; synthetic model and prefixes' % (B, V, rounds, reps)}
    for name, g, extra in graphs:
        out[name] = dict(summary(ms[name]), rounds_ms=[round(x, 3) for x in ms[name]])
        if g.prefix is not None:
            base = 'nbest' if name.startswith('nbest') else 'sample'
            out[name]['over_' + base] = round(out[name]['median'] / out[base]['median'], 4)
            ids = g(frames, regions, *extra)[0]
            P = g.prefix.shape[1]
            rows = ids.view(B, -1, ids.shape[-1])[:, :, :P]
            out[name]['rows_that_begin_with_it'] = int((rows == g.prefix.unsqueeze(1)).all(2).sum())
            out[name]['rows'] = rows.shape[0] * rows.shape[1]
    out['step_us'] = step_times(torch, step_calls(torch, net), rounds)
    net.ops.check_persistent()
    print(json.dumps(out))


def figures(root, reps=20, B=128, V=1000):
    """the decodes without the keyword in the checkout at `root`: ms per batch, the median of `reps` replays each"""
    torch, dlsg_amd, net, frames, regions = setup(root, B, V)
    cons = torch.randint(4, V, (B, 2, 2), generator=torch.Generator().manual_seed(2)).cuda()
    graphs = [('nbest', dlsg_amd.NBestBeamGraph(net, frames, regions, **OPTS), ()),
              ('constrained', dlsg_amd.ConstrainedBeamGraph(net, frames, regions, cons, **OPTS), (cons,)),
              ('sample', dlsg_amd.SampleGraph(net, frames, regions, n=5), (7,)),
              ('sample_top_k', dlsg_amd.SampleGraph(net, frames, regions, n=5, top_k=20, min_len=4), (7,))]
    out = {}
    for name, g, extra in graphs:
        timed(torch, g, 2, *extra)
        out[name] = round(statistics.median(timed(torch, g, 1, *extra) for _ in range(reps)), 3)
    net.ops.check_persistent()
    print(json.dumps(out))


def against(parent, reps=20):
    """parent, tree, parent, tree: a process each; section 33's rule per figure"""
    runs = []
    for root in (parent, ROOT, parent, ROOT):
        cmd = ['timeout', '-k', '10', str(LIMIT_S // 2), sys.executable, os.path.abspath(__file__), 'figures', root, str(reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if res.returncode:
            return res.returncode
        runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = {'what': 'the decodes without the keyword as hipGraph replays, batch 128, ms per batch (median of %d replays): parent, tree, '
                   'parent, tree, a process each; limit = the parent\'s larger figure + the difference of its two' % reps}
    for name in runs[0]:
        p, t = [runs[0][name], runs[2][name]], [runs[1][name], runs[3][name]]
        limit = max(p) + abs(p[0] - p[1])
        out[name] = {'parent': p, 'tree': t, 'limit': round(limit, 3), 'inside': max(t) <= limit}
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    argv = sys.argv[1:]
    if argv[:1] == ['run']:
        measure(*[int(x) for x in argv[1:3]])
    elif argv[:1] == ['steps']:
        steps_only(*[int(x) for x in argv[1:2]])
    elif argv[:1] == ['figures']:
        figures(argv[1], *[int(x) for x in argv[2:3]])
    elif argv[:1] == ['against']:
        sys.exit(against(os.path.abspath(argv[1]), *[int(x) for x in argv[2:3]]))
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + argv[:2]
        sys.exit(subprocess.call(cmd))

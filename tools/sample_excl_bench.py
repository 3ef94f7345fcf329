"""What exclusions cost the sampled decodes, at batch 128, n = 5, MSVD-shaped, vocabulary 1000, as replayed hipGraphs, one JSON line:
  (a) `sample`          -- `SampleGraph(n=5, min_len=1)` without `exclude` (train mode), which launches what it launched before the
                           keyword existed, beside `parent_a` and `parent_b`: the same graph in a checkout of the parent commit
                           (`--parent DIR`, its library built), held by TWO processes of their own, so that the difference of the
                           two parent runs is the run-to-run spread, and `tree_a`, `tree_b`: this tree's graph held the same
                           way, by two processes that hold nothing else -- the like-for-like figures (`sample` itself shares its
                           process with eleven other graphs);
  (b) `sample_excl`     -- the same graph with exclude = <unk> and seventeen bad endings (word, <end>): 18 shared entries;
  (c) `swor`, `swor_excl` -- `StochasticBeamGraph(n=5)` without and with the same exclusions;
  (d) `scst_<baseline>`, `scst_<baseline>_excl` -- one `SCSTTrainer.step` (use_graphs, device CIDEr-D reward) without and with
                           `sample_options=dict(exclude=...)`, for the baselines 'mean' and 'greedy' (under exclusions the greedy
                           baseline is a second sampled decode, at temperature 0, instead of the greedy graph).
The legs are timed in alternating rounds (the order rotates; the parents' processes take their turns among them) after a warm-up
replay each; every figure is ms per call including the device synchronisation that makes the result readable: the median over the
rounds, min, max and `spread` = (max - min) / median.  Per leg with exclusions also `hits`, the number of sampled captions that hold
an excluded entry (`exclusions_hit`; 0 by the rule), and per sampling leg the mean caption length.  `step_us`: the word-step launch
alone -- `sample_filter_embed(min_len=1)` and `sample_excl_embed` with the table, `beam_select_gumbel` and `beam_select_gumbel_excl`
-- on the logits of a mid-caption step, 200 back-to-back launches between two events per round, microseconds per launch.
The model's weights are synthetic (seeded noise) and so is the table (word ids 4 .. 20 for the endings, not the words of
`BAD_ENDINGS`, which a synthetic vocabulary does not have): the figures say what the launches cost, not how captions improve.
usage: python3 tools/sample_excl_bench.py [--parent DIR] [rounds=7] [calls per round=5]
The measurement runs in child processes under `timeout`."""
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 540
B, N, V = 128, 5, 1000


def summary(xs, digits=3):
    med = statistics.median(xs)
    return {'median': round(med, digits), 'min': round(min(xs), digits), 'max': round(max(xs), digits),
            'spread': round((max(xs) - min(xs)) / med, 4)}


def setup(root):
    """the package of the checkout at `root`, an MSVD-shaped model with seeded weights on the device in train mode, and B clips"""
    import torch
    sys.path[:0] = [root, os.path.join(root, 'd-lsg-video-caption_amd')]
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    net.load_state_dict(synth_state_dict(net.state_dict(), 0))
    net = net.to('cuda').train()
    net.update_beam_size(1)
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    return torch, dlsg_amd, net, frames.cuda(), regions.cuda()


def table(torch, dlsg_amd, vocab):
    """<unk> and seventeen bad endings, on the device"""
    shared = torch.full((18, 2), -1, dtype=torch.int64)
    shared[0, 0] = vocab('<unk>')
    shared[1:, 0] = torch.arange(4, 21)
    shared[1:, 1] = vocab('<end>')
    return dlsg_amd.Exclusions(shared.cuda(), None)


def timed(torch, call, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def serve(root):
    """a process that holds the `sample` graph of the checkout at `root`: a line with a number of replays in, ms per replay out"""
    torch, dlsg_amd, net, frames, regions = setup(root)
    graph = dlsg_amd.SampleGraph(net, frames, regions, n=N, min_len=1)
    seeds = iter(range(1, 10 ** 6))
    call = lambda: graph(frames, regions, next(seeds))      # noqa: E731
    timed(torch, call, 1)
    print('ready', flush=True)
    for line in sys.stdin:
        print('%.6f' % timed(torch, call, int(line)), flush=True)


def step_times(torch, dlsg_amd, net, ex, rounds, launches=200, t=6):
    """the word-step launches alone, on B*N rows of logits of a model-like scale"""
    from dlsg_amd import engine as E
    ops, L, end = net.ops, net.decoder.max_words, net.decoder.vocab('<end>')
    rows, W = B * N, net.decoder.word_embed.weight.shape[1]
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(rows, V, device='cuda', generator=gen) * 3
    Em = torch.randn(V, W, device='cuda', generator=gen)
    hist_tm = torch.randint(4, V, (L, rows), device='cuda', generator=gen)
    ids, out = torch.empty(rows, dtype=torch.int64, device='cuda'), torch.empty(rows, W, device='cuda')
    logp, ln = torch.empty(rows, device='cuda'), torch.full((rows,), L, dtype=torch.int64, device='cuda')
    kept = torch.empty(rows, dtype=torch.int32, device='cuda')
    common = dict(temperature=1.0, p=0.5, seed=5, site=E.SITE_WORD, site_sample=E.SITE_SAMPLE, row0=rows, min_len=1, hist=hist_tm, kept=kept)
    hist = torch.randint(4, V, (2, rows, L), device='cuda', generator=gen)
    last, lp = hist[0][:, t - 1].contiguous(), -torch.rand(rows, device='cuda', generator=gen) * 5
    pred, back, sel = (torch.empty(rows, dtype=torch.int64, device='cuda') for _ in range(3))
    nlp = torch.empty(rows, device='cuda')
    G = torch.zeros(2, rows, dtype=torch.float64, device='cuda')
    step = (x, last, lp, pred, nlp, back, sel, N, end, hist[0], hist[1], t, G[0], G[1])
    gk = dict(temperature=1.0, seed=5, site_sample=E.SITE_SAMPLE, min_len=1)
    calls = {'sample_filter_embed': lambda: ops.sample_filter_embed(x, Em, ids, out, logp, ln, t, end, **common),
             'sample_excl_embed': lambda: ops.sample_excl_embed(x, Em, ids, out, logp, ln, t, end, excl_shared=ex.shared, rows_per_clip=N, **common),
             'beam_select_gumbel': lambda: ops.beam_select_gumbel(*step, **gk),
             'beam_select_gumbel_excl': lambda: ops.beam_select_gumbel_excl(*step, ex.shared, None, **gk)}
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


def measure(parent, rounds=7, reps=5):
    torch, dlsg_amd, net, frames, regions = setup(ROOT)
    vocab = net.decoder.vocab
    ex = table(torch, dlsg_amd, vocab)
    seeds = iter(range(1, 10 ** 6))
    graphs = {'sample': dlsg_amd.SampleGraph(net, frames, regions, n=N, min_len=1),
              'sample_excl': dlsg_amd.SampleGraph(net, frames, regions, n=N, min_len=1, exclude=ex),
              'swor': dlsg_amd.StochasticBeamGraph(net, frames, regions, n=N),
              'swor_excl': dlsg_amd.StochasticBeamGraph(net, frames, regions, n=N, exclude=ex)}
    legs = {name: (lambda g=g: g(frames, regions, next(seeds))) for name, g in graphs.items()}
    rng = random.Random(0)
    words = [vocab.idx2word[i] for i in range(4, V)]
    refs = {str(b): [' '.join(rng.choice(words) for _ in range(rng.randint(5, 12))) for _ in range(20)] for b in range(B)}
    reward = dlsg_amd.DeviceCiderD(refs, vocab)
    vids = [str(b) for b in range(B)]
    trainers = {}
    for baseline in ('mean', 'greedy'):
        for name, so in (('scst_' + baseline, None), ('scst_%s_excl' % baseline, dict(exclude=ex))):
            trainers[name] = dlsg_amd.SCSTTrainer(net, reward, n_samples=N, baseline=baseline, use_graphs=True, sample_options=so)
            legs[name] = lambda tr=trainers[name]: tr.step(frames, regions, vids)
    for name, call in legs.items():                            # captures and first replays outside the timing
        timed(torch, call, 2)
    turns = list(legs)
    others = {}
    if parent:
        for name, root in (('parent_a', parent), ('tree_a', ROOT), ('parent_b', parent), ('tree_b', ROOT)):
            others[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), 'serve', root], stdin=subprocess.PIPE,
                                            stdout=subprocess.PIPE, universal_newlines=True)
            assert others[name].stdout.readline().strip() == 'ready'
        turns[1:1] = ['parent_a', 'tree_a']
        turns[4:4] = ['parent_b', 'tree_b']
    ms = {name: [] for name in turns}
    for r in range(rounds):
        for i in range(len(turns)):
            name = turns[(i + r) % len(turns)]
            if name in others:
                others[name].stdin.write('%d\n' % reps)
                others[name].stdin.flush()
                ms[name].append(float(others[name].stdout.readline()))
            else:
                ms[name].append(timed(torch, legs[name], reps))
    for p in others.values():
        p.stdin.close()
        p.wait()
    out = {'what': 'sampled decodes without and under exclusions (<unk> and 17 bad endings) as hipGraph replays: batch %d, n = %d, MSVD-shaped, '
                   'vocabulary %d, train mode; %d alternating rounds of %d calls, ms per call; synthetic model and table' % (B, N, V, rounds, reps)}
    for name in turns:
        out[name] = dict(summary(ms[name]), rounds_ms=[round(x, 3) for x in ms[name]])
    for name, base in (('parent_a', 'parent_b'), ('tree_a', 'tree_b'), ('tree_a', 'parent_a'), ('tree_b', 'parent_b'), ('tree_a', 'parent_b'),
                       ('tree_b', 'parent_a'), ('sample', 'parent_a'), ('sample', 'parent_b'), ('sample_excl', 'sample'), ('swor_excl', 'swor'),
                       ('scst_mean_excl', 'scst_mean'), ('scst_greedy_excl', 'scst_greedy')):
        if name in out and base in out:
            out.setdefault('ratios', {})['%s/%s' % (name, base)] = round(out[name]['median'] / out[base]['median'], 4)
    L = net.decoder.max_words
    for name in ('sample', 'sample_excl'):
        ids, _, lens = graphs[name](frames, regions, 3)
        out[name]['hits'] = int(dlsg_amd.exclusions_hit(ids.view(B, N, L), lens.view(B, N), ex, V).sum())
        out[name]['mean_len'] = round(float(lens.double().mean()), 3)
    for name in ('swor', 'swor_excl'):
        ids, logp, lens = graphs[name](frames, regions, 3)
        out[name]['hits'] = int(dlsg_amd.exclusions_hit(ids, lens, ex, V)[logp > -float('inf')].sum())
        out[name]['mean_len'] = round(float(lens.double().mean()), 3)
    for tr in trainers.values():
        tr.trainer.check()
    out['step_us'] = step_times(torch, dlsg_amd, net, ex, rounds)
    net.ops.check_persistent()
    print(json.dumps(out))


if __name__ == '__main__':
    argv = sys.argv[1:]
    if argv[:1] == ['serve']:
        serve(argv[1])
    elif argv[:1] == ['run']:
        measure(argv[1] or None, *[int(x) for x in argv[2:4]])
    else:
        parent = ''
        if argv[:1] == ['--parent']:
            parent, argv = os.path.abspath(argv[1]), argv[2:]
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run', parent] + argv[:2]
        sys.exit(subprocess.call(cmd))

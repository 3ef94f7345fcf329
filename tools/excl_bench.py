"""Beam search under exclusions against the n-best beam search, at batch 128, beam 5, MSVD-shaped, vocabulary 1000,
no_repeat_ngram = 3, min_len = 4, length_penalty 0.7, as replayed hipGraphs, one JSON line:
  * `nbest`          -- `NBestBeamGraph` without `exclude`: the comparator, which launches what it launched before the keyword existed;
  * `parent_nbest`   -- the same graph in a checkout of the parent commit (`--parent DIR`, its library built), in a process of its own;
  * `excl_unk`       -- `NBestBeamGraph(exclude=...)` with the one shared entry (<unk>,);
  * `excl_endings`   -- with <unk> and seventeen bad endings (word, <end>): 18 shared entries;
  * `excl_per_clip`  -- with those and eight entries of one to three words per clip;
  * `excl_64_words`  -- with 64 shared one-word entries, a list of words to keep out: the longest list a row can get from one table.
The graphs are timed in alternating rounds (the order rotates; the parent's process takes its turn among them) after a warm-up
replay each; every figure is ms per batch including the device synchronisation that makes the result readable; the median over the
rounds, min, max and `spread` = (max - min) / median.  Per graph with exclusions also `hits`, the number of captions of finite
score that hold an excluded entry (`exclusions_hit`) -- 0 by the step's rule, so the tool doubles as a check at the workload's size
--, and the mean score of the best caption beside the unrestricted one's.  `step_us`: the select launch alone -- `beam_select_hist`,
`beam_select_ens` with one member and `beam_select_excl` without a table and with each of the tables -- on the logits of a mid-caption step, 200
back-to-back launches between two events per round, microseconds per launch.
The model's weights are synthetic (seeded noise) and so are the tables (word ids, not the words of `BAD_ENDINGS`, which a synthetic
vocabulary does not have): the figures say what the launches cost, not how captions improve.
usage: python3 tools/excl_bench.py [--parent DIR] [rounds=11] [replays per round=5]
       python3 tools/excl_bench.py steps [launches=200]     the three step kernels alone, for a kernel trace of their own
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
TABLES = ('excl_unk', 'excl_endings', 'excl_per_clip', 'excl_64_words')


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


def tables(torch, dlsg_amd, vocab, B, V):
    """the `Exclusions` of the measurement, on the device, P = 3 throughout"""
    gen = torch.Generator().manual_seed(3)
    unk, end = vocab('<unk>'), vocab('<end>')
    shared = torch.full((18, 3), -1, dtype=torch.int64)
    shared[0, 0] = unk
    shared[1:, 0] = torch.arange(4, 21)
    shared[1:, 1] = end
    per_clip = torch.randint(4, V, (B, 8, 3), generator=gen)
    for a in range(8):                                         # entries of one, two and three words
        per_clip[:, a, 1 + a % 3:] = -1
    words = torch.full((64, 3), -1, dtype=torch.int64)
    words[:, 0] = torch.randperm(V - 4, generator=gen)[:64] + 4
    E = dlsg_amd.Exclusions
    return {'excl_64_words': E(words.cuda(), None), 'excl_unk': E(shared[:1].cuda(), None), 'excl_endings': E(shared.cuda(), None), 'excl_per_clip': E(shared.cuda(), per_clip.cuda())}


def timed(torch, graph, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        graph(graph.frames, graph.regions)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def serve(root):
    """a process that holds the `nbest` graph of the checkout at `root`: a line with a number of replays in, ms per batch out"""
    torch, dlsg_amd, net, frames, regions = setup(root)
    graph = dlsg_amd.NBestBeamGraph(net, frames, regions, **OPTS)
    timed(torch, graph, 1)
    print('ready', flush=True)
    for line in sys.stdin:
        print('%.6f' % timed(torch, graph, int(line)), flush=True)


def step_calls(torch, dlsg_amd, net, ex, B=128, k=5, t=6):
    """the select launches on (B*k, V) logits of a model-like scale"""
    ops, V, L = net.ops, net.decoder.vocab_size, net.decoder.max_words
    end, R = net.decoder.vocab('<end>'), B * k
    gen = torch.Generator(device='cuda').manual_seed(1)
    logits = torch.randn(R, V, device='cuda', generator=gen)
    hist = torch.randint(4, V, (2, R, L), device='cuda', generator=gen)
    last, lp = hist[0][:, t - 1].contiguous(), -torch.rand(R, device='cuda', generator=gen) * 5
    pred, back, rows = (torch.empty(R, dtype=torch.int64, device='cuda') for _ in range(3))
    nlp = torch.empty(R, device='cuda')
    step = (last, lp, pred, nlp, back, rows, k, end, hist[0], hist[1], t)
    calls = {'beam_select_hist': lambda: ops.beam_select_hist(logits, *step, 3, 4),
             'beam_select_ens': lambda: ops.beam_select_ens([logits], [1.0], 0, *step, 3, 4),
             'beam_select_excl_empty': lambda: ops.beam_select_excl([logits], [1.0], 0, *step, None, None, 3, 4)}
    for name in TABLES:
        calls['beam_select_' + name] = lambda e=ex[name]: ops.beam_select_excl([logits], [1.0], 0, *step, e.shared, e.per_clip, 3, 4)
    return calls


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
    calls = step_calls(torch, dlsg_amd, net, tables(torch, dlsg_amd, net.decoder.vocab, 128, net.decoder.vocab_size))
    for name in ('beam_select_hist', 'beam_select_ens', 'beam_select_excl_per_clip'):
        for _ in range(launches):
            calls[name]()
        torch.cuda.synchronize()
    print(json.dumps({'launched': launches, 'kernels': ['beam_select_hist_kernel', 'beam_select_ens_kernel', 'beam_select_excl_kernel']}))


def measure(parent, rounds=11, reps=5, B=128, V=1000):
    torch, dlsg_amd, net, frames, regions = setup(ROOT, B, V)
    ex = tables(torch, dlsg_amd, net.decoder.vocab, B, V)
    graphs = [('nbest', dlsg_amd.NBestBeamGraph(net, frames, regions, **OPTS))]
    graphs += [(name, dlsg_amd.NBestBeamGraph(net, frames, regions, exclude=ex[name], **OPTS)) for name in TABLES]
    for _, g in graphs:                                        # first replays outside the timing
        timed(torch, g, 1)
    turns = [name for name, _ in graphs]
    other = None
    if parent:
        other = subprocess.Popen([sys.executable, os.path.abspath(__file__), 'serve', parent], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 universal_newlines=True)
        assert other.stdout.readline().strip() == 'ready'
        turns.insert(1, 'parent_nbest')
    ms = {name: [] for name in turns}
    held = dict(graphs)
    for r in range(rounds):
        for i in range(len(turns)):
            name = turns[(i + r) % len(turns)]
            if name == 'parent_nbest':
                other.stdin.write('%d\n' % reps)
                other.stdin.flush()
                ms[name].append(float(other.stdout.readline()))
            else:
                ms[name].append(timed(torch, held[name], reps))
    if other is not None:
        other.stdin.close()
        other.wait()
    out = {'what': 'beam search under exclusions and the n-best beam search as hipGraph replays: batch %d, beam 5, MSVD-shaped, vocabulary '
                   '%d; %d alternating rounds of %d replays, ms per batch; synthetic model and tables' % (B, V, rounds, reps)}
    free = held['nbest'](frames, regions)[1][:, 0].clone()
    for name in turns:
        out[name] = dict(summary(ms[name]), rounds_ms=[round(x, 3) for x in ms[name]])
        if name != 'nbest':
            out[name]['over_nbest'] = round(out[name]['median'] / out['nbest']['median'], 4)
        if name in ex:
            ids, scores, lens = held[name](frames, regions)
            hit = dlsg_amd.exclusions_hit(ids, lens, held[name].exclude, V)
            out[name]['hits'] = int(hit[scores > -float('inf')].sum())
            out[name]['mean_score'] = round(float(scores[:, 0].mean()), 4)
            out[name]['changed_clips'] = int((ids[:, 0] != held['nbest'].out[0][:, 0]).any(1).sum())
    out['nbest']['mean_score'] = round(float(free.mean()), 4)
    out['step_us'] = step_times(torch, step_calls(torch, dlsg_amd, net, ex), rounds)
    net.ops.check_persistent()
    print(json.dumps(out))


if __name__ == '__main__':
    argv = sys.argv[1:]
    if argv[:1] == ['serve']:
        serve(argv[1])
    elif argv[:1] == ['run']:
        measure(argv[1] or None, *[int(x) for x in argv[2:4]])
    elif argv[:1] == ['steps']:
        steps_only(*[int(x) for x in argv[1:2]])
    else:
        parent = ''
        if argv[:1] == ['--parent']:
            parent, argv = os.path.abspath(argv[1]), argv[2:]
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run', parent] + argv[:2]
        sys.exit(subprocess.call(cmd))

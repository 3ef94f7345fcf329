"""Scoring given captions, at batch 128 x 5 candidates, MSVD-shaped, vocabulary 1000, one JSON line:
  (a) `kernel_us`   -- the `dlsg_seq_logprob` launch alone on the teacher-forced logits of the 640 candidates a beam-5 search
                       returned, for M = 1 and M = 3 members (mode 'prob'), with and without `tok_rank`: 200 back-to-back launches
                       between two events per round, microseconds per launch; `read_bytes` = sum of len x V x 4 x M, the rows the
                       kernel has to read once, and `hbm_fraction` = read_bytes / time / 8 TB/s (the MI355X's peak HBM bandwidth);
  (b) `torch_us`    -- the comparator, code this feature does not touch: torch.log_softmax + gather over the WHOLE (L, R, V)
                       tensor of each member on the same buffers (M = 3: plus the logsumexp over the members), timed the same way;
  (c) `graphs_ms`   -- as replayed hipGraphs, ms per batch including the synchronisation that makes the result readable:
                       `nbest` (`NBestBeamGraph`, one model searches), `rescore` (`RescoreBeamGraph`: that search, then three
                       members rescore its five beams) and `ensemble` (`EnsembleBeamGraph` of the same three members).
Everything is timed in alternating rounds (the order rotates) after a warm-up; the median over the rounds, min, max and
`spread` = (max - min) / median.  The models' weights are synthetic (seeded noise): the figures say what the pieces cost, not
how captions improve.
usage: python3 tools/score_bench.py [rounds=11] [replays per round=5]
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 400
OPTS = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=3, min_len=4)
HBM_BYTES_PER_S = 8.0e12


def summary(xs, digits=3):
    med = statistics.median(xs)
    return {'median': round(med, digits), 'min': round(min(xs), digits), 'max': round(max(xs), digits),
            'spread': round((max(xs) - min(xs)) / med, 4)}


def event_rounds(torch, calls, rounds, launches=200):
    """every call `launches` times back to back between two events, in rotating order; round 0 warms up -> name -> [us per launch]"""
    us = {name: [] for name in calls}
    names = list(calls)
    for r in range(rounds + 1):
        for i in range(len(names)):
            name = names[(i + r) % len(names)]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                calls[name]()
            b.record()
            b.synchronize()
            if r:
                us[name].append(a.elapsed_time(b) / launches * 1e3)
    return us


def measure(rounds=11, reps=5, B=128, V=1000):
    import torch
    for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    nets = []
    for seed in (0, 3, 4):
        torch.manual_seed(0)
        net = dlsg_amd.CapGnnModel(args, vocab)
        net.load_state_dict(synth_state_dict(net.state_dict(), seed))
        nets.append(net.to('cuda').eval())
    ens = dlsg_amd.Ensemble(nets)
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    frames, regions = frames.cuda(), regions.cuda()
    ops, end = nets[0].ops, vocab('<end>')
    with torch.no_grad():
        ids, _, lens = nets[0].beam_search(frames, regions, **OPTS)
        n, L = ids.shape[1], ids.shape[2]
        rows = ids.reshape(B * n, L).contiguous()
        logits = ens.teacher_logits(frames, regions, rows, seq_per_clip=n)
    words = int(lens.sum())
    out = {'what': 'scoring given captions: batch %d x %d candidates of a beam search, MSVD-shaped, vocabulary %d, L = %d; %d '
                   'alternating rounds; synthetic models' % (B, n, V, L, rounds),
           'candidates': B * n, 'mean_len': round(words / (B * n), 3)}

    # (a) the launch alone, (b) log_softmax + gather over the whole tensor
    tgt = rows.t().unsqueeze(2)
    logw = torch.log(torch.tensor(ens.weights, device='cuda')).view(-1, 1, 1)

    def plain(M):
        lp = [torch.log_softmax(x, 2).gather(2, tgt).squeeze(2) for x in logits[:M]]
        return lp[0] if M == 1 else torch.logsumexp(torch.stack(lp) + logw[:M], 0)
    calls = {}
    for M in (1, 3):
        w = [1.0] * M
        calls['M%d' % M] = lambda M=M, w=w: ops.seq_logprob(logits[:M], w, 0, rows, None, 0.7, True, False, end=end)
        calls['M%d_rank' % M] = lambda M=M, w=w: ops.seq_logprob(logits[:M], w, 0, rows, None, 0.7, True, True, end=end)
        calls['torch_M%d' % M] = lambda M=M: plain(M)
    with torch.no_grad():
        us = event_rounds(torch, calls, rounds)
    out['kernel_us'], out['torch_us'] = {}, {}
    for name, v in us.items():
        s = dict(summary(v, 2), rounds_us=[round(x, 2) for x in v])
        M = 3 if 'M3' in name else 1
        if name.startswith('torch'):
            s['read_bytes'] = L * B * n * V * 4 * M
            out['torch_us'][name[6:]] = s
        else:
            s['read_bytes'] = words * V * 4 * M
            s['hbm_fraction'] = round(s['read_bytes'] / (s['median'] * 1e-6) / HBM_BYTES_PER_S, 4)
            out['kernel_us'][name] = s
    for M in (1, 3):
        out['kernel_us']['M%d' % M]['over_torch'] = round(out['kernel_us']['M%d' % M]['median'] / out['torch_us']['M%d' % M]['median'], 4)

    # (c) the captured forms
    graphs = [('nbest', dlsg_amd.NBestBeamGraph(nets[0], frames, regions, **OPTS)),
              ('rescore', dlsg_amd.RescoreBeamGraph(nets[0], ens, frames, regions, n_best=1, **OPTS)),
              ('ensemble', dlsg_amd.EnsembleBeamGraph(ens, frames, regions, **OPTS))]
    ms = {name: [] for name, _ in graphs}
    for name, g in graphs:
        g(g.frames, g.regions)
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(graphs)):
            name, g = graphs[(i + r) % len(graphs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(reps):
                g(g.frames, g.regions)
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out['graphs_ms'] = {name: dict(summary(ms[name]), rounds_ms=[round(x, 3) for x in ms[name]]) for name, _ in graphs}
    for name in ('rescore', 'ensemble'):
        out['graphs_ms'][name]['over_nbest'] = round(out['graphs_ms'][name]['median'] / out['graphs_ms']['nbest']['median'], 4)
    order = graphs[1][1](frames, regions)[3]
    out['rescore_changes_best'] = round(float((order[:, 0] != 0).double().mean()), 4)
    ops.check_persistent()
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        measure(*[int(x) for x in sys.argv[2:4]])
    else:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run'] + sys.argv[1:3]
        sys.exit(subprocess.call(cmd))

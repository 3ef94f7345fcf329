"""The soft-target CrossEntropy (`dlsg_ce_ragged_soft`: label smoothing, ensemble word-level distillation), one JSON line per part.
  kernel -- 1 664 rows (26 x 64, time-major, lengths 3..26) x V in {1 000, 10 000}, device-event time per launch:
              `ce_ragged`              dlsg_ce_ragged, the launch the soft one replaces;
              `soft_m0`                dlsg_ce_ragged_soft, M = 0, eps = 0.1: the same bytes (row read three times, dlogits written once);
              `soft_m{1,3}_{prob,logprob}`  with teachers, and the achieved bytes / s from the byte count
                                       ((3 + passes * M) * V * 4 + V * 4) per counted row, passes = 3 ('prob') or 4 ('logprob').
  step   -- the MSVD-shaped train step at batch 64, vocabulary 1 000, use_graphs=True, ms per step:
              `plain`                  (a) Trainer();
              `smooth`                 (b) Trainer(label_smoothing=0.1): against (a);
              `distill_3`              (c) Trainer(teacher=Ensemble of three members, mode 'prob', distill_weight=0.5);
              `teacher_3`              (d) the three members' teacher-forced eval forwards alone, as one replayed hipGraph:
                                       (c) against (a) + (d) is what the loss itself costs.
The legs of a part live in one process and are timed in alternating rounds (the order rotates from round to round); `spread` of a
leg is (max - min) / median over its rounds.
usage: python3 tools/soft_ce_bench.py [kernel|step|all] [rounds=9]
The measurement runs in a child process under `timeout`."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420


def _paths():
    for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)


def _stats(xs, unit, digits):
    med = statistics.median(xs)
    return {'median_' + unit: round(med, digits), 'min_' + unit: round(min(xs), digits), 'max_' + unit: round(max(xs), digits),
            'spread': round((max(xs) - min(xs)) / med, 4)}


def measure_kernel(rounds=9, launches=200, B=64, L=26):
    import torch
    _paths()
    from dlsg_amd.graphs import capture
    from dlsg_amd.hip import HipOps
    ops = HipOps()
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(3, L + 1, (B,), generator=g).cuda()
    counted = int(lens.sum())
    for V in (1000, 10000):
        logits = torch.randn(L, B, V, generator=g).cuda()
        teachers = [torch.randn(L, B, V, generator=g).cuda() for _ in range(3)]
        tg = torch.randint(0, V, (B, L), generator=g).cuda()
        dl = torch.empty_like(logits)
        rl = torch.empty(3 * L * B, device='cuda')
        loss = torch.empty(3, device='cuda')
        legs = [('ce_ragged', 0, 0, lambda: ops.ce_ragged(logits, tg, lens, dl, rl, loss[:1], True)),
                ('soft_m0', 0, 0, lambda: ops.ce_ragged_soft(logits, tg, lens, dl, rl, loss, True, smoothing=0.1))]
        for M in (1, 3):
            for mode, name in ((0, 'prob'), (1, 'logprob')):
                legs.append(('soft_m%d_%s' % (M, name), M, 3 + mode,
                             lambda M=M, mode=mode: ops.ce_ragged_soft(logits, tg, lens, dl, rl, loss, True, smoothing=0.1,
                                                                       teachers=teachers[:M], mode=mode, alpha=0.5)))
        us = {leg[0]: [] for leg in legs}
        # a leg's launches are replayed as one hipGraph: the host (whose wrappers differ in what they check) is out of the timing
        graphs = {}
        for name, _, _, fn in legs:
            graphs[name] = capture(logits.device, lambda fn=fn: [fn() for _ in range(launches)] and None)[0]
            graphs[name].replay()
        torch.cuda.synchronize()
        for r in range(rounds):
            for i in range(len(legs)):
                name = legs[(i + r) % len(legs)][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[name].replay()
                e1.record()
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) / launches * 1e3)
        out = {'what': 'ce kernels (row kernel + loss sum): %d rows (%d counted) x V = %d, %d alternating rounds of %d launches replayed as one '
                       'hipGraph, us per launch between device events' % (L * B, counted, V, rounds, launches), 'V': V}
        for name, M, passes, _ in legs:
            out[name] = _stats(us[name], 'us', 2)
            if M:
                out[name]['GB_per_s'] = round(counted * ((3 + passes * M) * V * 4 + V * 4) / (out[name]['median_us'] * 1e-6) / 1e9, 1)
        out['soft_m0_over_ce_ragged'] = round(out['soft_m0']['median_us'] / out['ce_ragged']['median_us'], 4)
        print(json.dumps(out), flush=True)


def measure_step(rounds=9, reps=5, B=64, V=1000):
    import torch
    _paths()
    import dlsg_amd
    from dlsg_amd.graphs import capture
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)

    def net(seed, train):
        torch.manual_seed(0)
        m = dlsg_amd.CapGnnModel(args, vocab)
        m.load_state_dict(synth_state_dict(m.state_dict(), seed))
        return m.to('cuda').train(train)

    frames, regions, caps, lens = synth_batch(args, V, B, 1)
    frames, regions, caps = frames.cuda(), regions.cuda(), caps[:, :26].contiguous().cuda()
    lens = torch.as_tensor(lens).cuda()
    teacher = dlsg_amd.Ensemble([net(10 + i, False) for i in range(3)], mode='prob')
    trainers = {'plain': dlsg_amd.Trainer(net(0, True), use_graphs=True, check_every=0),
                'smooth': dlsg_amd.Trainer(net(0, True), use_graphs=True, check_every=0, label_smoothing=0.1),
                'distill_3': dlsg_amd.Trainer(net(0, True), use_graphs=True, check_every=0, teacher=teacher, distill_weight=0.5)}
    legs = [(name, (lambda tr=tr: tr.step(frames, regions, caps, lens, 1.0))) for name, tr in trainers.items()]
    for _, fn in legs:                                          # capture + first replays outside the timing
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for m in teacher.members:
        m.flatten_parameters_()
    tgraph, _ = capture(frames.device, lambda: teacher.teacher_logits(frames, regions, caps))
    legs.append(('teacher_3', tgraph.replay))
    tgraph.replay()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for r in range(rounds):
        for i in range(len(legs)):
            name, fn = legs[(i + r) % len(legs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'train step as hipGraph replays: batch %d, MSVD-shaped, vocabulary %d; %d alternating rounds of %d steps, ms per '
                   'step' % (B, V, rounds, reps)}
    for name, _ in legs:
        out[name] = _stats(ms[name], 'ms', 3)
        out[name]['rounds_ms'] = [round(x, 3) for x in ms[name]]
    a, b, c, d = [out[k]['median_ms'] for k in ('plain', 'smooth', 'distill_3', 'teacher_3')]
    out['smooth_minus_plain_ms'] = round(b - a, 3)
    out['distill_3_minus_plain_and_teacher_3_ms'] = round(c - (a + d), 3)
    out['loss_parts_distill_3'] = [round(float(x), 5) for x in trainers['distill_3'].last_loss_parts]
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'run':
        part, rounds = sys.argv[2], int(sys.argv[3])
        if part in ('kernel', 'all'):
            measure_kernel(rounds)
        if part in ('step', 'all'):
            measure_step(rounds)
    else:
        part = sys.argv[1] if len(sys.argv) > 1 else 'all'
        rounds = sys.argv[2] if len(sys.argv) > 2 else '9'
        if part not in ('kernel', 'step', 'all'):
            sys.exit(__doc__)
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'run', part, rounds]
        sys.exit(subprocess.call(cmd))

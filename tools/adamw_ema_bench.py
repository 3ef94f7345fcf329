"""What weight decay and the averaged weights cost the captured train step: MSVD-shaped, batch 64, vocabulary 1000, dropout on, one
JSON line with a leg per form of the update:
  * `off`        -- Trainer(use_graphs=True): the step as bench.py times it (dlsg_adam);
  * `decay`      -- weight_decay=1e-2 under decay_filter = p.ndim > 1: dlsg_adamw_ema with a decay table per trainable range;
  * `ema`        -- ema_decay=0.999: dlsg_adamw_ema with the average, 36 B per parameter against 28;
  * `decay_ema`  -- both;
  * `off_lerp`   -- the `off` step followed by one `ema.lerp_(weights, 1 - d)` launch over the arena: the unfused way to keep the
                    average, which reads the fresh weights again (12 B per parameter on top of Adam's 28).
The trainers (a model each, same weights and batch) live in one process and are timed in alternating rounds (the order rotates from
round to round); every figure is ms per step over a round of replays with one device synchronisation at its end.  `spread` is
(max - min) / median over a leg's rounds: `off`'s own spread is the yardstick for the differences.
usage: python3 tools/adamw_ema_bench.py [--tree DIR] [rounds=9] [steps per round=20]
       python3 tools/adamw_ema_bench.py [--tree DIR] kernels LEG [steps=10]     -- one leg's replays only, for a per-kernel trace
--tree DIR imports dlsg_amd from another checkout (the parent build: only `off` and `off_lerp` exist there, the others are left out).
The measurement runs in a child process under `timeout`; under a profiler run that child's own command, so that the traced
program is the one that opens the GPU:
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o adam -- python3 tools/adamw_ema_bench.py run-kernels ema"""
import inspect
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420
D = 0.999


def ndim_filter(name, p):
    return p.ndim > 1


LEGS = {'off': {}, 'decay': dict(weight_decay=1e-2, decay_filter=ndim_filter), 'ema': dict(ema_decay=D),
        'decay_ema': dict(weight_decay=1e-2, decay_filter=ndim_filter, ema_decay=D), 'off_lerp': {}}


def make_trainer(tree, B=64, V=1000, **kw):
    import torch
    for p in (tree, os.path.join(tree, 'd-lsg-video-caption_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    net.load_state_dict(synth_state_dict(net.state_dict(), 0))
    net = net.to('cuda').train()
    batch = [t.cuda() for t in synth_batch(args, V, B, 1)]
    tr = dlsg_amd.Trainer(net, use_graphs=True, check_every=0, **kw)
    eps = dlsg_amd.ss_epsilon(0)
    for _ in range(3):                                          # capture + first replays outside the timing
        tr.step(*batch, eps)
    torch.cuda.synchronize()
    return tr, tr.static_inputs() or batch, eps


def legs_of(tree):
    sys.path.insert(0, os.path.join(tree, 'd-lsg-video-caption_amd'))
    import dlsg_amd
    new = 'ema_decay' in inspect.signature(dlsg_amd.Trainer.__init__).parameters
    return [k for k in LEGS if new or not LEGS[k]]


def stepper(name, tr, fb, eps):
    if name != 'off_lerp':
        return lambda: tr.step(*fb, eps)
    flat = tr.model._flat
    avg = flat.clone()

    def step():
        tr.step(*fb, eps)
        avg.lerp_(flat, 1.0 - D)
    return step


def measure(tree, rounds=9, reps=20):
    import torch
    random.seed(12)
    legs = [(name, stepper(name, *make_trainer(tree, **LEGS[name]))) for name in legs_of(tree)]
    ms = {name: [] for name, _ in legs}
    for r in range(rounds):
        for i in range(len(legs)):
            name, step = legs[(i + r) % len(legs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    out = {'what': 'captured train step, MSVD-shaped, batch 64, vocabulary 1000, dropout on, by form of the update; %d alternating '
                   'rounds of %d replays, ms per step' % (rounds, reps)}
    for name, _ in legs:
        med = statistics.median(ms[name])
        out[name] = {'median_ms': round(med, 3), 'min_ms': round(min(ms[name]), 3), 'max_ms': round(max(ms[name]), 3),
                     'spread': round((max(ms[name]) - min(ms[name])) / med, 4), 'rounds_ms': [round(x, 3) for x in ms[name]]}
        if name != 'off':
            out[name]['minus_off_ms'] = round(med - out['off']['median_ms'], 3)
    print(json.dumps(out))


def kernels(tree, leg, steps=10):
    import torch
    random.seed(12)
    tr, fb, eps = make_trainer(tree, **LEGS[leg])
    step = stepper(leg, tr, fb, eps)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    tabs = getattr(tr, '_decay_tabs', {})
    print(json.dumps({'leg': leg, 'replays': steps + 2, 'trainable_ranges': len(tr._train_ranges),
                      'parameter_MB': round(4e-6 * sum(hi - lo for lo, hi in tr._train_ranges), 1),
                      'decay_intervals': [0 if t is None else int(t.shape[0]) for _, t in tabs.values()]}))


if __name__ == '__main__':
    argv = sys.argv[1:]
    tree = ROOT
    if argv[:1] == ['--tree']:
        tree, argv = os.path.abspath(argv[1]), argv[2:]
    if argv[:1] == ['run']:
        measure(tree, *[int(x) for x in argv[1:3]])
    elif argv[:1] == ['run-kernels']:
        kernels(tree, argv[1], *[int(x) for x in argv[2:3]])
    else:
        mode, rest = ('run-kernels', argv[1:3]) if argv[:1] == ['kernels'] else ('run', argv[:2])
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--tree', tree, mode] + rest
        sys.exit(subprocess.call(cmd))

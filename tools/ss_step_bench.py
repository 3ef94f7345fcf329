"""Trainer.step at batch 64, MSVD-shaped, fp32, replayed graph, at several scheduled-sampling probabilities.

bench.py measures epoch 0 (eps = 0.95: about one of the 25 coin-driven word steps samples its word); the schedule
(dlsg_amd.ss_epsilon, run_gun.py:136) decays to 0.6, where about ten of them do.  This tool times the same step at each
--eps with the same weights, batch and coin seed, so that a change to the sampled word step can be priced where training
spends most of its epochs.

    python tools/ss_step_bench.py [--eps 0.95 0.6] [--steps 30] [--warmup 3] [--tree DIR]

--tree DIR imports the package of another checkout (built there) instead of this one: the same script then measures two
trees in one session.  One JSON line per eps: ms_per_step, the mean number of sampled word steps per step, the loss."""
import argparse
import json
import os
import random
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--eps', type=float, nargs='+', default=[0.95, 0.6])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--seed', type=int, default=12)
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, 'd-lsg-video-caption_amd')]
    import dlsg_amd
    from dlsg_amd.synth import synth_state_dict, synth_batch
    assert os.path.abspath(dlsg_amd.__file__).startswith(tree), dlsg_amd.__file__

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    args, V = dlsg_amd.msvd_shaped(), 1000
    vocab = dlsg_amd.make_vocab(V)
    for eps in a.eps:
        torch.manual_seed(0)
        net = dlsg_amd.CapGnnModel(args, vocab)
        net.load_state_dict(synth_state_dict(net.state_dict(), 0))
        net = net.to(dev).train()
        batch = [t.to(dev) for t in synth_batch(args, V, a.batch, 1)]
        tr = dlsg_amd.Trainer(net, use_graphs=True, graph_fallback=False)
        random.seed(a.seed)
        drawn = []
        draw = net._draw_coins

        def counted(L, infer, tf_ratio):
            coins = draw(L, infer, tf_ratio)
            drawn.append(sum(1 for c in coins[:-1] if not c))      # the last step's coin chooses no next word
            return coins
        net._draw_coins = counted
        for _ in range(a.warmup):
            tr.step(*batch, eps)
        if tr.static_inputs() is not None:
            batch = tr.static_inputs()
        torch.cuda.synchronize()
        del drawn[:]
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = tr.step(*batch, eps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({'tree': tree, 'eps': eps, 'batch': a.batch, 'steps': a.steps, 'ms_per_step': round(1e3 * dt / a.steps, 3),
                          'sampled_word_steps_per_step': round(sum(drawn) / max(1, len(drawn)), 2), 'final_loss': round(float(loss), 5)}),
              flush=True)
        del tr, net


if __name__ == '__main__':
    main()

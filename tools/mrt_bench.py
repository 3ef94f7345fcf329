"""Minimum-risk training at the MSVD shape (batch 64, n = 5 candidates per clip, vocabulary 1000, train mode), one JSON line per part.
  * `step` (default) -- the Trainer's step as replayed graphs on the same 320 caption rows: the risk form (`step(risk=...)`) against
    the weighted form (`step(seq_weights=...)`), alternating rounds in one process; the expected difference is one more read of
    the logits.
  * `kernels` -- `dlsg_risk_rows`, `dlsg_risk_grad` and `dlsg_ce_ragged_weighted` alone on (26, 320, V) logits, V = 1000 and
    10 000: HIP events around back-to-back launches replayed from a hipGraph, alternating rounds, with the bytes each launch has to
    move (rows kernel: the counted rows once; grad kernel: the counted rows read once and every row written once; CrossEntropy: the
    same as the grad kernel -- its two further reads of a row are served by the L2) and the achieved bytes/s.
  * `mrt` -- a whole `MRTTrainer` step with the device reward for 'swor' and 'beam' (n = 5, beam size 5) against an `SCSTTrainer`
    step, graph replays, alternating rounds.
usage: python3 tools/mrt_bench.py [step|kernels|mrt] [steps=20] [batch=64] [n=5] [rounds=3]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import dlsg_amd  # noqa: E402
from scst_bench import event_ms, setup, timed  # noqa: E402


def spread(v):
    return {'ms': v, 'best_ms': min(v), 'spread': round((max(v) - min(v)) / min(v), 4)}


def fixed_rows(net, B, n, V, L):
    """B*n caption rows of 5..12 seeded words and <end>, their lengths and seeded rewards"""
    g = torch.Generator().manual_seed(3)
    end = net.decoder.vocab('<end>')
    lens = torch.randint(6, 14, (B * n,), generator=g)
    ids = torch.randint(4, V, (B * n, L), generator=g)
    for r in range(B * n):
        ids[r, int(lens[r]) - 1:] = end
    return ids.cuda(), lens.cuda(), torch.rand(B * n, generator=g, dtype=torch.float64).cuda()


def step_main(steps=20, B=64, n=5, rounds=3):
    net, vocab, frames, regions, refs = setup(B)
    L = net.decoder.max_words
    ids, lens, rewards = fixed_rows(net, B, n, 1000, L)
    adv = (rewards - rewards.view(B, n).mean(1, keepdim=True).expand(B, n).reshape(-1)).float()
    risk = dict(rewards=rewards, n=n, alpha=1.0, length_penalty=1.0)
    forms = {'weighted': lambda tr: tr.step(frames, regions, ids, lens, 1.0, max_len=L, seq_weights=adv, seq_per_clip=n),
             'risk': lambda tr: tr.step(frames, regions, ids, lens, 1.0, max_len=L, risk=risk, seq_per_clip=n)}
    trainers = {k: dlsg_amd.Trainer(net, lr=0.0, use_graphs=True) for k in forms}
    for k, fn in forms.items():
        for _ in range(2):
            fn(trainers[k])                              # captures
    legs = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            legs[k].append(round(timed(lambda: fn(trainers[k]), steps), 3))
            trainers[k].check()
    out = {k: spread(v) for k, v in legs.items()}
    print(json.dumps({'what': 'Trainer step as replayed graphs, MSVD shape, %d clips x %d captions (seq_per_clip), vocabulary 1000: the '
                              'minimum-risk form against the weighted CrossEntropy form' % (B, n), 'legs': out,
                      'risk_minus_weighted_ms': round(out['risk']['best_ms'] - out['weighted']['best_ms'], 3), 'steps': steps}))


def kernels_main(steps=20, B=64, n=5, rounds=3):
    ops = dlsg_amd.hip.HipOps()
    rows, L, per = B * n, 26, 50
    for V in (1000, 10000):
        g = torch.Generator().manual_seed(V)
        logits = (torch.randn(L, rows, V, generator=g) * 2).cuda()
        tg = torch.randint(0, V, (rows, L), generator=g).cuda()
        lens = torch.randint(6, 14, (rows,), generator=g).cuda()
        rewards = torch.rand(rows, generator=g, dtype=torch.float64).cuda()
        w = torch.randn(rows, generator=g).cuda()
        dl = torch.empty_like(logits)
        lse, tok, rl = (torch.empty(rows * L, device='cuda') for _ in range(3))
        f64 = dict(dtype=torch.float64, device='cuda')
        Q, s, R, stats = torch.empty(rows, **f64), torch.empty(rows, **f64), torch.empty(B, **f64), torch.empty(4, **f64)
        loss = torch.empty(1, device='cuda')
        legs = {'risk_rows': lambda: ops.risk_rows(logits, tg, lens, lse, tok, n, True),
                'risk_grad': lambda: ops.risk_grad(logits, tg, lens, lse, tok, rewards, None, dl, Q, s, R, loss, stats, n, True, 1.0, 1.0),
                'ce_ragged_weighted': lambda: ops.ce_ragged_weighted(logits, tg, lens, w, dl, rl, loss, True)}
        counted = int(lens.clamp(max=L).sum())
        row = 4 * V
        need = {'risk_rows': counted * row, 'risk_grad': counted * row + rows * L * row, 'ce_ragged_weighted': counted * row + rows * L * row}
        graphs = {}
        side = torch.cuda.Stream()
        for k, fn in legs.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()                                     # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(side)
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for _ in range(per):
                    fn()
        us = {k: [] for k in legs}
        for _ in range(rounds):
            for k in legs:
                us[k].append(round(event_ms(graphs[k].replay, steps) / per * 1e3, 2))
        best = {k: min(v) for k, v in us.items()}
        print(json.dumps({'what': 'loss launches alone on (26, %d, %d) logits, %d counted rows of %d, HIP events, %d launches per replay'
                                  % (rows, V, counted, rows * L, per), 'V': V, 'us': us, 'best_us': best,
                          'spread': {k: round((max(v) - min(v)) / min(v), 4) for k, v in us.items()},
                          'bytes': need, 'TB_per_s': {k: round(need[k] / best[k] * 1e-6, 3) for k in legs}}))


def mrt_main(steps=10, B=64, n=5, rounds=3):
    net, vocab, frames, regions, refs = setup(B)
    dc = dlsg_amd.DeviceCiderD(refs, vocab)
    vb = [str(b) for b in range(B)]
    trainers = {'scst': dlsg_amd.SCSTTrainer(net, dc, n_samples=n, use_graphs=True, lr=0.0),
                'mrt_swor': dlsg_amd.MRTTrainer(net, dc, n_candidates=n, candidates='swor', use_graphs=True, lr=0.0),
                'mrt_beam': dlsg_amd.MRTTrainer(net, dc, n_candidates=n, candidates='beam', candidate_options=dict(beam_size=n),
                                                use_graphs=True, lr=0.0)}
    for tr in trainers.values():
        for _ in range(2):
            out = tr.step(frames, regions, vb)           # captures
    legs = {k: [] for k in trainers}
    last = {}
    for _ in range(rounds):
        for k, tr in trainers.items():
            legs[k].append(round(timed(lambda: last.__setitem__(k, tr.step(frames, regions, vb)), steps), 3))
            tr.trainer.check()
    print(json.dumps({'what': 'whole steps with the device CIDEr-D reward as replayed graphs, MSVD shape, %d clips x %d rows, vocabulary '
                              '1000, rows expanded n-fold: SCSTTrainer against MRTTrainer on swor and beam lists' % (B, n),
                      'legs': {k: spread(v) for k, v in legs.items()},
                      'last_step': {k: {a: float(b) for a, b in v.items()} for k, v in last.items()}, 'steps': steps}))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else 'step'
    nums = [int(x) for x in sys.argv[1:] if x.isdigit()]
    {'step': step_main, 'kernels': kernels_main, 'mrt': mrt_main}[mode](*nums[:4])

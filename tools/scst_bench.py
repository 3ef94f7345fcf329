"""Self-critical training at the MSVD shape (batch 64, n = 5 samples per clip, vocabulary 1000, train mode), one JSON line:
  * `sample_graph_ms` -- a replay of SampleGraph (encoder on 320 rows + 26 sampled word steps) against `greedy_graph_ms`, a
    GreedyGraph replay on the same 320 rows (the clips repeated 5 times): the cost of sampling over argmax in the word loop;
  * `ciderd_ms` -- host ms of CiderD.scores for 320 hypotheses (a corpus of 64 clips x 20 references);
  * `scst_step_ms` -- one SCSTTrainer step (use_graphs), split into `sample_ms` (SampleGraph replay + copy of the words to the
    host), `reward_ms` (decode + CIDEr-D + advantages, host) and `train_ms` (the Trainer's weighted step on 320 rows).
  * `device_reward` -- the same with the reward on the GPU (`scoring.DeviceCiderD`, vocabulary 1000): `cider_kernel_ms` (HIP
    events around `dlsg_cider_d` on the 320 rows), `advantage_kernel_ms` (`dlsg_scst_advantage`), `scst_step_ms` and its split
    (`reward_ms`: the CIDEr-D and advantage launches, no host transfer), and the scores' largest difference to the host scorer.
  * `share` -- one more line: the device-reward step with the encoder run once per clip (`SCSTTrainer(share_encoder=True)`:
    shared sampling, `Trainer.step(seq_per_clip=n)`) against the unshared step, both timed in the same process in alternating
    rounds, each with its sample / reward / train split.
  * `filter` -- one more line: a SampleGraph replay with the sampling controls on (top_k 50, top_p 0.9, no_repeat_ngram 3,
    min_len 4: `dlsg_sample_filter_embed` in the word step) against the plain one, HIP events around the replays, alternating
    rounds in one process; and the two kernels alone on the same 320 rows of logits (vocabulary 1000 and 10 000), HIP events
    around 200 back-to-back launches each.
  * `mixed` -- one more line: `dlsg_caption_metrics` (BLEU-1..4 + ROUGE_L + the weighted mix) against `dlsg_cider_d` on the same
    320 sampled-like rows x 20 and x 40 references (vocabulary 10 000, a corpus of 300 clips; HIP events around back-to-back
    launches replayed from a hipGraph, alternating rounds), and the graph-replayed SCST step with the CIDEr-only device reward against the mixed reward
    {'cider': 1, 'bleu4': 2, 'rouge_l': 1} (`scoring.DeviceMixedReward`), alternating rounds in one process.
usage: python3 tools/scst_bench.py [steps=10] [batch=64] [n=5]
       python3 tools/scst_bench.py mixed [steps=20] [batch=64] [n=5] [rounds=2]
       python3 tools/scst_bench.py filter [steps=20] [batch=64] [n=5] [rounds=3]
       python3 tools/scst_bench.py share [steps=10] [batch=64] [n=5] [rounds=2]
       python3 tools/scst_bench.py kernels      (rocprofv3 --kernel-trace --stats target: eager greedy and sampled decodes)
       python3 tools/scst_bench.py reward-kernels   (rocprofv3 target: 20 launches each of dlsg_cider_d and dlsg_scst_advantage)"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import dlsg_amd  # noqa: E402
from dlsg_amd import scst as SC  # noqa: E402
from dlsg_amd.synth import synth_state_dict, synth_batch  # noqa: E402


def setup(B, V=1000):
    args = dlsg_amd.msvd_shaped()
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab)
    net.load_state_dict(synth_state_dict(net.state_dict(), 0))
    net = net.to('cuda').train()
    net.update_beam_size(1)
    frames, regions, _, _ = synth_batch(args, V, B, 1)
    rng = random.Random(0)
    words = [vocab.idx2word[i] for i in range(4, V)]
    refs = {str(b): [' '.join(rng.choice(words) for _ in range(rng.randint(5, 12))) for _ in range(20)] for b in range(B)}
    return net, vocab, frames.cuda(), regions.cuda(), refs


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def kernels(B=64, n=5):
    """eager greedy decode and eager sampled decode on B*n rows, 3 each: argmax_kernel and sample_embed_kernel side by side"""
    net, vocab, frames, regions, refs = setup(B)
    fx, rx = SC.expand_rows(frames, n), SC.expand_rows(regions, n)
    L = net.decoder.max_words
    with torch.no_grad():
        for k in range(3):
            net._engine_forward(fx, rx, None, L, [False] * L, True, 100 + k, {})
            net.sample(frames, regions, n=n, seed=200 + k)
    torch.cuda.synchronize()
    print('kernels: 3 greedy + 3 sampled decodes of %d rows' % (B * n))


def event_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reward_kernels(B=64, n=5):
    """the reward launches alone on B*n sampled rows: 20 x dlsg_cider_d, 20 x dlsg_scst_advantage"""
    net, vocab, frames, regions, refs = setup(B)
    dc = dlsg_amd.DeviceCiderD(refs, vocab)
    ids, _, lens = net.sample(frames, regions, n=n, seed=3)
    cidx = dc.index([str(b) for b in range(B) for _ in range(n)])
    adv = torch.empty(B * n, dtype=torch.float32, device='cuda')
    stats = torch.empty(3, dtype=torch.float64, device='cuda')
    for _ in range(20):
        r = dc.scores_device(ids, cidx)
        net.ops.scst_advantage(r, lens, None, n, adv, stats)
    torch.cuda.synchronize()
    print('reward kernels: 20 x %d rows' % (B * n))


def device_leg(net, vocab, frames, regions, refs, steps, B, n):
    dc = dlsg_amd.DeviceCiderD(refs, vocab)
    vids = [str(b) for b in range(B) for _ in range(n)]
    ids, _, lens = net.sample(frames, regions, n=n, seed=3)
    cidx = dc.index(vids)
    adv = torch.empty(B * n, dtype=torch.float32, device='cuda')
    stats = torch.empty(3, dtype=torch.float64, device='cuda')
    r = dc.scores_device(ids, cidx)
    kernel_ms = event_ms(lambda: dc.scores_device(ids, cidx))
    adv_ms = event_ms(lambda: net.ops.scst_advantage(r, lens, None, n, adv, stats))
    host = dc.cider.scores(vids, [net.decoder.decode_tokens(x) for x in ids.cpu()])
    err = float(np.abs(r.cpu().numpy() - host).max())

    tr = SC.SCSTTrainer(net, dc, n_samples=n, use_graphs=True)
    vb = [str(b) for b in range(B)]
    for _ in range(2):
        tr.step(frames, regions, vb)                   # captures
    step_ms = timed(lambda: tr.step(frames, regions, vb), steps)
    parts = {'sample': 0.0, 'reward': 0.0, 'train': 0.0}
    inner_sample, inner_step = tr._sample, tr.trainer.step
    inner_scores, inner_adv = dc.scores_device, net.ops.scst_advantage

    def clock(key, fn):
        def f(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            parts[key] += time.perf_counter() - t
            return out
        return f
    tr._sample = clock('sample', inner_sample)
    dc.scores_device = clock('reward', inner_scores)
    net.ops.scst_advantage = clock('reward', inner_adv)
    tr.trainer.step = clock('train', inner_step)
    for _ in range(steps):
        out = tr.step(frames, regions, vb)
    torch.cuda.synchronize()
    del net.ops.scst_advantage
    tr.trainer.check()
    return {'cider_kernel_ms': round(kernel_ms, 4), 'advantage_kernel_ms': round(adv_ms, 4), 'rows': B * n,
            'refs_per_clip': len(refs['0']), 'max_abs_diff_to_host': err, 'scst_step_ms': round(step_ms, 2),
            'parts_ms': {k: round(v / steps * 1e3, 2) for k, v in parts.items()},
            'last_step': {k: float(v) for k, v in out.items()}}


def step_leg(net, dc, frames, regions, steps, B, share):
    """ms per device-reward SCST step (graph replays), and its split measured on further steps with a synchronisation around
    each part"""
    n = share['n']
    tr = SC.SCSTTrainer(net, dc, n_samples=n, use_graphs=True, share_encoder=share['on'])
    vb = [str(b) for b in range(B)]
    for _ in range(2):
        tr.step(frames, regions, vb)                   # captures
    step_ms = timed(lambda: tr.step(frames, regions, vb), steps)
    parts = {'sample': 0.0, 'reward': 0.0, 'train': 0.0}
    inner_scores, inner_adv = dc.scores_device, net.ops.scst_advantage

    def clock(key, fn):
        def f(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            parts[key] += time.perf_counter() - t
            return out
        return f
    tr._sample = clock('sample', tr._sample)
    dc.scores_device = clock('reward', inner_scores)
    net.ops.scst_advantage = clock('reward', inner_adv)
    tr.trainer.step = clock('train', tr.trainer.step)
    try:
        for _ in range(steps):
            tr.step(frames, regions, vb)
        torch.cuda.synchronize()
    finally:
        del net.ops.scst_advantage
        del dc.scores_device
    tr.trainer.check()
    return {'scst_step_ms': round(step_ms, 2), 'parts_ms': {k: round(v / steps * 1e3, 2) for k, v in parts.items()}}


def share_main(steps=10, B=64, n=5, rounds=2):
    net, vocab, frames, regions, refs = setup(B)
    dc = dlsg_amd.DeviceCiderD(refs, vocab)
    legs = []
    for r in range(rounds):
        for on in (False, True):
            leg = step_leg(net, dc, frames, regions, steps, B, {'n': n, 'on': on})
            leg.update(round=r, share_encoder=on)
            legs.append(leg)
    best = {on: min(x['scst_step_ms'] for x in legs if x['share_encoder'] == on) for on in (False, True)}
    print(json.dumps({
        'what': 'SCST step with the device reward at the MSVD shape, batch %d x %d samples, vocabulary 1000, train mode, hipGraph '
                'replays: encoder on the %d repeated rows (share_encoder False) against once per clip (True)' % (B, n, B * n),
        'legs': legs, 'best_unshared_ms': best[False], 'best_shared_ms': best[True],
        'saved_ms': round(best[False] - best[True], 2), 'steps': steps}))


MIX = {'cider': 1.0, 'bleu4': 2.0, 'rouge_l': 1.0}


def metric_kernels(B, n, refs_per_clip, rounds, reps=3000):
    """HIP-event us per launch of dlsg_cider_d, of dlsg_caption_metrics (scores only) and of the mixed-reward launch, on B*n rows
    that are references of their clip with a fifth of the words replaced (a heavy-headed vocabulary of 10 000, 300 clips)"""
    vocab = dlsg_amd.make_vocab(10000)
    rng = random.Random(refs_per_clip)
    words = [vocab.idx2word[i] for i in range(4, len(vocab))]
    pick = lambda: words[min(int(rng.paretovariate(0.8)) - 1, len(words) - 1)]
    refs = {'v%03d' % c: [' '.join(pick() for _ in range(rng.randint(5, 12))) for _ in range(refs_per_clip)] for c in range(300)}
    mixed = dlsg_amd.DeviceMixedReward(refs, vocab, MIX)
    dc, dm = mixed.cider, mixed.metrics
    vids = [v for v in rng.sample(sorted(refs), B) for _ in range(n)]
    end, L = vocab('<end>'), 26
    rows = []
    for v in vids:
        ws = [rng.randrange(4, len(vocab)) if rng.random() < 0.2 else vocab(w) for w in rng.choice(refs[v]).split()]
        rows.append((ws + [end] + [rng.randrange(len(vocab)) for _ in range(L)])[:L])
    ids = torch.tensor(rows, dtype=torch.int64, device='cuda')
    cidx = dc.index(vids)
    base = dc.scores_device(ids, cidx)
    out5 = torch.empty(B * n, 5, dtype=torch.float64, device='cuda')
    rew = torch.empty(B * n, dtype=torch.float64, device='cuda')
    ops = dm._ops()
    legs = {'cider_d': lambda: ops.cider_d(ids, cidx, end, dc, base),
            'caption_metrics': lambda: ops.caption_metrics(ids, cidx, end, dm, scores=out5),
            'caption_metrics_reward': lambda: ops.caption_metrics(ids, cidx, end, dm, reward=rew, weights=mixed.w, base=base)}
    # a hipGraph of `per` launches per leg, so that the host's launch rate is not what the events see
    per, graphs = 200, {}
    side = torch.cuda.Stream()
    for k, fn in legs.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                       # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(per):
                fn()
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for k in legs:
            us[k].append(round(event_ms(graphs[k].replay, reps // per) / per * 1e3, 2))
    hyps = [' '.join(vocab.idx2word[t] for t in r[:r.index(end)]) for r in rows]
    err = float(np.abs(rew.cpu().numpy() - mixed.scores(vids, hyps)).max())
    return {'rows': B * n, 'refs_per_clip': refs_per_clip, 'launches_per_leg': reps, 'us': us, 'best_us': {k: min(v) for k, v in us.items()},
            'max_abs_diff_to_host_reward': err}


def mixed_main(steps=20, B=64, n=5, rounds=2):
    kern = [metric_kernels(B, n, q, rounds) for q in (20, 40)]
    net, vocab, frames, regions, refs = setup(B)
    rewards = {'cider_only': dlsg_amd.DeviceCiderD(refs, vocab), 'mixed': dlsg_amd.DeviceMixedReward(refs, vocab, MIX)}
    vb = [str(b) for b in range(B)]
    trainers = {}
    for k, rw in rewards.items():
        trainers[k] = SC.SCSTTrainer(net, rw, n_samples=n, use_graphs=True)
        for _ in range(2):
            trainers[k].step(frames, regions, vb)      # captures
    legs = {k: [] for k in trainers}
    for _ in range(rounds):
        for k, tr in trainers.items():
            legs[k].append(round(timed(lambda: tr.step(frames, regions, vb), steps), 3))
            tr.trainer.check()
    best = {k: min(v) for k, v in legs.items()}
    print(json.dumps({
        'what': 'caption-metric kernels against dlsg_cider_d (HIP events, back-to-back launches in a hipGraph) and the graph-replayed SCST step at '
                'the MSVD shape, batch %d x %d samples, vocabulary 1000, with the CIDEr-only device reward against %s' % (B, n, MIX),
        'kernels': kern, 'step_legs_ms': legs, 'best_cider_only_ms': best['cider_only'], 'best_mixed_ms': best['mixed'],
        'mixed_minus_cider_only_ms': round(best['mixed'] - best['cider_only'], 3), 'steps': steps}))


FILTER_OPTS = dict(top_k=50, top_p=0.9, no_repeat_ngram=3, min_len=4)


def filter_main(steps=20, B=64, n=5, rounds=3):
    from dlsg_amd import engine as E
    net, vocab, frames, regions, refs = setup(B)
    graphs = {'plain': dlsg_amd.SampleGraph(net, frames, regions, n=n),
              'filtered': dlsg_amd.SampleGraph(net, frames, regions, n=n, **FILTER_OPTS)}
    seeds = iter(range(1, 10 ** 6))
    legs = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            legs[k].append(round(event_ms(lambda: g(frames, regions, next(seeds)), steps), 3))
    lens = graphs['filtered'](frames, regions, 3)[2].double().mean().item()
    lens0 = graphs['plain'](frames, regions, 3)[2].double().mean().item()
    # the two kernels alone: 320 rows at word step 6, histories of random words
    rows, L, W = B * n, net.decoder.max_words, net.decoder.word_embed.weight.shape[1]
    kern = {}
    for V in (1000, 10000):
        g = torch.Generator().manual_seed(V)
        x = (torch.randn(rows, V, generator=g) * 3).cuda()
        Em = torch.randn(V, W, generator=g).cuda()
        hist = torch.randint(4, 40, (L, rows), generator=g).cuda()
        ids, out = torch.empty(rows, dtype=torch.int64, device='cuda'), torch.empty(rows, W, device='cuda')
        logp, ln = torch.empty(rows, device='cuda'), torch.full((rows,), L, dtype=torch.int64, device='cuda')
        kept = torch.empty(rows, dtype=torch.int32, device='cuda')
        common = dict(temperature=1.0, p=0.5, seed=5, site=E.SITE_WORD, site_sample=E.SITE_SAMPLE, row0=rows)

        def filt(**o):
            return lambda: net.ops.sample_filter_embed(x, Em, ids, out, logp, ln, 6, 2, hist=hist, kept=kept, **common, **o)
        kern[V] = {'sample_embed_us': round(event_ms(lambda: net.ops.sample_embed(x, Em, ids, out, logp, ln, 6, 2, **common), 200) * 1e3, 2),
                   'filter_all_on_us': round(event_ms(filt(**FILTER_OPTS), 200) * 1e3, 2),
                   'filter_bans_only_us': round(event_ms(filt(no_repeat_ngram=3, min_len=4), 200) * 1e3, 2),
                   'filter_top_k_only_us': round(event_ms(filt(top_k=50), 200) * 1e3, 2),
                   'filter_top_p_only_us': round(event_ms(filt(top_p=0.9), 200) * 1e3, 2)}
    best = {k: min(v) for k, v in legs.items()}
    print(json.dumps({
        'what': 'SampleGraph replay at the MSVD shape, batch %d x %d samples, vocabulary 1000, train mode: plain sampling against '
                '%s; HIP events, %d replays per leg, alternating' % (B, n, FILTER_OPTS, steps),
        'legs_ms': legs, 'best_plain_ms': best['plain'], 'best_filtered_ms': best['filtered'],
        'filtered_over_plain': round(best['filtered'] / best['plain'], 4), 'mean_len_plain': lens0, 'mean_len_filtered': lens,
        'kernels_320_rows': kern}))


def main(steps=10, B=64, n=5):
    net, vocab, frames, regions, refs = setup(B)
    rows = B * n
    fx, rx = SC.expand_rows(frames, n).contiguous(), SC.expand_rows(regions, n).contiguous()
    sg = dlsg_amd.SampleGraph(net, frames, regions, n=n)
    net.eval()
    gg = dlsg_amd.GreedyGraph(net, fx, rx)
    net.train()
    seeds = iter(range(1, 10 ** 6))
    sample_ms = timed(lambda: sg(frames, regions, next(seeds)), steps)
    greedy_ms = timed(lambda: gg(fx, rx), steps)
    del gg, sg
    reward = dlsg_amd.CiderD(refs)
    ids = net.sample(frames, regions, n=n, seed=3)[0].cpu()
    hyps = [net.decoder.decode_tokens(x) for x in ids]
    vids = [str(b) for b in range(B) for _ in range(n)]
    t0 = time.perf_counter()
    for _ in range(3):
        reward.scores(vids, hyps)
    cider_ms = (time.perf_counter() - t0) / 3 * 1e3

    tr = SC.SCSTTrainer(net, reward, n_samples=n, use_graphs=True)
    parts = {'sample': 0.0, 'reward': 0.0, 'train': 0.0}
    inner_sample, inner_scores, inner_step = tr._sample, reward.scores, tr.trainer.step

    def clock(key, fn, sync):
        def f(*a, **k):
            if sync:
                torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            if sync:
                torch.cuda.synchronize()
            parts[key] += time.perf_counter() - t
            return out
        return f
    vb = [str(b) for b in range(B)]
    for _ in range(2):
        tr.step(frames, regions, vb)                   # captures
    step_ms = timed(lambda: tr.step(frames, regions, vb), steps)
    tr._sample = clock('sample', inner_sample, True)
    reward.scores = clock('reward', inner_scores, False)
    tr.trainer.step = clock('train', inner_step, True)
    for _ in range(steps):
        out = tr.step(frames, regions, vb)
    torch.cuda.synchronize()
    tr.trainer.check()
    dev = device_leg(net, vocab, frames, regions, refs, steps, B, n)
    print(json.dumps({
        'what': 'SCST at the MSVD shape: batch %d x %d samples = %d rows, vocabulary 1000, train mode, hipGraph replays' % (B, n, rows),
        'sample_graph_ms': round(sample_ms, 3), 'greedy_graph_ms': round(greedy_ms, 3),
        'sample_over_greedy': round(sample_ms / greedy_ms, 3),
        'ciderd_ms': round(cider_ms, 2), 'ciderd_hyps': rows,
        'scst_step_ms': round(step_ms, 2),
        'parts_ms': {k: round(v / steps * 1e3, 2) for k, v in parts.items()},
        'parts_note': 'separate steps with a device synchronisation around sample and train: they add up to more than scst_step_ms',
        'last_step': {k: (float(v) if k == 'loss' else v) for k, v in out.items()},
        'device_reward': dev,
        'steps': steps}))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'kernels':
        kernels()
    elif len(sys.argv) > 1 and sys.argv[1] == 'reward-kernels':
        reward_kernels()
    elif len(sys.argv) > 1 and sys.argv[1] == 'filter':
        filter_main(*[int(x) for x in sys.argv[2:6]])
    elif len(sys.argv) > 1 and sys.argv[1] == 'mixed':
        mixed_main(*[int(x) for x in sys.argv[2:6]])
    elif len(sys.argv) > 1 and sys.argv[1] == 'share':
        share_main(*[int(x) for x in sys.argv[2:6]])
    else:
        main(*[int(x) for x in sys.argv[1:4]])

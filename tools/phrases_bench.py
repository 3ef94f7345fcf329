"""Constrained beam search with phrases beside the word search, at batch 128, beam 5, MSVD-shaped, vocabulary 1000,
no_repeat_ngram = 0, min_len = 4, length_penalty 0.7, as replayed hipGraphs, one JSON line per call:
  * `words3`     -- `ConstrainedBeamGraph` with three one-word constraints per clip as a (B, 3, 1) tensor (`beam_select_cons`);
  * `phrases3x1` -- the same words as a (B, 3, 1, 1) phrase tensor (`beam_select_phrases`, P = 1);
  * `phrases3x3` -- three 3-word phrases per clip (random words).
The graphs are timed in alternating rounds (the order rotates) after a warm-up replay each; ms per batch including the device
synchronisation; median, min, max and every round.  Per graph also `all_met`, the share of clips whose row 0 meets every
constraint.  `--tree DIR` imports the package of another checkout (built there): a tree without `pack_phrases` measures `words3`
alone, so the same script run on the parent commit and on this tree, turn by turn, says whether the word path moved.  `steps`
runs the three searches eagerly, twice each: the target of `rocprofv3 --kernel-trace --stats`.  The model's weights are synthetic.
usage: python3 tools/phrases_bench.py [--tree DIR] [--rounds 3] [--reps 5] [steps]"""
import argparse
import json
import os
import statistics
import sys
import time

OPTS = dict(beam_size=5, length_penalty=0.7, no_repeat_ngram=0, min_len=4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='?', default='graphs', choices=('graphs', 'steps'))
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, 'd-lsg-video-caption_amd')]
    import torch
    import dlsg_amd
    from dlsg_amd.synth import synth_batch, synth_state_dict
    assert os.path.abspath(dlsg_amd.__file__).startswith(tree), dlsg_amd.__file__
    B, V = 128, 1000
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(dlsg_amd.msvd_shaped(), vocab)
    net.load_state_dict(synth_state_dict(net.state_dict(), 0))
    net = net.to('cuda').eval()
    frames, regions, _, _ = synth_batch(dlsg_amd.msvd_shaped(), V, B, 1)
    frames, regions = frames.cuda(), regions.cuda()
    gen = torch.Generator().manual_seed(3)
    words = torch.randint(4, V, (B, 3, 1), generator=gen)
    cons = {'words3': words.cuda()}
    if hasattr(dlsg_amd, 'pack_phrases'):
        cons['phrases3x1'] = words.unsqueeze(3).cuda()
        cons['phrases3x3'] = torch.randint(4, V, (B, 3, 1, 3), generator=gen).cuda()
    if a.mode == 'steps':
        for name, c in cons.items():
            for _ in range(2):
                net.constrained_beam_search(frames, regions, c, **OPTS)
        torch.cuda.synchronize()
        net.ops.check_persistent()
        return
    graphs = [(name, dlsg_amd.ConstrainedBeamGraph(net, frames, regions, c, return_met=True, **OPTS)) for name, c in cons.items()]
    for name, g in graphs:                                     # first replays outside the timing
        g(g.frames, g.regions, g.cons)
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in graphs}
    for r in range(a.rounds):
        for i in range(len(graphs)):
            name, g = graphs[(i + r) % len(graphs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                g(g.frames, g.regions, g.cons)
                torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.reps * 1e3)
    out = {'tree': tree, 'what': 'ConstrainedBeamGraph replays: batch %d, beam 5, MSVD-shaped, vocabulary %d, %d alternating rounds of %d '
                                 'replays, ms per batch; synthetic model' % (B, V, a.rounds, a.reps)}
    for name, g in graphs:
        met = g(g.frames, g.regions, g.cons)[3]
        out[name] = {'median': round(statistics.median(ms[name]), 3), 'min': round(min(ms[name]), 3), 'max': round(max(ms[name]), 3),
                     'rounds_ms': [round(x, 3) for x in ms[name]], 'all_met': round(float((met[:, 0] == 3).double().mean()), 4)}
    net.ops.check_persistent()
    print(json.dumps(out))


if __name__ == '__main__':
    main()

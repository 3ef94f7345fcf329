"""Records tests/golden/beam_step_bits.npz: the outputs of the four beam-search step kernels (dlsg_beam_select, _hist, _ens,
_groups) on seeded step cases, as computed on an MI355X by the commit BEFORE the kernels were rebuilt from shared phases
(csrc/beam.hpp).  tests/test_gpu_beam_step_bits.py runs the same launches on the tree and compares every bit, so the fixture is
recorded once from that parent build and never from the tree under test: check the parent out into a scratch worktree, `make` its
csrc/, and run this file under one `timeout` with that worktree's d-lsg-video-caption_amd on PYTHONPATH (the builders below come
from this tree's tests/, the kernels and `HipOps` from the parent).

The inputs come from the builders of the step tests (step_case, member_logits), so only outputs are stored: per kernel and
output one array, the launches' results concatenated in the order of `launches()`; new_lp as its int32 bit pattern."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.append(p)

from test_gpu_beam_nbest import END, step_case, steps_of          # noqa: E402
from test_gpu_ensemble import member_logits                       # noqa: E402

FIXTURE = os.path.join(HERE, 'beam_step_bits.npz')
# (B, k, V), L: every K of the kernels' dispatch, V below a wave and V no multiple of 64, the longest history at the largest K
SHAPES = [((2, 1, 40), 26), ((2, 2, 64), 26), ((3, 3, 50), 26), ((2, 4, 70), 26), ((7, 5, 1000), 26), ((2, 6, 97), 26),
          ((2, 7, 130), 26), ((4, 8, 10007), 26), ((4, 8, 10007), 64)]
WEIGHTS = {1: [1.0], 3: [0.2, 0.5, 0.3]}
PENALTIES = (0.5, float('inf'))
KERNELS = ('select', 'hist', 'ens', 'groups')
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'cnt', 'hout')


def step_keys():
    """(dims, L, g, t, min_len) of every step case.  The 63-token history rows of L = 64 are most of the fixture's size, so of
    that shape's steps only the ones with the n-gram ban stay, and its last step only with the min_len a search can ask for (< L);
    that and three (members, mode) settings for the group kernel keep the file under its 256 KB"""
    keys = [(dims, L, g, t, m) for dims, L in SHAPES for g in (0, 3) for t in steps_of(L, g) for m in (0, t + 1)]
    return [key for key in keys if key[1] == 26 or (key[2] == 3 and key[4] < key[1])]


def launches(key):
    """(kernel, options) of every launch on one step case, in the order the fixture stores them"""
    (B, k, V), L, g, t, m = key
    out = [('select', ())] if m == 0 else []                       # (no bans: the case's min_len does not reach it)
    out.append(('hist', ()))
    out += [('ens', (M, mode)) for M in WEIGHTS for mode in (0, 1)]
    out += [('groups', (M, mode, G, pen)) for M, mode in ((1, 0), (3, 0), (3, 1)) for G in range(2, k + 1) if k % G == 0
            for pen in PENALTIES]
    return out


def run_launch(ops, kernel, opt, key, c, lgs):
    """one launch on fresh output arrays -> {output: CPU tensor}; `c` the case on the device, `lgs` the three members' logits"""
    (B, k, V), L, g, t, m = key
    o = {n: torch.zeros_like(c[n]) for n in OUTPUTS}
    outs = (o['pred'], o['nlp'], o['back'], o['rows'])
    if kernel == 'select':
        ops.beam_select(c['lg'][:, 1:V + 1], c['last'], c['lp'], *outs, k, END, first=t == 0, ended_count=o['cnt'])
    elif kernel == 'hist':
        ops.beam_select_hist(c['lg'][:, 1:V + 1], c['last'], c['lp'], *outs, k, END, c['hist'], o['hout'], t, g, m, ended_count=o['cnt'])
    else:
        M, mode = opt[:2]
        xs = [x[:, 1:V + 1] for x in lgs[:M]]
        if kernel == 'ens':
            ops.beam_select_ens(xs, WEIGHTS[M], mode, c['last'], c['lp'], *outs, k, END, c['hist'], o['hout'], t, g, m,
                                ended_count=o['cnt'])
        else:
            ops.beam_select_groups(xs, WEIGHTS[M], mode, c['last'], c['lp'], *outs, k, END, c['hist'], o['hout'], t, g, m, opt[2],
                                   opt[3], ended_count=o['cnt'])
    if kernel == 'select':
        del o['hout']
    return {n: v.cpu() for n, v in o.items()}


def run_all(ops, device='cuda'):
    """every launch of every step case -> {kernel: [(label, {output: CPU tensor})]}"""
    res = {kn: [] for kn in KERNELS}
    for key in step_keys():
        dims, L, g, t, m = key
        c = {n: v.to(device) for n, v in step_case(dims, L, t, g, 100 * g + t).items()}
        lgs = [x.to(device) for x in member_logits(key, 3)]
        for kernel, opt in launches(key):
            res[kernel].append(('%s%r dims=%r L=%d g=%d t=%d min_len=%d' % (kernel, opt, dims, L, g, t, m),
                                run_launch(ops, kernel, opt, key, c, lgs)))
    return res


def as_stored(name, x):
    """the array of one output as the fixture keeps it: float32 as its bits, so that -inf and NaN compare as well"""
    x = x.contiguous().view(-1)
    return (x.view(torch.int32) if x.dtype == torch.float32 else x).numpy()


def main():
    from dlsg_amd.hip import HipOps
    import dlsg_amd
    print('recording with', os.path.dirname(dlsg_amd.__file__))
    res = run_all(HipOps())
    arrays = {}
    for kn, runs in res.items():
        for n in runs[0][1]:
            arrays['%s_%s' % (kn, n)] = np.concatenate([as_stored(n, o[n]) for _, o in runs])
        print(kn, len(runs), 'launches')
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, **arrays)


if __name__ == '__main__':
    main()

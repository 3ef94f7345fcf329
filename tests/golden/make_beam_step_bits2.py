"""Records tests/golden/beam_step_bits2.npz: the outputs of the two later beam-search step kernels (dlsg_beam_select_gumbel, _cons)
on seeded step cases, as computed on an MI355X by the commit BEFORE their searches, wrappers and phases were folded into the
shared ones.  It is the sibling of make_beam_step_bits.py (whose fixture stays as it was recorded) and is used the same way:
tests/test_gpu_beam_step_bits.py runs the same launches on the tree and compares every bit, so the fixture is recorded once from
that parent build and never from the tree under test -- check the parent out into a scratch worktree, `make` its csrc/, and run
this file under one `timeout` with that worktree's d-lsg-video-caption_amd on PYTHONPATH.

The shapes and the step keys are make_beam_step_bits.py's; the inputs come from the builders of the two kernels' step tests
(`build_case` of tests/test_sbs_host.py, `build_cons_case` of tests/test_constrained_host.py, seeded 100 g + t), so only outputs
are stored: per kernel and output one array, the launches' results concatenated in the order of `launches()`; new_lp as its
int32 bit pattern, G_out (float64) as its int64 bit pattern."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.append(p)

from make_beam_step_bits import SHAPES, step_keys                  # noqa: E402,F401
from test_constrained_host import CW, build_cons_case, run_cons    # noqa: E402
from test_sbs_host import STEP_SEED, TEMPERATURES, build_case, run_gumbel      # noqa: E402

FIXTURE = os.path.join(HERE, 'beam_step_bits2.npz')
KERNELS = ('gumbel', 'cons')
OUTPUTS = {'gumbel': ('pred', 'nlp', 'back', 'rows', 'cnt', 'hout', 'gout'), 'cons': ('pred', 'nlp', 'back', 'rows', 'cnt', 'hout', 'met')}
SEED_FORMS = ('int', 'word')                                       # the seed as a Python int and as a device word


def launches(key):
    """(kernel, options) of every launch on one step case, in the order the fixture stores them"""
    return [('gumbel', (temp, form)) for temp in TEMPERATURES for form in SEED_FORMS] + [('cons', cw) for cw in CW]


def run_launch(ops, kernel, opt, key, device):
    """one launch on a freshly built case -> {output: CPU tensor}"""
    dims, L, g, t, m = key
    if kernel == 'gumbel':
        c = {n: v.to(device) for n, v in build_case(dims, L, t, g, 100 * g + t).items()}
        seed = STEP_SEED if opt[1] == 'int' else torch.tensor([STEP_SEED], dtype=torch.int64, device=device)
        run_gumbel(ops, c, (dims, L, g, t, m, opt[0]), seed=seed)
    else:
        c = {n: v.to(device) for n, v in build_cons_case(dims, L, t, g, opt, 100 * g + t).items()}
        c['met'].fill_(7)                                          # (the launch writes every row's count)
        run_cons(ops, c, (dims, L, g, t, m, opt))
    return {n: c[n].cpu() for n in OUTPUTS[kernel]}


def run_all(ops, device='cuda'):
    """every launch of every step case -> {kernel: [(label, {output: CPU tensor})]}"""
    res = {kn: [] for kn in KERNELS}
    for key in step_keys():
        dims, L, g, t, m = key
        for kernel, opt in launches(key):
            res[kernel].append(('%s%r dims=%r L=%d g=%d t=%d min_len=%d' % (kernel, opt, dims, L, g, t, m),
                                run_launch(ops, kernel, opt, key, device)))
    return res


def as_stored(name, x):
    """the array of one output as the fixture keeps it: floating point as its bits, so that -inf and NaN compare as well"""
    x = x.contiguous().view(-1)
    return (x.view({torch.float32: torch.int32, torch.float64: torch.int64}[x.dtype]) if x.is_floating_point() else x).numpy()


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

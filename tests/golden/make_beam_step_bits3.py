"""Records tests/golden/beam_step_bits3.npz: the outputs of the two beam-search step kernels under exclusions
(dlsg_beam_select_excl, dlsg_beam_select_gumbel_excl) on seeded step cases, as computed on an MI355X by the commit BEFORE the fold
of the two kernels into their parents as a template axis was tried (built, passed this fixture, missed its
speed condition and was left out, so the kernels are still that commit's text; the fixture is what the next attempt needs).  It is
the sibling of make_beam_step_bits2.py (whose fixture stays as it was recorded) and is used the same way:
tests/test_gpu_beam_step_bits.py runs the same launches on the tree and compares every bit, so the fixture is recorded once from
that parent build and never from the tree under test -- check the parent out into a scratch worktree, `make` its csrc/, and run
this file under one `timeout` with that worktree's d-lsg-video-caption_amd on PYTHONPATH.

The shapes and the step keys are make_beam_step_bits.py's; every key runs under the four kinds of table of
tests/test_excl_host.py (`build_tables`: none, lists below the bucketing threshold, P = 4 with cut entries and a bad ending, the 96
entries of the bucketed list).  The inputs come from the builders of the two kernels' step tests, seeded 100 g + t:
`build_excl_case` with the members (M, mode) taken in turn from `MEMBERS`, and `build_case` of tests/test_sbs_host.py at temperature
0.7 with the seed as a Python int and as a device word.  So only outputs are stored: per kernel and output one array, the
launches' results concatenated in the order of `launches()`; new_lp as its int32 bit pattern, G_out (float64) as its int64 bit
pattern."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.append(p)

from make_beam_step_bits import SHAPES, step_keys                  # noqa: E402,F401
from make_beam_step_bits2 import SEED_FORMS, as_stored             # noqa: E402,F401
from dlsg_amd.engine import SITE_SAMPLE                            # noqa: E402
from test_excl_host import MEMBERS, TABLES, build_excl_case, build_tables, run_excl      # noqa: E402
from test_sbs_host import END, STEP_SEED, build_case               # noqa: E402

FIXTURE = os.path.join(HERE, 'beam_step_bits3.npz')
KERNELS = ('excl', 'gumbel_excl')
OUTPUTS = {'excl': ('pred', 'nlp', 'back', 'rows', 'cnt', 'hout'), 'gumbel_excl': ('pred', 'nlp', 'back', 'rows', 'cnt', 'hout', 'gout')}
TEMPERATURE = 0.7


def launches(key):
    """(kernel, options) of every launch on one step case, in the order the fixture stores them: the members of the `excl`
    launches go round MEMBERS over all the keys"""
    at = step_keys().index(key) * len(TABLES)
    return [('excl', (tab,) + MEMBERS[(at + i) % len(MEMBERS)]) for i, tab in enumerate(TABLES)] + \
           [('gumbel_excl', (tab, form)) for tab in TABLES for form in SEED_FORMS]


def on(device, x):
    return None if x is None else x.to(device)


def run_launch(ops, kernel, opt, key, device):
    """one launch on a freshly built case -> {output: CPU tensor}"""
    dims, L, g, t, m = key
    V = dims[2]
    if kernel == 'excl':
        full = key + opt
        c, lgs, shared, per_clip = build_excl_case(full, 100 * g + t)
        c = {n: v.to(device) for n, v in c.items()}
        run_excl(ops, c, [x.to(device) for x in lgs], on(device, shared), on(device, per_clip), full)
    else:
        c = build_case(dims, L, t, g, 100 * g + t)
        shared, per_clip = build_tables(c, dims, t, opt[0], torch.Generator().manual_seed(100 * g + t + 55))
        c = {n: v.to(device) for n, v in c.items()}
        seed = STEP_SEED if opt[1] == 'int' else torch.tensor([STEP_SEED], dtype=torch.int64, device=device)
        ops.beam_select_gumbel_excl(c['lg'][:, 1:V + 1], c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'], dims[1], END,
                                    c['hist'], c['hout'], t, c['gin'], c['gout'], on(device, shared), on(device, per_clip),
                                    temperature=TEMPERATURE, seed=seed, site_sample=SITE_SAMPLE, no_repeat_ngram=g, min_len=m,
                                    ended_count=c['cnt'])
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

"""GPU (-m gpu): the two instantiations of dec_mid_fwd / dec_mid_bwd -- loads requested where they are used (sched=1) and
every independent load requested up front into registers (sched=2) -- run the same arithmetic in the same order, so every
output buffer is bit-identical (torch.equal) on identical inputs.  Shapes cover the vector and the scalar path, the last slots
of the register arrays (widths of 2048, 72 attended rows), more attended rows than the registers hold, and the K' / V' block
index of beam search."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, Q, H, D, P, ns)
CASES = {
    'a': (3, 48, 32, 40, 5, 2),             # vector path; P is not a multiple of 4
    'b': (2, 50, 34, 38, 3, 1),             # widths not multiples of 4: the V = 1 instantiations; one stream
    'c': (2, 2048, 2048, 2048, 72, 2),      # the widest row and the most attended rows the kernels take
    'd': (2, 600, 520, 300, 32, 2),         # more attended rows than are held in registers, widths not multiples of 1024
    'e': (6, 96, 64, 80, 4, 2),             # forward: three consecutive rows share a K' / V' block (kv_div=3)
}


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def run_both(build, run, outs, scheds=(1, 2)):
    """build(gen) -> dict of CPU tensors; run(t, sched) launches on dict t; every tensor named in outs must come out equal."""
    base = build(torch.Generator().manual_seed(1234))
    res = []
    for sched in scheds:
        t = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in base.items()}
        run(t, sched)
        torch.cuda.synchronize()
        res.append(t)
    for o in outs:
        assert torch.isfinite(res[0][o]).all(), (o, 'non-finite')
        assert torch.equal(res[0][o], res[1][o]), (o, (res[0][o] - res[1][o]).abs().max().item())


def fwd_case(hip, dims, nslab, with_cprev, drop, kv_div=1, scheds=(1, 2)):
    B, Q, H, D, P, ns = dims
    Bk = B // kv_div

    def build(g):
        d = dict(slabs=rnd(g, nslab, B, 4 * Q), add=rnd(g, B, 2, 4 * Q), bi=rnd(g, 4 * Q), bh=rnd(g, 4 * Q), cp=rnd(g, B, Q),
                 c=torch.zeros(B, Q), h=torch.zeros(B, Q), gates=torch.zeros(B, 4 * Q), gq=rnd(g, Q), bq=rnd(g, Q),
                 qcur=torch.zeros(B, Q), stq=torch.zeros(B, 2), alpha=torch.zeros(B, ns * P))
        for s in range(ns):
            d['K%d' % s] = rnd(g, Bk, P, Q, scale=0.2); d['V%d' % s] = rnd(g, Bk, P, H)
            d['g%d' % s] = rnd(g, H); d['b%d' % s] = rnd(g, H)
            d['cpre%d' % s] = torch.zeros(B, H); d['ctx%d' % s] = torch.zeros(B, H); d['stc%d' % s] = torch.zeros(B, 2)
        return d

    def run(t, sched):
        R = range(ns)
        hip.dec_mid_fwd(t['slabs'], t['add'][:, 1], t['bi'], t['bh'], t['cp'] if with_cprev else None, t['c'], t['h'], t['gates'],
                        (t['gq'], t['bq']), t['qcur'], t['stq'], 0.3 if drop else 0.0, 11, [t['K%d' % s] for s in R],
                        [t['V%d' % s] for s in R], [(t['g%d' % s], t['b%d' % s]) for s in R], [t['cpre%d' % s] for s in R],
                        [t['ctx%d' % s] for s in R], [t['stc%d' % s] for s in R], t['alpha'],
                        [0.2 if drop else 0.0, 0.4 if drop else 0.0][:ns], [21, 22][:ns], 0.3, seed=5, kv_div=kv_div, sched=sched)
    outs = ['c', 'h', 'gates', 'qcur', 'stq', 'alpha'] + [k % s for s in range(ns) for k in ('cpre%d', 'ctx%d', 'stc%d')]
    run_both(build, run, outs, scheds)


# gate slabs (1, 3 and 7: a remainder alone, the query gates' three, a full group of four and a remainder), with and without
# c_prev, dropout off and on
FWD_VARIANTS = [(3, True, True), (1, False, False), (7, True, True)]


@pytest.mark.parametrize('variant', FWD_VARIANTS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_dec_mid_fwd_early_loads_are_bit_identical(hip, case, variant):
    nslab, with_cprev, drop = variant
    fwd_case(hip, CASES[case], nslab, with_cprev, drop, kv_div=3 if case == 'e' else 1)


def bwd_case(hip, dims, S, nrec, with_dalpha, drop, scheds=(1, 2)):
    """nrec = 0: the last word step (no recurrent inputs, dlh_rec not written)."""
    B, Q, H, D, P, ns = dims
    last = nrec == 0

    def build(g):
        d = dict(slabs=rnd(g, S, B, ns * H + Q + D), rec=rnd(g, max(nrec, 1), B, Q + D), dlh=torch.zeros(B, D),
                 alpha=torch.softmax(rnd(g, B, ns, P), 2).reshape(B, ns * P), dalpha=rnd(g, B, ns * P), ds=torch.zeros(B, ns * P),
                 qh=rnd(g, B, Q), gq=rnd(g, Q), partq=torch.zeros(B, 2, Q), gates=torch.sigmoid(rnd(g, B, 4 * Q)), c=rnd(g, B, Q),
                 cp=rnd(g, B, Q), dc=rnd(g, B, Q), dg=torch.zeros(B, 4 * Q))
        qh = d['qh']
        d['stq'] = torch.cat([qh.mean(1, keepdim=True), 1 / torch.sqrt(qh.var(1, unbiased=False, keepdim=True) + 1e-5)], 1)
        for s in range(ns):
            d['K%d' % s] = rnd(g, B, P, Q, scale=0.2); d['V%d' % s] = rnd(g, B, P, H)
            d['g%d' % s] = rnd(g, H); d['cpre%d' % s] = rnd(g, B, H)
            y = torch.tanh(d['cpre%d' % s])
            d['stc%d' % s] = torch.cat([y.mean(1, keepdim=True), 1 / torch.sqrt(y.var(1, unbiased=False, keepdim=True) + 1e-5)], 1)
            d['partc%d' % s] = torch.zeros(B, 2, H); d['dcpre%d' % s] = torch.zeros(B, H)
        return d

    def run(t, sched):
        R = range(ns)
        hip.dec_mid_bwd(t['slabs'], None if last else t['dlh'], [t['cpre%d' % s] for s in R], [t['stc%d' % s] for s in R],
                        [t['g%d' % s] for s in R], [t['partc%d' % s] for s in R], [t['dcpre%d' % s] for s in R],
                        [0.2 if drop else 0.0, 0.4 if drop else 0.0][:ns], [21, 22][:ns], [t['K%d' % s] for s in R],
                        [t['V%d' % s] for s in R], t['alpha'], t['dalpha'] if with_dalpha else None, t['ds'], t['qh'], t['stq'],
                        t['gq'], t['partq'], 0.3 if drop else 0.0, 11, None if last else t['rec'][:, :, :Q], t['gates'], t['c'],
                        t['cp'], t['dc'], t['dg'], 0.3, seed=5, sched=sched)
    outs = ['ds', 'partq', 'dg', 'dc'] + ([] if last else ['dlh']) + [k % s for s in range(ns) for k in ('dcpre%d', 'partc%d')]
    run_both(build, run, outs, scheds)


# (input-gradient slabs, recurrent slabs, dalpha given, dropout on): the last step and two inner steps
BWD_VARIANTS = [(3, 0, True, True), (5, 3, False, True), (6, 5, True, False)]


@pytest.mark.parametrize('variant', BWD_VARIANTS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_dec_mid_bwd_early_loads_are_bit_identical(hip, case, variant):
    bwd_case(hip, CASES[case], *variant)


def test_the_library_takes_the_early_loads_when_rows_fit_the_cus(hip):
    """sched=0 at 3 rows (fewer than any device's CUs) is the early-load kernel: equal to sched=2, forward and backward."""
    fwd_case(hip, CASES['a'], 3, True, True, scheds=(0, 2))
    bwd_case(hip, CASES['a'], 5, 3, True, True, scheds=(0, 2))


def test_an_unknown_sched_is_refused(hip):
    with pytest.raises(RuntimeError):
        fwd_case(hip, CASES['a'], 3, True, True, scheds=(3, 3))
    with pytest.raises(RuntimeError):
        bwd_case(hip, CASES['a'], 5, 3, True, True, scheds=(3, 3))

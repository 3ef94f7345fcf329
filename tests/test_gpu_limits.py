"""GPU (-m gpu): the limits of the fused kernels.  The engine picks a fused kernel or the composed path (gemm + softmax + gemm
+ rowln) from the predicates HipOps.*_supported (dlsg_amd/limits.py); the launchers in csrc/ hold their own copy of the same
limits.  On a grid around every limit: the launcher's status equals the predicate, a refused call launched nothing (every
output still NaN), an accepted call matches a float64 restatement written here (dropout off).  Then the grouped launches
(rowln, LatentPSL `_multi`) with two items that differ wherever their launcher allows: bit-equal to the single launches, the
single launches against float64, and their refusals.

Bound everywhere: |got - ref| <= TOL * max(1, max|ref|) + TOL with TOL = 3e-5, the bound of tests/test_gpu_ops.py."""
import math
import re

import pytest
import torch

from dlsg_amd import limits
from dlsg_amd.engine import o2v_nsplit
from emul_ops import _mask

pytestmark = pytest.mark.gpu

TOL = 3e-5
OK, EINVAL = 0, -1
NAN = float('nan')
WORST = {}       # kernel -> largest error / bound seen in this run (printed by every test that adds to it)


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def status(fn, *a, **k):
    """the launcher's return code behind a HipOps wrapper (HipOps._check raises '<entry point> failed with code <rc>')"""
    try:
        fn(*a, **k)
    except RuntimeError as e:
        m = re.search(r'failed with code (-?\d+)', str(e))
        assert m, e
        return int(m.group(1))
    return OK


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def nans(*shape):
    return torch.full(shape, NAN, device='cuda')


def dev(*ts):
    return [t.cuda() for t in ts]


def untouched(outs, what):
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool(torch.isnan(t).all()), (what, k, 'written by a refused call')


def close(kernel, what, outs, refs):
    torch.cuda.synchronize()
    for k, ref in refs.items():
        got = outs[k].detach().cpu().double().reshape(ref.shape)
        assert bool(torch.isfinite(got).all()), (kernel, what, k, 'non-finite')
        err = (got - ref).abs().max().item()
        bound = TOL * max(1.0, ref.abs().max().item()) + TOL
        WORST[kernel] = max(WORST.get(kernel, 0.0), err / bound)
        assert err <= bound, (kernel, what, k, 'max err %g, bound %g' % (err, bound))


def report(kernel):
    print('%s: worst error / bound = %.3f' % (kernel, WORST.get(kernel, 0.0)))


def ln64(t, eps=1e-5):
    mean = t.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((t - mean) ** 2).mean(-1, keepdim=True) + eps)
    return mean, rstd


# ------------------------------------------------------------------------------------------------ LatentPSL
def psl_inputs(g, B, T, P, H):
    return dict(ov=rnd(g, B, T, H), th=rnd(g, P, H, scale=0.1), ga=1 + 0.2 * rnd(g, H), be=0.2 * rnd(g, H))


def psl_fwd_ref(ov, th, ga, be, mask=None, eps=1e-5):
    """float64: adj = softmax over the frames of ov theta^T, u = adj^T ov, out = Dropout(LayerNorm(tanh(u)))"""
    ov, th, ga, be = ov.double(), th.double(), ga.double(), be.double()
    B, T, H = ov.shape
    P = th.shape[0]
    adj = torch.softmax(ov @ th.t(), 1)
    u = (adj.transpose(1, 2) @ ov).reshape(B * P, H)
    y = torch.tanh(u)
    mean, rstd = ln64(y, eps)
    out = (y - mean) * rstd * ga + be
    if mask is not None:
        out = out * mask.double()
    return dict(adj=adj, u=u, out=out, st=torch.cat([mean, rstd], 1))


def psl_bwd_ref(dout, u, st, ga, adj, ov, th, mask=None):
    """float64 backward of psl_fwd_ref from the saved state as given (u, the statistics and adj are inputs of the kernel)"""
    dout, u, st, ga, adj, ov, th = [t.double() for t in (dout, u, st, ga, adj, ov, th)]
    B, T, H = ov.shape
    P = th.shape[0]
    y = torch.tanh(u)
    mean, rstd = st[:, :1], st[:, 1:2]
    x = (y - mean) * rstd
    g = dout if mask is None else dout * mask.double()
    part = torch.stack([(g * x).view(B, P, H).sum(1), g.view(B, P, H).sum(1)], 1)
    gx = g * ga
    du = (rstd * (gx - gx.mean(1, keepdim=True) - x * (gx * x).mean(1, keepdim=True)) * (1 - y * y)).view(B, P, H)
    dadj = ov @ du.transpose(1, 2)
    dlg = adj * (dadj - (adj * dadj).sum(1, keepdim=True))
    return dict(dov=(adj @ du + dlg @ th).reshape(B * T, H), dth=dlg.transpose(1, 2) @ ov, part=part)


def psl_fwd_outs(B, T, P, H):
    return dict(adj=nans(B, T, P), u=nans(B * P, H), out=nans(B * P, H), st=nans(B * P, 2))


def psl_bwd_outs(B, T, P, H):
    return dict(dov=nans(B * T, H), dth=nans(B, P, H), part=nans(B, 2, H))


@pytest.mark.parametrize('H', [4, 6, 64, 96, 512, 1024, 2048, 2052])
def test_latent_psl_forward_predicate_is_the_launcher(hip, H):
    """includes the 64-KB theta edges (P, H) = (32, 512), (16, 1024), (8, 2048), the first refused (17, 1024), (9, 2048), and
    (T, P, H) = (32, 8, 2048), (32, 32, 512): no limit on T x H"""
    g = torch.Generator().manual_seed(100 + H)
    seen = set()
    for T in (1, 32, 33):
        for P in (1, 8, 9, 16, 17, 32, 33):
            B = 1 + (T + P) % 2
            i = psl_inputs(g, B, T, P, H)
            o = psl_fwd_outs(B, T, P, H)
            ov, th, ga, be = dev(i['ov'], i['th'], i['ga'], i['be'])
            rc = status(hip.latent_psl_fwd, ov, th, ga, be, o['adj'], o['u'], o['out'], o['st'], p=0.0)
            want = hip.latent_psl_supported(T, P, H)
            assert want == limits.latent_psl(T, P, H)
            assert (rc == OK) == bool(want), ('latent_psl_fwd', (T, P, H), 'status %d, predicate %s' % (rc, want))
            seen.add(bool(want))
            if rc != OK:
                assert rc == EINVAL, (T, P, H, rc)
                untouched(o, ('latent_psl_fwd', T, P, H))
            else:
                close('latent_psl_fwd', (B, T, P, H), o, psl_fwd_ref(i['ov'], i['th'], i['ga'], i['be']))
    assert seen == ({False} if H in (6, 2052) else {True, False})
    report('latent_psl_fwd')


@pytest.mark.parametrize('H', [4, 96, 1024, 2048, 2052])
def test_latent_psl_backward_predicate_is_the_launcher(hip, H):
    """includes the 150-KB edge of the staged frame nodes: T = 29 / 30 at H = 1024"""
    g = torch.Generator().manual_seed(200 + H)
    for T in (1, 29, 30, 32, 33):
        for P in (1, 8, 9):
            B = 1 + (T + P) % 2
            i = psl_inputs(g, B, T, P, H)
            f = psl_fwd_ref(i['ov'], i['th'], i['ga'], i['be'])
            u, st, adj = f['u'].float(), f['st'].float(), f['adj'].float()
            dout = rnd(g, B * P, H)
            o = psl_bwd_outs(B, T, P, H)
            a = dev(dout, u, st, i['ga'], adj, i['ov'], i['th'])
            rc = status(hip.latent_psl_bwd, *a, o['dov'], o['dth'], o['part'], p=0.0)
            want = hip.latent_psl_bwd_supported(T, P, H)
            assert want == limits.latent_psl_bwd(T, P, H)
            assert (rc == OK) == bool(want), ('latent_psl_bwd', (T, P, H), 'status %d, predicate %s' % (rc, want))
            if rc != OK:
                assert rc == EINVAL, (T, P, H, rc)
                untouched(o, ('latent_psl_bwd', T, P, H))
            else:
                close('latent_psl_bwd', (B, T, P, H), o, psl_bwd_ref(dout, u, st, i['ga'], adj, i['ov'], i['th']))
    assert hip.latent_psl_bwd_supported(29, 8, 1024) and not hip.latent_psl_bwd_supported(30, 8, 1024)
    report('latent_psl_bwd')


# ------------------------------------------------------------------------------------------------ self-attention core
def sa_fwd_ref(K, Q, V, scale, mask):
    K, Q, V = K.double(), Q.double(), V.double()
    lg = (K @ Q.transpose(1, 2)) * scale
    if mask is not None:
        lg = torch.where(mask > 0, lg, torch.full_like(lg, -9e15))
    w = torch.softmax(lg, 2)
    return dict(w=w, out=w @ V)


def sa_bwd_ref(w, K, Q, V, dout, scale):
    w, K, Q, V, dout = [t.double() for t in (w, K, Q, V, dout)]
    dw = dout @ V.transpose(1, 2)
    dlg = w * (dw - (w * dw).sum(2, keepdim=True))
    return dict(dV=w.transpose(1, 2) @ dout, dK=scale * (dlg @ Q), dQ=scale * (dlg.transpose(1, 2) @ K))


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('D', [64, 96, 128, 2048])
def test_self_attention_core_predicate_is_the_launcher(hip, D, masked):
    """forward and backward; D = 2048 at B <= 2 spreads a clip's columns over several workgroups, D <= 128 does not"""
    g = torch.Generator().manual_seed(300 + D)
    scale = 1.0 / math.sqrt(D / 8.0)
    for T in (1, 32, 33):
        B = 1 + T % 2
        K, Q, V, dout = rnd(g, B, T, D, scale=0.3), rnd(g, B, T, D, scale=0.3), rnd(g, B, T, D), rnd(g, B, T, D)
        mask = (torch.rand(B, T, T, generator=g) > 0.3).float() if masked else None
        want = hip.sa_core_supported(T, D)
        assert want == limits.sa_core(T, D)
        o = dict(w=nans(B, T, T), out=nans(B, T, D))
        Kd, Qd, Vd, dd = dev(K, Q, V, dout)
        rc = status(hip.sa_core_fwd, Kd, Qd, Vd, o['w'], o['out'], scale, mask=None if mask is None else mask.cuda())
        assert (rc == OK) == bool(want), ('sa_core_fwd', (T, D), 'status %d, predicate %s' % (rc, want))
        f = sa_fwd_ref(K, Q, V, scale, mask)
        w = f['w'].float()
        ob = dict(dK=nans(B, T, D), dQ=nans(B, T, D), dV=nans(B, T, D))
        rcb = status(hip.sa_core_bwd, w.cuda(), Kd, Qd, Vd, dd, ob['dK'], ob['dQ'], ob['dV'], scale)
        assert (rcb == OK) == bool(want), ('sa_core_bwd', (T, D), 'status %d, predicate %s' % (rcb, want))
        if not want:
            assert rc == EINVAL and rcb == EINVAL
            untouched(o, ('sa_core_fwd', T, D))
            untouched(ob, ('sa_core_bwd', T, D))
        else:
            close('sa_core_fwd', (B, T, D, masked), o, f)
            close('sa_core_bwd', (B, T, D, masked), ob, sa_bwd_ref(w, K, Q, V, dout, scale))
    report('sa_core_fwd')
    report('sa_core_bwd')


# ------------------------------------------------------------------------------------------------ o2v graph
def o2v_fwd_ref(y, v, go, bo, scale, eps=1e-5):
    y, v, go, bo = y.double(), v.double(), go.double(), bo.double()
    B, NO, H = y.shape
    T = v.shape[1]
    mean, rstd = ln64(y, eps)
    o = (y - mean) * rstd * go + bo
    S = scale * (o @ v.transpose(1, 2))
    m = S.max(1, keepdim=True)[0]
    l = torch.exp(S - m).sum(1, keepdim=True)
    p = torch.exp(S - m) / l
    return dict(z=(p.transpose(1, 2) @ o + v).reshape(B * T, H), S=S, ostats=torch.cat([mean.reshape(-1, 1), rstd.reshape(-1, 1)], 1),
                ml=torch.stack([m.reshape(-1), l.reshape(-1)], 1))


def o2v_bwd_ref(y, ostats, go, bo, v, S, dz, scale):
    y, ostats, go, bo, v, S, dz = [t.double() for t in (y, ostats, go, bo, v, S, dz)]
    B, NO, H = y.shape
    xh = (y - ostats[:, :1].view(B, NO, 1)) * ostats[:, 1:2].view(B, NO, 1)
    o = xh * go + bo
    P = torch.softmax(S, 1)
    dP = o @ dz.transpose(1, 2)
    dS = P * (dP - (P * dP).sum(1, keepdim=True))
    do = P @ dz + scale * (dS @ v)
    gx = do * go
    d = ostats[:, 1:2].view(B, NO, 1) * (gx - gx.mean(2, keepdim=True) - xh * (gx * xh).mean(2, keepdim=True))
    dy = d * (1 - y * y)
    return dict(dy=dy, dv=dz + scale * (dS.transpose(1, 2) @ o), part=torch.stack([(do * xh).sum(1), do.sum(1)], 1), dysum=dy.sum(1))


@pytest.mark.parametrize('H', [64, 96, 512, 1024, 2048])
def test_o2v_graph_predicate_is_the_launcher(hip, H):
    """forward and backward, 16 objects per frame, the chunk count the engine would choose"""
    g = torch.Generator().manual_seed(400 + H)
    O = 16
    scale = 1.0 / math.sqrt(H / 4.0)
    for T in (32, 33):
        B = 1 + T % 2
        NO = T * O
        ns = o2v_nsplit(B, NO)
        y, v, go, bo, dz = torch.tanh(rnd(g, B, NO, H)), rnd(g, B, T, H), 1 + 0.2 * rnd(g, H), 0.2 * rnd(g, H), rnd(g, B, T, H)
        want = hip.o2v_supported(T, H)
        assert want == limits.o2v(T, H)
        o = dict(z=nans(B * T, H), ml=nans(B * T, 2), ostats=nans(B * NO, 2), S=nans(B, NO, T))
        yd, vd, god, bod, dzd = dev(y, v, go, bo, dz)
        rc = status(hip.o2v_fwd, yd, vd, god, bod, o['z'], o['ml'], o['ostats'], o['S'], scale, ns)
        assert (rc == OK) == bool(want), ('o2v_fwd', (T, H), 'status %d, predicate %s' % (rc, want))
        f = o2v_fwd_ref(y, v, go, bo, scale)
        st, S, ml, z = [f[k].float() for k in ('ostats', 'S', 'ml', 'z')]
        ob = dict(dy=nans(B, NO, H), dv=nans(B, T, H), dysum=nans(B * ns, H))
        item = dict(y=yd, ostats=st.cuda(), g_obj=god, b_obj=bod, v=vd, z=z.cuda().view(B, T, H), dz=dzd, S=S.cuda(), ml=ml.cuda(),
                    dy=ob['dy'], dv=ob['dv'], dysum=ob['dysum'])
        parts = []
        rcb = status(lambda: parts.extend(hip.o2v_bwd_multi([item], scale, ns)))
        assert (rcb == OK) == bool(want), ('o2v_bwd', (T, H), 'status %d, predicate %s' % (rcb, want))
        if not want:
            assert rc == EINVAL and rcb == EINVAL
            untouched(o, ('o2v_fwd', T, H))
            untouched(ob, ('o2v_bwd', T, H))
        else:
            torch.cuda.synchronize()
            got = dict(z=o['z'], S=o['S'], ostats=o['ostats'], lse=o['ml'][:, 0] + torch.log(o['ml'][:, 1]))
            ref = dict(z=f['z'], S=f['S'], ostats=f['ostats'], lse=f['ml'][:, 0] + torch.log(f['ml'][:, 1]))
            close('o2v_fwd', (B, T, H, ns), got, ref)
            gotb = dict(dy=ob['dy'], dv=ob['dv'], part=parts[0].view(B, ns, 2, H).sum(1), dysum=ob['dysum'].view(B, ns, H).sum(1))
            close('o2v_bwd', (B, T, H, ns), gotb, o2v_bwd_ref(y, st, go, bo, v, S, dz, scale))
    report('o2v_fwd')
    report('o2v_bwd')


# ------------------------------------------------------------------------------------------------ persistent recurrences
@pytest.mark.parametrize('B,H', [(65, 64), (3, 96), (65, 96)])
def test_persistent_bilstm_refuses_what_its_predicate_refuses(hip, B, H):
    T = 3
    assert hip.bilstm_supported(3, T, 64), 'a whole MI355X is expected: 2 * H / 8 compute units'
    assert not hip.bilstm_supported(B, T, H)
    z = lambda *s: torch.zeros(*s, device='cuda')
    two = lambda *s: [z(*s), z(*s)]
    out = nans(B, T, 2 * H)
    rc = status(hip.bilstm_fwd, two(B * T, 4 * H), two(4 * H, H), two(4 * H), two(4 * H), out, two(B, T, H), two(B, T, H),
                two(B, T, 4 * H))
    assert rc == EINVAL
    dg = [nans(B, T, 4 * H), nans(B, T, 4 * H)]
    rcb = status(hip.bilstm_bwd, two(B, T, 4 * H), two(B, T, H), z(B, T, 2 * H), two(4 * H, H), dg)
    assert rcb == EINVAL
    untouched(dict(out=out, dg0=dg[0], dg1=dg[1]), ('bilstm', B, H))


@pytest.mark.parametrize('level', [0, 1])
def test_critic_lstm_seq_refuses_what_its_predicate_refuses(hip, level):
    """H = 96 is outside {64, 512}: the predicate answers 0 and the launcher returns DLSG_EINVAL before its first launch"""
    import ctypes as C
    from dlsg_amd import abi
    L, n, H = 4, 65, 96
    assert hip.lstm_seq_supported(L, n, 64) and not hip.lstm_seq_supported(L, n, H)
    z = lambda *s: torch.zeros(*s, device='cuda')
    outs = dict(Hs=nans(n, L, H), Cs=nans(n, L, H), DA=nans(n, L, 4 * H), DH=nans(n, L, H), DC=nans(n, L, H))
    keep = dict(W=z(4 * H, H), addend=z(n, L, 4 * H), As=z(n, L, 4 * H), dHs=z(n, L, H), xbuf=z(L * 4 * H * 128), xbuf2=z(L * 4 * H * 128),
                flags=torch.zeros(4096, dtype=torch.int32, device='cuda'), err=torch.zeros(1, dtype=torch.int32, device='cuda'))
    a = abi.dlsg_lstm_seq_args()
    for k, t in list(keep.items()) + list(outs.items()):
        setattr(a, k, C.c_void_p(t.data_ptr()))
    a.L, a.n, a.H, a.batch_major = L, n, H, 1
    assert hip.lib.dlsg_lstm_seq(C.byref(a), level, hip._stream()) == EINVAL
    untouched(outs, ('lstm_seq', level))


# ------------------------------------------------------------------------------------------------ grouped launches
def rowln_ref(x, ga, be, res=None, pre_tanh=0, mask=None, eps=1e-5):
    z = x.double() if res is None else x.double() + res.double()
    t = torch.tanh(z) if pre_tanh == 1 else z
    mean, rstd = ln64(t, eps)
    v = (t - mean) * rstd * ga.double() + be.double()
    if mask is not None:
        v = v * mask.double()
    return dict(y=v, st=torch.cat([mean, rstd], 1)), t


def rowln_bwd_ref(dy, x, ga, st, nblk, res=None, pre_tanh=0, mask=None, dx_old=None, eps=1e-5):
    """st None: the kernel recomputes the statistics.  Block b of the launch owns rows b, b + nblk, ...: dgb_part[b]"""
    f, t = rowln_ref(x, ga, torch.zeros_like(ga), res, pre_tanh, None, eps)
    st = f['st'] if st is None else st.double()
    xh = (t - st[:, :1]) * st[:, 1:2]
    g = dy.double() if mask is None else dy.double() * mask.double()
    gx = g * ga.double()
    d = st[:, 1:2] * (gx - gx.mean(1, keepdim=True) - xh * (gx * xh).mean(1, keepdim=True))
    if pre_tanh:
        d = d * (1 - t * t)
    if dx_old is not None:
        d = d + dx_old.double()
    part = torch.stack([torch.stack([(g[b::nblk] * xh[b::nblk]).sum(0), g[b::nblk].sum(0)]) for b in range(nblk)])
    return dict(dx=d, part=part)


def rowln_items(g, rows, widths=(48, 2048)):
    """item 0: plain, with statistics; item 1: tanh(x + res) with dropout, no statistics kept"""
    na, nb = widths
    a = dict(x=rnd(g, rows, na + 8)[:, 4:4 + na], gamma=1 + 0.2 * rnd(g, na), beta=0.2 * rnd(g, na), dy=rnd(g, rows, na), dx0=rnd(g, rows, na))
    b = dict(x=rnd(g, rows, nb), gamma=1 + 0.2 * rnd(g, nb), beta=0.2 * rnd(g, nb), res=rnd(g, rows, nb), dy=rnd(g, rows, nb))
    return a, b


def rowln_fwd_calls(a, b, rows):
    """-> (device argument dicts of the two items with NaN outputs, the outputs by name)"""
    ca = dict(x=a['x'].cuda(), gamma=a['gamma'].cuda(), beta=a['beta'].cuda(), y=nans(rows, a['x'].shape[1]), stats=nans(rows, 2))
    cb = dict(x=b['x'].cuda(), gamma=b['gamma'].cuda(), beta=b['beta'].cuda(), y=nans(rows, b['x'].shape[1]), res=b['res'].cuda(),
              pre_tanh=1, p1=0.3, site1=5, seed=77)
    return [ca, cb], dict(ya=ca['y'], sta=ca['stats'], yb=cb['y'])


def rowln_bwd_calls(hip, a, b, rows, sta, nblk=None):
    nblk = hip.rowln_bwd_nblk(rows) if nblk is None else nblk
    ca = dict(dy=a['dy'].cuda(), x=a['x'].cuda(), gamma=a['gamma'].cuda(), beta=a['beta'].cuda(), dx=a['dx0'].cuda(), stats=sta.cuda(),
              dgb_part=nans(nblk, 2, a['x'].shape[1]), accum_dx=True)
    cb = dict(dy=b['dy'].cuda(), x=b['x'].cuda(), gamma=b['gamma'].cuda(), beta=b['beta'].cuda(), dx=nans(rows, b['x'].shape[1]),
              res=b['res'].cuda(), pre_tanh=1, p1=0.3, site1=5, seed=77, dgb_part=nans(nblk, 2, b['x'].shape[1]))
    return [ca, cb], dict(dxa=ca['dx'], pa=ca['dgb_part'], dxb=cb['dx'], pb=cb['dgb_part'])


@pytest.mark.parametrize('rows', [37, 300])
def test_rowln_grouped_launch_of_two_different_items(hip, rows):
    """n = 48 beside n = 2048, one item plain with statistics and accum_dx, the other tanh(x + res) with dropout and recomputed
    statistics: a wrong blockIdx.y -> item mapping cannot pass"""
    g = torch.Generator().manual_seed(500 + rows)
    a, b = rowln_items(g, rows)
    mask = _mask(77, 5, rows, 2048, 0.3)
    multi, mo = rowln_fwd_calls(a, b, rows)
    single, so = rowln_fwd_calls(a, b, rows)
    hip.rowln_fwd_multi(multi)
    for c in single:
        hip.rowln_fwd(**c)
    torch.cuda.synchronize()
    for k in mo:
        assert torch.equal(mo[k], so[k]), k
    fa, _ = rowln_ref(a['x'], a['gamma'], a['beta'])
    fb, _ = rowln_ref(b['x'], b['gamma'], b['beta'], b['res'], 1, mask)
    close('rowln_fwd', rows, so, dict(ya=fa['y'], sta=fa['st'], yb=fb['y']))
    sta = fa['st'].float()
    nblk = hip.rowln_bwd_nblk(rows)
    multi, mo = rowln_bwd_calls(hip, a, b, rows, sta)
    single, so = rowln_bwd_calls(hip, a, b, rows, sta)
    hip.rowln_bwd_multi(multi)
    for c in single:
        hip.rowln_bwd(**c)
    torch.cuda.synchronize()
    for k in mo:
        assert torch.equal(mo[k], so[k]), k
    ra = rowln_bwd_ref(a['dy'], a['x'], a['gamma'], sta, nblk, dx_old=a['dx0'])
    rb = rowln_bwd_ref(b['dy'], b['x'], b['gamma'], None, nblk, b['res'], 1, mask)
    close('rowln_bwd', rows, so, dict(dxa=ra['dx'], pa=ra['part'], dxb=rb['dx'], pb=rb['part']))
    report('rowln_fwd')
    report('rowln_bwd')


def test_rowln_grouped_launch_refusals(hip):
    """count 0 and 3, unequal rows, n = 2049, a dgb_part of the wrong block count: DLSG_EINVAL, nothing written"""
    g = torch.Generator().manual_seed(7)
    rows = 37
    a, b = rowln_items(g, rows)
    a2, _ = rowln_items(g, rows + 1)
    w, _ = rowln_items(g, rows, widths=(2049, 48))
    sta = torch.zeros(rows, 2)
    sta[:, 1] = 1.0

    def fwd(items, extra_rows=None):
        calls, outs = [], {}
        for i, it in enumerate(items):
            r = it['x'].shape[0]
            c = dict(x=it['x'].cuda(), gamma=it['gamma'].cuda(), beta=it['beta'].cuda(), y=nans(r, it['x'].shape[1]), stats=nans(r, 2))
            calls.append(c)
            outs.update({'y%d' % i: c['y'], 'st%d' % i: c['stats']})
        return calls, outs

    def bwd(items, nblk):
        calls, outs = [], {}
        for i, it in enumerate(items):
            r, n = it['x'].shape
            c = dict(dy=it['dy'].cuda(), x=it['x'].cuda(), gamma=it['gamma'].cuda(), beta=it['beta'].cuda(), dx=nans(r, n),
                     dgb_part=nans(nblk, 2, n))
            calls.append(c)
            outs.update({'dx%d' % i: c['dx'], 'p%d' % i: c['dgb_part']})
        return calls, outs

    good = hip.rowln_bwd_nblk(rows)
    for what, items in (('count 3', [a, b, a]), ('unequal rows', [a, a2]), ('n = 2049', [a, w])):
        calls, outs = fwd(items)
        assert status(hip.rowln_fwd_multi, calls) == EINVAL, what
        untouched(outs, ('rowln_fwd_multi', what))
        calls, outs = bwd(items, good)
        assert status(hip.rowln_bwd_multi, calls) == EINVAL, what
        untouched(outs, ('rowln_bwd_multi', what))
    assert status(hip.rowln_fwd_multi, []) == EINVAL and status(hip.rowln_bwd_multi, []) == EINVAL
    for nblk in (good - 1, good + 1):
        calls, outs = bwd([a, b], nblk)
        assert status(hip.rowln_bwd_multi, calls) == EINVAL, nblk
        untouched(outs, ('rowln_bwd_multi', 'nblk', nblk))
        calls, outs = bwd([a], nblk)
        assert status(hip.rowln_bwd_multi, calls) == EINVAL, nblk
        untouched(outs, ('rowln_bwd', 'nblk', nblk))
    calls, outs = bwd([a, b], good)               # the same arguments with the right block count are taken
    assert status(hip.rowln_bwd_multi, calls) == OK
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in outs.values())


def psl_fwd_call(i, B, T, P, H, site):
    o = psl_fwd_outs(B, T, P, H)
    ov, th, ga, be = dev(i['ov'], i['th'], i['ga'], i['be'])
    return dict(ov=ov, theta=th, gamma=ga, beta=be, adj=o['adj'], u=o['u'], out=o['out'], stats=o['st'], p=0.3, site=site, seed=9), o


def psl_bwd_call(i, f, dout, B, T, P, H, site):
    o = psl_bwd_outs(B, T, P, H)
    d, u, st, ga, adj, ov, th = dev(dout, f['u'].float(), f['st'].float(), i['ga'], f['adj'].float(), i['ov'], i['th'])
    return dict(dout=d, u=u, stats=st, gamma=ga, adj=adj, ov=ov, theta=th, dov=o['dov'], dtheta_part=o['dth'], part=o['part'], p=0.3,
                site=site, seed=9), o


def test_latent_psl_forward_grouped_launch_of_two_different_items(hip):
    """T = 7 beside T = 32 at equal B, P, H, each with its own dropout site"""
    g = torch.Generator().manual_seed(61)
    B, P, H = 3, 5, 96
    items = [(T, site, psl_inputs(g, B, T, P, H)) for T, site in ((7, 11), (32, 12))]
    multi = [psl_fwd_call(i, B, T, P, H, site) for T, site, i in items]
    single = [psl_fwd_call(i, B, T, P, H, site) for T, site, i in items]
    hip.latent_psl_fwd_multi([c for c, _ in multi])
    for c, _ in single:
        hip.latent_psl_fwd(**c)
    torch.cuda.synchronize()
    for (_, mo), (_, so), (T, site, i) in zip(multi, single, items):
        for k in mo:
            assert torch.equal(mo[k], so[k]), (T, k)
        close('latent_psl_fwd', ('grouped', T), so, psl_fwd_ref(i['ov'], i['th'], i['ga'], i['be'], _mask(9, site, B * P, H, 0.3)))
    report('latent_psl_fwd')


def test_latent_psl_backward_grouped_launch_of_two_different_items(hip):
    """P = 1 beside P = 8 at equal B, T, H, each with its own dropout site"""
    g = torch.Generator().manual_seed(62)
    B, T, H = 3, 26, 96
    multi, single, refs = [], [], []
    for P, site in ((1, 11), (8, 12)):
        i = psl_inputs(g, B, T, P, H)
        f = psl_fwd_ref(i['ov'], i['th'], i['ga'], i['be'])
        dout = rnd(g, B * P, H)
        multi.append(psl_bwd_call(i, f, dout, B, T, P, H, site))
        single.append(psl_bwd_call(i, f, dout, B, T, P, H, site))
        refs.append(psl_bwd_ref(dout, f['u'].float(), f['st'].float(), i['ga'], f['adj'].float(), i['ov'], i['th'],
                                _mask(9, site, B * P, H, 0.3)))
    hip.latent_psl_bwd_multi([c for c, _ in multi])
    for c, _ in single:
        hip.latent_psl_bwd(**c)
    torch.cuda.synchronize()
    for (_, mo), (_, so), ref in zip(multi, single, refs):
        for k in mo:
            assert torch.equal(mo[k], so[k]), k
        close('latent_psl_bwd', 'grouped', so, ref)
    report('latent_psl_bwd')


def test_latent_psl_grouped_launch_refusals(hip):
    """count 0 and 3; forward items of unequal P or H; backward items of unequal T: DLSG_EINVAL, nothing written"""
    g = torch.Generator().manual_seed(63)
    B = 2

    def fwd(shapes):
        calls, outs = [], {}
        for n, (T, P, H) in enumerate(shapes):
            c, o = psl_fwd_call(psl_inputs(g, B, T, P, H), B, T, P, H, 3)
            calls.append(c)
            outs.update({'%s%d' % (k, n): t for k, t in o.items()})
        return calls, outs

    def bwd(shapes):
        calls, outs = [], {}
        for n, (T, P, H) in enumerate(shapes):
            i = psl_inputs(g, B, T, P, H)
            c, o = psl_bwd_call(i, psl_fwd_ref(i['ov'], i['th'], i['ga'], i['be']), rnd(g, B * P, H), B, T, P, H, 3)
            calls.append(c)
            outs.update({'%s%d' % (k, n): t for k, t in o.items()})
        return calls, outs

    for what, shapes in (('count 3', [(7, 5, 64)] * 3), ('unequal P', [(7, 5, 64), (7, 6, 64)]), ('unequal H', [(7, 5, 64), (7, 5, 96)])):
        calls, outs = fwd(shapes)
        assert status(hip.latent_psl_fwd_multi, calls) == EINVAL, what
        untouched(outs, ('latent_psl_fwd_multi', what))
    for what, shapes in (('count 3', [(7, 5, 64)] * 3), ('unequal T', [(7, 5, 64), (8, 5, 64)]), ('unequal H', [(7, 5, 64), (7, 5, 96)])):
        calls, outs = bwd(shapes)
        assert status(hip.latent_psl_bwd_multi, calls) == EINVAL, what
        untouched(outs, ('latent_psl_bwd_multi', what))
    assert status(hip.latent_psl_fwd_multi, []) == EINVAL and status(hip.latent_psl_bwd_multi, []) == EINVAL

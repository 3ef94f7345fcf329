"""GPU (-m gpu): dlsg_adamw_ema -- weight decay (decoupled and L2) and the averaged weights inside Adam's launch -- against the
emulation and torch on the CPU, its decay table, its idle and skip paths, dlsg_swap_f32, and the Trainer / SCSTTrainer steps that
carry them (eager, captured, with the RCCL collectives in the graph, `averaged()` under a captured beam search).
Host logic: tests/test_adamw_ema_host.py."""
import copy
import functools
import random

import pytest
import torch

import dlsg_amd
from test_adamw_ema_host import DecayEmul, DecayOracle, arena_error, ndim_filter
from test_grad_clip_host import check_weights
from test_gpu_grad_clip import build, adam_state, bits, HP

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ARRAYS = ('p', 'm', 'v', 'ema')


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def table_for(n, ends=((0, 1), (3, 70), (1000, 1026))):
    """the decay table of these tests, ends deliberately no multiples of 4, cut to n elements"""
    return [(lo, min(hi, n)) for lo, hi in ends if lo < n]


def close(got, ref):
    """the project's 1e-6 Adam bound, by magnitude: the decoupled factor multiplies p itself, so its rounding is one ulp of p"""
    return bool(((got - ref).abs() <= 1e-6 * ref.abs().clamp(min=1.0)).all())


def run_both(hip, off, n, seed, table=None, with_ema=True, **kw):
    """one dlsg_adamw_ema launch over [off, off + n) of longer arrays, and the emulation of it on the CPU -> two dicts of whole arrays"""
    tot = off + n + 9
    p0, gr, m0, v0 = adam_state(seed, tot)
    e0 = p0 + 0.01 * torch.randn(tot, generator=torch.Generator().manual_seed(seed + 1))
    sl = slice(off, off + n)
    tab = None if table is None else torch.tensor(table, dtype=torch.int64).view(-1, 2)
    dev = dict(p=p0.to(DEV), g=gr.to(DEV), m=m0.to(DEV), v=v0.to(DEV), ema=e0.to(DEV))
    hip.adamw_ema(dev['p'][sl], dev['g'][sl], dev['m'][sl], dev['v'][sl], *HP, ema=dev['ema'][sl] if with_ema else None,
                  decay_ranges=None if tab is None else tab.to(DEV), **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    ref = dict(p=p0.clone(), m=m0.clone(), v=v0.clone(), ema=e0.clone())
    DecayEmul().adamw_ema(ref['p'][sl], gr[sl], ref['m'][sl], ref['v'][sl], *HP, ema=ref['ema'][sl] if with_ema else None,
                          decay_ranges=tab, **kw)
    start = dict(p=p0, m=m0, v=v0, ema=e0)
    return {k: dev[k].cpu() for k in ARRAYS}, ref, start


def check_range(got, ref, start, off, n, with_ema=True):
    for k in ARRAYS:
        assert close(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
        assert torch.equal(bits(got[k][:off]), bits(start[k][:off])) and torch.equal(bits(got[k][off + n:]), bits(start[k][off + n:])), k
    assert not torch.equal(ref['p'], start['p']) and torch.equal(ref['ema'], start['ema']) != with_ema
    if not with_ema:
        assert torch.equal(bits(got['ema']), bits(start['ema']))


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize('decoupled', [True, False])
@pytest.mark.parametrize('off,n', [(0, 5000), (1, 4999), (3, 1026), (2, 3), (5, 1), (0, 4), (7, 100003)])
def test_adamw_ema_ranges_at_any_offset_with_a_table_off_the_16_byte_grid(hip, off, n, decoupled):
    """offsets and sizes of tests/test_gpu_ops.py::test_adam_ranges_at_any_offset; clip record and clamp both active, so the order
    clip -> decay -> update -> average is what is compared"""
    rec = torch.tensor([3.0, 0.37, 0.0, 0.0])
    table = table_for(n)
    for with_ema in (True, False):
        for tab in (table, None):
            got, ref, start = run_both(hip, off, n, off * 100 + n, tab, with_ema, weight_decay=0.1, decoupled=decoupled, ema_decay=0.9,
                                       record=rec, clip_value=0.3)
            check_range(got, ref, start, off, n, with_ema)
    # the table took part: inside it the launch without decay ends elsewhere, outside it does not
    got = run_both(hip, off, n, off * 100 + n, table, True, weight_decay=0.1, decoupled=decoupled, ema_decay=0.9, record=rec,
                   clip_value=0.3)[0]
    plain = run_both(hip, off, n, off * 100 + n, None, True, weight_decay=0.0, decoupled=decoupled, ema_decay=0.9, record=rec,
                     clip_value=0.3)[0]
    inside = torch.zeros(off + n + 9, dtype=torch.bool)
    for lo, hi in table:
        inside[off + lo:off + hi] = True
    assert torch.equal(bits(got['p'][~inside]), bits(plain['p'][~inside])) and torch.equal(bits(got['v'][~inside]), bits(plain['v'][~inside]))
    moved = bits(got['p'][inside]) != bits(plain['p'][inside])
    assert float(moved.float().mean()) > 0.9


def test_hyper_words_override_the_scalars_and_give_the_same_result(hip):
    """the four device words a replayed graph reads, computed in float64 and rounded once, against the launch that derives them"""
    off, n = 1, 4999
    lr, b1, b2, eps, step, gs = HP
    wd, d = 0.1, 0.9
    for decoupled in (True, False):
        hyper = torch.tensor([lr / (1.0 - b1 ** step), (1.0 - b2 ** step) ** 0.5, 1.0 - lr * wd if decoupled else wd, 1.0 - d],
                             dtype=torch.float64).float()
        a = run_both(hip, off, n, 7, table_for(n), True, weight_decay=wd, decoupled=decoupled, ema_decay=d)
        # (scalars deliberately wrong where hyper replaces them; weight_decay > 0 only selects the decaying kernel)
        p0, gr, m0, v0 = adam_state(7, off + n + 9)
        e0 = a[2]['ema']
        sl = slice(off, off + n)
        dev = dict(p=p0.to(DEV), g=gr.to(DEV), m=m0.to(DEV), v=v0.to(DEV), ema=e0.to(DEV))
        hip.adamw_ema(dev['p'][sl], dev['g'][sl], dev['m'][sl], dev['v'][sl], 1.0, b1, b2, eps, 1, gs, weight_decay=7.0,
                      decoupled=decoupled, ema=dev['ema'][sl], ema_decay=0.5, hyper=hyper.to(DEV),
                      decay_ranges=torch.tensor(table_for(n), dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        for k in ARRAYS:
            assert close(dev[k].cpu(), a[1][k]), k


def test_three_steps_match_torch_adamw_and_a_lerp_ema(hip):
    """tests/test_gpu_ops.py::test_adam_matches_torch_optim with weight decay and an EMA kept by lerp_"""
    g = torch.Generator().manual_seed(3)
    p0, grads = torch.randn(5000, generator=g), [torch.randn(5000, generator=g) for _ in range(3)]
    lr, wd, d = 1.6e-4, 1e-2, 0.9
    for cls, decoupled in ((torch.optim.AdamW, True), (torch.optim.Adam, False)):
        ref = torch.nn.Parameter(p0.clone())
        opt = cls([ref], lr=lr, betas=(0.5, 0.9), weight_decay=wd)
        ema_ref = p0.clone()
        p = p0.clone().to(DEV); m = torch.zeros_like(p); v = torch.zeros_like(p); ema = p.clone()
        for i, gr in enumerate(grads):
            ref.grad = gr.clone() / 4
            opt.step()
            ema_ref.lerp_(ref.detach(), 1 - d)
            hip.adamw_ema(p, gr.to(DEV), m, v, lr, 0.5, 0.9, 1e-8, i + 1, 0.25, weight_decay=wd, decoupled=decoupled, ema=ema, ema_decay=d)
        torch.cuda.synchronize()
        st = opt.state[ref]
        for got, want in ((p, ref.detach()), (m, st['exp_avg']), (v, st['exp_avg_sq']), (ema, ema_ref)):
            assert close(got.cpu(), want), float((got.cpu() - want).abs().max())
        assert float((ema_ref - ref.detach()).abs().max()) > 1e-5


def test_idle_options_give_adam_clippeds_bits(hip):
    off, n = 1, 100003
    p0, gr, m0, v0 = adam_state(5, off + n + 9)
    sl = slice(off, off + n)
    rec = torch.tensor([3.0, 0.37, 0.0, 0.0], device=DEV)

    def run(fn, **kw):
        p, m, v, g = p0.to(DEV), m0.to(DEV), v0.to(DEV), gr.to(DEV)
        fn(p[sl], g[sl], m[sl], v[sl], *HP, record=rec, clip_value=0.3, **kw)
        torch.cuda.synchronize()
        return p, m, v
    want = run(hip.adam_clipped)
    assert not torch.equal(want[0], p0.to(DEV))
    ema = p0.to(DEV)
    tab = torch.tensor(table_for(n), dtype=torch.int64, device=DEV)
    for kw in (dict(), dict(weight_decay=0.0, ema=None, decay_ranges=None), dict(decoupled=False),
               dict(decay_ranges=tab),                                                    # no decay: the table is not read
               dict(ema=ema[sl], ema_decay=0.9)):                                          # the average does not touch p, m, v
        got = run(hip.adamw_ema, **kw)
        for a, b in zip(got, want):
            assert torch.equal(bits(a), bits(b)), sorted(kw)
    assert not torch.equal(ema, p0.to(DEV))


def test_a_non_finite_record_and_the_time_out_word_keep_all_four_arrays(hip):
    n = 4099
    p0, gr, m0, v0 = adam_state(9, n)
    start = dict(p=p0, m=m0, v=v0, ema=p0 * 0.5)
    tab = torch.tensor(table_for(n), dtype=torch.int64, device=DEV)

    def launch(rec):
        dev = {k: t.to(DEV) for k, t in start.items()}
        hip.adamw_ema(dev['p'], gr.to(DEV), dev['m'], dev['v'], *HP, weight_decay=0.1, ema=dev['ema'], ema_decay=0.9, record=rec,
                      decay_ranges=tab)
        torch.cuda.synchronize()
        return dev

    def unchanged(dev):
        return [k for k in ARRAYS if torch.equal(bits(dev[k].cpu()), bits(start[k]))]
    assert unchanged(launch(torch.tensor([1.0, 1.0, 0.0, 0.0], device=DEV))) == []
    assert unchanged(launch(torch.tensor([float('nan'), 0.0, 1.0, 0.0], device=DEV))) == list(ARRAYS)
    # the persistent kernels' time-out word (tests/test_gpu_ops.py::test_adam_is_guarded_by_the_persistent_time_out_word): set, not provoked
    word = hip._persist_word(tab.device)
    try:
        word.fill_(7)
        assert unchanged(launch(None)) == list(ARRAYS)
    finally:
        word.zero_()
    torch.cuda.synchronize()
    assert unchanged(launch(None)) == []


def test_a_full_table_is_accepted_and_one_more_interval_is_refused(hip):
    from dlsg_amd.hip import ADAM_MAX_RANGES
    assert ADAM_MAX_RANGES == dlsg_amd.abi.defines['DLSG_ADAM_MAX_RANGES'] >= 256
    table = [(40 * i + 1, 40 * i + 2 + i % 7) for i in range(ADAM_MAX_RANGES)]         # every interval off the 16-byte grid
    n = 40 * ADAM_MAX_RANGES + 3
    got, ref, start = run_both(hip, 3, n, 21, table, True, weight_decay=0.1, decoupled=True, ema_decay=0.9)
    check_range(got, ref, start, 3, n)
    plain = run_both(hip, 3, n, 21, None, True, weight_decay=0.0, ema_decay=0.9)[0]
    inside = torch.zeros(3 + n + 9, dtype=torch.bool)
    for lo, hi in table:
        inside[3 + lo:3 + hi] = True
    assert torch.equal(bits(got['p'][~inside]), bits(plain['p'][~inside]))
    assert float((bits(got['p'][inside]) != bits(plain['p'][inside])).float().mean()) > 0.9
    # one more: DLSG_EINVAL from the host side of the entry point, nothing launched
    table.append((40 * ADAM_MAX_RANGES + 1, 40 * ADAM_MAX_RANGES + 2))
    p0, gr, m0, v0 = adam_state(21, n)
    dev = [t.to(DEV) for t in (p0, gr, m0, v0, p0)]
    with pytest.raises(RuntimeError, match='code -1'):
        hip.adamw_ema(dev[0], dev[1], dev[2], dev[3], *HP, weight_decay=0.1, ema=dev[4], ema_decay=0.9,
                      decay_ranges=torch.tensor(table, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    for a, b in zip(dev, (p0, gr, m0, v0, p0)):
        assert torch.equal(bits(a.cpu()), bits(b))
    with pytest.raises(RuntimeError, match='code -1'):
        hip.adamw_ema(dev[0], dev[1], dev[2], dev[3], *HP, weight_decay=-0.1)


@pytest.mark.parametrize('n', [1, 4, 1026, 100003])
def test_swap_exchanges_two_arrays_in_place(hip, n):
    g = torch.Generator().manual_seed(n)
    a0, b0 = torch.randn(n + 12, generator=g), torch.randn(n + 12, generator=g)
    for oa, ob in ((1, 1), (1, 2), (0, 0)):                 # a shared alignment off the 16-byte grid, two alignments, aligned
        a, b = a0.to(DEV), b0.to(DEV)
        hip.swap(a[oa:oa + n], b[ob:ob + n])
        torch.cuda.synchronize()
        wa, wb = a0.clone(), b0.clone()
        wa[oa:oa + n], wb[ob:ob + n] = b0[ob:ob + n], a0[oa:oa + n]
        assert torch.equal(bits(a.cpu()), bits(wa)) and torch.equal(bits(b.cpu()), bits(wb)), (oa, ob)
    hip.swap(a[1:1 + n], a[1:1 + n])                        # an array against itself: as it was
    torch.cuda.synchronize()
    assert torch.equal(bits(a.cpu()), bits(wa))


# ---------------------------------------------------------------- Trainer, small config (B = 3)
LR, WD, D = 1e-3, 0.5, 0.9                                  # tests/test_adamw_ema_host.py's: the decay is 15 times the bound
OPTS = dict(lr=LR, weight_decay=WD, decay_filter=ndim_filter, ema_decay=D, ema_warmup=True)


def two_steps(**kw):
    """-> (trainer, [(weights, m, v, ema) after each of two steps])"""
    collectives = kw.pop('force_collectives', False)
    net, args, vocab, sd, (frames, regions, caps, lens) = build()
    tr = dlsg_amd.Trainer(net, **kw)
    tr.force_collectives = collectives
    out = []
    for _ in range(2):
        tr.step(frames.to(DEV), regions.to(DEV), caps.to(DEV), lens, 1.0)
        torch.cuda.synchronize()
        out.append(tuple(t.clone() for t in (net._flat, tr.m, tr.v, tr.ema)))
    return tr, out


@functools.lru_cache(maxsize=None)
def captured_run():
    """the captured trainer's two steps (decay under a filter, warmed-up average, an active norm clip), made once"""
    return two_steps(use_graphs=True, max_grad_norm=0.5, **OPTS)


def test_trainer_eager_and_captured_steps_agree_bit_for_bit():
    tr_g, captured = captured_run()
    tr_e, eager = two_steps(use_graphs=False, device_coins=True, max_grad_norm=0.5, **OPTS)
    assert tr_g._graphs is not None and len(tr_g._graphs) == 1 and tr_e._graphs is None
    assert tr_g._static['hyper'].numel() == 4
    for e, g in zip(eager, captured):
        for name, a, b in zip(('weights',) + ARRAYS[1:], e, g):
            assert torch.equal(bits(a), bits(b)), name
    assert not torch.equal(captured[0][3], captured[0][0]) and not torch.equal(captured[0][3], captured[1][3])
    assert float(tr_g._clip_rec[1]) < 1.0 and int(tr_g.skipped_steps) == 0           # the clip was active


def test_trainer_steps_match_the_oracle_with_adamw_and_a_lerp_ema():
    """as tests/test_adamw_ema_host.py, at the bound of tests/test_gpu_parity.py::test_trainer_step_loss_and_adam (1e-4)"""
    net, args, vocab, sd, (frames, regions, caps, lens) = build()
    orc = DecayOracle(args, vocab, sd, LR, WD, True, ndim_filter, D, True)
    tr = dlsg_amd.Trainer(net, **OPTS)
    for step in range(2):
        want_loss = orc.step(frames, regions, caps, lens)
        loss = tr.step(frames.to(DEV), regions.to(DEV), caps.to(DEV), lens, 1.0)
        flat, ema = net._flat.cpu(), tr.ema.cpu()
        ew, ee = arena_error(net, flat, dict(orc.model.named_parameters())), arena_error(net, ema, orc.ema)
        print('step %d: loss %.9g oracle %.9g; weights %.3g, ema %.3g (bound 1e-4)' % (step + 1, float(loss), float(want_loss), ew, ee))
        assert abs(float(loss) - float(want_loss)) <= 1e-4
        check_weights(net, orc, 1e-4)
        assert ew <= 1e-4 and ee <= 1e-4
    for k, p in net.named_parameters():                  # an unused parameter keeps its bits
        if k in net.unused_parameters:
            assert torch.equal(bits(p.detach().cpu()), bits(sd[k]))


def test_captured_step_makes_no_host_synchronisation():
    tr, _ = captured_run()
    net, args, vocab, sd, (frames, regions, caps, lens) = build()
    f, r, c, ln = frames.to(DEV), regions.to(DEV), caps.to(DEV), lens.to(DEV)
    every, tr.check_every = tr.check_every, 0
    before = tr.model._flat.clone(), tr.ema.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        tr.step(f, r, c, ln, 1.0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
        tr.check_every = every
    torch.cuda.synchronize()
    assert len(tr._graphs) == 1 and not torch.equal(before[0], tr.model._flat) and not torch.equal(before[1], tr.ema)


def test_the_update_stays_inside_the_one_graph_with_rccl_collectives():
    _, captured = captured_run()
    tr, got = two_steps(use_graphs=True, comm='rccl', max_grad_norm=0.5, force_collectives=True, **OPTS)
    try:
        info = tr.collectives_info()
        assert info['graph_replays_per_step'] == 1 and info['where'] == "inside the step's hipGraph", info
        assert tr._adam_in_graph and tr._rccl is not None
        # one rank: the all-reduce is the identity, the step that of the trainer without collectives
        for a, b in zip(got, captured):
            for x, y in zip(a, b):
                assert torch.equal(bits(x), bits(y))
    finally:
        tr.close()


def test_a_beam_graph_captured_before_averaged_decodes_with_the_average_inside():
    net, args, vocab, sd, (frames, regions, caps, lens) = build()
    f, r = frames.to(DEV), regions.to(DEV)
    tr = dlsg_amd.Trainer(net, lr=1e-2, ema_decay=0.5)
    opts = dict(beam_size=3, length_penalty=0.7)
    graph = dlsg_amd.NBestBeamGraph(net, f, r, **opts)
    for _ in range(2):
        tr.step(f, r, caps.to(DEV), lens, 1.0)
    raw = [x.clone() for x in graph(f, r)]
    twin = copy.deepcopy(net)
    twin.load_state_dict(tr.ema_state_dict())
    want = twin.beam_search(f, r, **opts)
    with tr.averaged():
        got = [x.clone() for x in graph(f, r)]
        with pytest.raises(RuntimeError):
            tr.step(f, r, caps.to(DEV), lens, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0])                  # the ids of the averaged model
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    back = [x.clone() for x in graph(f, r)]
    assert all(torch.equal(a, b) for a, b in zip(back, raw))
    assert not all(torch.equal(a, b) for a, b in zip(raw, got))          # (scores, if not ids: the two models differ)


def test_one_scst_step_with_ema_decay_moves_the_average():
    from dlsg_amd import scoring as S
    from test_gpu_cider_device import gpu_net, scst_corpus
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(train=True)
    reward = S.CiderD(scst_corpus(vocab)).to_device(vocab)
    tr = dlsg_amd.SCSTTrainer(net, reward, n_samples=4, lr=1e-3, check_every=0, weight_decay=0.1, decay_filter=ndim_filter, ema_decay=0.9)
    start = net._flat.clone()
    assert torch.equal(tr.trainer.ema, start)
    random.seed(1)
    tr.step(frames, regions, ['0', '1', '2'])
    torch.cuda.synchronize()
    ema = tr.trainer.ema
    assert not torch.equal(ema, start) and not torch.equal(ema, net._flat) and bool(torch.isfinite(ema).all())

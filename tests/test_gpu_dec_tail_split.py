"""GPU (-m gpu): dec_tail_fwd with the vocabulary scan of a sampled step split over several workgroups per row
(include/dlsg.h, dlsg_dec_tail_args.s_ws / s_split).  Every case runs a forced split and the unsplit launch (s_split = 1) on
the same inputs and asks for the same bits in all seven outputs: c, hd, gates, dout, st_l, s_ids, s_we.  All launches of this
module go through the one workspace HipOps keeps for the device, so a counter a launch left behind would show in the next."""
import pytest
import torch

pytestmark = pytest.mark.gpu

OUTS = ['c', 'hd', 'gates', 'dout', 'stl', 'ids', 'we']
SENT_ID, SENT_WE = 3, 7.0


@pytest.fixture(scope='module')
def hip():
    from dlsg_amd.hip import HipOps
    return HipOps()


def inputs(seed, B, D, V, Wd, nslab=2):
    """CPU tensors of one launch; ids / we hold a sentinel pattern"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(slabs=r(nslab, B, 4 * D), bi=r(4 * D), bh=r(4 * D), cp=r(B, D), gl=r(D), bl=r(D), W=r(V, D), b=r(V), E=r(V, Wd),
                c=torch.zeros(B, D), hd=torch.zeros(B, D), gates=torch.zeros(B, 4 * D), dout=torch.zeros(B, D), stl=torch.zeros(B, 2),
                ids=torch.full((B,), SENT_ID, dtype=torch.int64), we=torch.full((B, Wd + 4), SENT_WE))


def launch(hip, t, split, coin=0, p=0.3, alias=False):
    """one launch on tensors `t` (device); the outputs it wrote"""
    Wd = t['E'].shape[1]
    coins = torch.tensor([1, coin, 1], dtype=torch.int32, device='cuda')
    hip.dec_tail_split = split
    try:
        hip.dec_tail_fwd(t['slabs'], t['bi'], t['bh'], t['c'] if alias else t['cp'], t['c'], t['hd'], t['gates'], (t['gl'], t['bl']),
                         t['dout'], t['stl'], p, 31, seed=5,
                         sample=dict(coins=coins, t=1, W=t['W'], b=t['b'], E=t['E'], ids_out=t['ids'], we_out=t['we'][:, :Wd], p=0.25,
                                     site=9, row0=2 * t['c'].shape[0]))
    finally:
        hip.dec_tail_split = 0
    torch.cuda.synchronize()
    ws = hip._tail_ws[t['c'].device].view(-1, hip_words())
    assert int(ws[:, 2 * max_split()].abs().sum()) == 0, 'a ticket counter was left behind'
    return {k: t[k].clone() for k in OUTS}


def hip_words():
    from dlsg_amd import abi
    return abi.defines['DLSG_DEC_TAIL_WS_WORDS']


def max_split():
    from dlsg_amd import abi
    return abi.defines['DLSG_DEC_TAIL_MAX_SPLIT']


def fresh(base):
    return {k: v.clone().cuda() for k, v in base.items()}


def same(got, want, what):
    for k in OUTS:
        a, b = got[k], want[k]
        if a.dtype == torch.float32:            # bit patterns: NaNs compare as well, and -0 is not +0
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), (what, k)


def check_ids_fp64(out, base, what):
    """ids against an fp64 argmax of the projection, on the rows whose best two logits are more than 1e-4 of their magnitude
    apart (closer ones may order either way in fp32); at most a tenth of the rows may be left out"""
    lg = out['dout'].cpu().double() @ base['W'].double().t() + base['b'].double()
    top = lg.topk(2, dim=1)
    clear = (top.values[:, 0] - top.values[:, 1]) > 1e-4 * top.values[:, 0].abs()
    assert int((~clear).sum()) * 10 <= lg.shape[0], (what, 'too many near-ties for this seed')
    assert torch.equal(out['ids'].cpu()[clear], top.indices[:, 0][clear]), what


def test_bench_shape(hip):
    """B = 64, D = 1024, V = 1000, Wd = 300, four gate slabs, dropout on, split 4"""
    base = inputs(11, 64, 1024, 1000, 300, nslab=4)
    want = launch(hip, fresh(base), 1)
    got = launch(hip, fresh(base), 4)
    same(got, want, 'bench shape')
    check_ids_fp64(got, base, 'bench shape')
    assert (got['we'][:, 300:] == SENT_WE).all()


def test_more_parts_than_vocabulary_rows(hip):
    base = inputs(12, 3, 64, 5, 12)
    same(launch(hip, fresh(base), 8), launch(hip, fresh(base), 1), 'V = 5, split 8')


@pytest.mark.parametrize('split', [2, 3])
def test_scalar_path_unequal_shares(hip, split):
    """D = 130: no 16-byte vectors; V = 67: shares of 33 / 34 and 22 / 22 / 23 rows"""
    base = inputs(13, 5, 130, 67, 33)
    want = launch(hip, fresh(base), 1)
    got = launch(hip, fresh(base), split)
    same(got, want, 'scalar split %d' % split)
    check_ids_fp64(got, base, 'scalar split %d' % split)


@pytest.mark.parametrize('D', [64, 130])
def test_ties_across_parts_take_the_lower_index(hip, D):
    """rows of W and entries of b repeat with period 7, so every logit of a row appears in every part with the same bits: the
    first of the equal maxima wins whatever the split and whichever part arrives last"""
    base = inputs(14, 6, D, 64, 9)
    base['W'] = base['W'][:7].repeat(10, 1)[:64].contiguous()
    base['b'] = base['b'][:7].repeat(10)[:64].contiguous()
    want = launch(hip, fresh(base), 1)
    assert int(want['ids'].max()) < 7
    for split in range(2, max_split() + 1):
        same(launch(hip, fresh(base), split), want, 'ties, split %d' % split)


def test_row_without_a_maximum_gets_word_0(hip):
    base = inputs(15, 4, 64, 50, 8)
    base['slabs'][:, 2] = float('nan')
    want = launch(hip, fresh(base), 1)
    assert int(want['ids'][2]) == 0 and torch.isnan(want['dout'][2]).all()
    for split in (2, 5):
        same(launch(hip, fresh(base), split), want, 'NaN row, split %d' % split)


def test_coin_set_leaves_ids_and_embedding_alone(hip):
    base = inputs(16, 64, 256, 300, 20)
    want_tf = launch(hip, fresh(base), 1, coin=1)
    t = fresh(base)
    got_tf = launch(hip, t, 4, coin=1)
    same(got_tf, want_tf, 'teacher-forced')
    assert (got_tf['ids'] == SENT_ID).all() and (got_tf['we'] == SENT_WE).all()
    # the same tensors, the same workspace, now a sampled step
    same(launch(hip, t, 4), launch(hip, fresh(base), 1), 'sampled after teacher-forced')


def test_workspace_reuse(hip):
    base = inputs(17, 64, 256, 300, 20)
    want = launch(hip, fresh(base), 1)
    for split in (4, 4, 2, 4):                    # two sampled launches in a row, then another split and back
        same(launch(hip, fresh(base), split), want, 'reuse, split %d' % split)
    small = inputs(18, 7, 64, 40, 8)              # other rows and another split on the same workspace
    same(launch(hip, fresh(small), 8), launch(hip, fresh(small), 1), 'reuse, B = 7')
    same(launch(hip, fresh(base), 4), want, 'reuse, back to B = 64')


def test_graph_replay(hip):
    from dlsg_amd import graphs
    base = inputs(11, 64, 1024, 1000, 300, nslab=4)
    want = launch(hip, fresh(base), 1)
    t = fresh(base)
    Wd = 300
    coins = torch.tensor([1, 0, 1], dtype=torch.int32, device='cuda')
    sample = dict(coins=coins, t=1, W=t['W'], b=t['b'], E=t['E'], ids_out=t['ids'], we_out=t['we'][:, :Wd], p=0.25, site=9, row0=128)

    def body():
        hip.dec_tail_fwd(t['slabs'], t['bi'], t['bh'], t['cp'], t['c'], t['hd'], t['gates'], (t['gl'], t['bl']), t['dout'], t['stl'],
                         0.3, 31, seed=5, sample=sample)
    hip.dec_tail_split = 4
    try:
        graph, _ = graphs.capture(t['c'].device, body)
    finally:
        hip.dec_tail_split = 0
    for r in range(3):
        for k in OUTS:
            t[k].fill_(SENT_ID if k == 'ids' else SENT_WE)
        graph.replay()
        torch.cuda.synchronize()
        same({k: t[k] for k in OUTS}, want, 'replay %d' % r)


def test_fallbacks_take_the_unsplit_kernel(hip):
    # c_prev aliased to c: the other parts would read the cell state part 0 overwrites
    base = inputs(19, 8, 64, 40, 8)
    ta, tb = fresh(base), fresh(base)
    ta['c'].copy_(ta['cp']); tb['c'].copy_(tb['cp'])
    same(launch(hip, ta, 4, alias=True), launch(hip, tb, 1, alias=True), 'c_prev is c')
    # the library's choice for more rows than half the compute units
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert hip.lib.dlsg_dec_tail_split(130, cus) == 1 and hip.lib.dlsg_dec_tail_split(64, cus) == min(max_split(), cus // 64)
    base = inputs(20, 130, 64, 40, 8)
    same(launch(hip, fresh(base), 0), launch(hip, fresh(base), 1), 'B = 130, s_split = 0')

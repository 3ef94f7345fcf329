"""GPU (-m gpu): the two sampling steps under exclusions on the MI355X.  The oracle of both kernels is the EXISTING kernel on the
same logits with the words the rule bans for a row at that step set to -inf (`emul_sample_excl.banned_by_tables`, on
`emul_excl.excluded_word`, from the row's history on the CPU): `dlsg_sample_excl_embed` against `dlsg_sample_filter_embed`,
`dlsg_beam_select_gumbel_excl` against `dlsg_beam_select_gumbel`.  Then the keyword through `sample`, `sample_without_replacement`,
their graph classes and an SCST step.  The CPU side is tests/test_sample_excl_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import abi
from dlsg_amd import engine as E
from dlsg_amd.beam import BAD_ENDINGS, Exclusions, exclusions_hit, pack_exclusions
from dlsg_amd.graphs import expand_rows
from dlsg_amd.hip import HipOps
from emul_sample_excl import banned_by_tables, masked
from test_gpu_sample_filter import inputs, run_filter
from test_gpu_scst import gpu_net
from test_sample_excl_host import caption_words, renamed_vocab
from test_scst_host import LengthReward

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS, END, P = 64, 3, 4
INF = float('inf')
LIFT = 40.0                                                        # a word lifted to this logit is drawn unless it is banned


@pytest.fixture(scope='module')
def ops():
    return HipOps()


def run_excl(ops, logits, E_, shared, per_clip, rows_per_clip, t=0, end=-1, tau=1.0, p=0.0, seed=7, row0=0, hist=None, **opts):
    rows = logits.shape[0]
    ids = torch.empty(rows, dtype=torch.int64, device=DEV)
    out = torch.empty(rows, E_.shape[1], device=DEV)
    logp = torch.empty(rows, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lens = torch.full((rows,), 64, dtype=torch.int64, device=DEV)
    ops.sample_excl_embed(logits, E_, ids, out, logp, lens, t, end, temperature=tau, p=p, seed=seed, site=E.SITE_WORD,
                          site_sample=E.SITE_SAMPLE, row0=row0, hist=hist, kept=kept, rows_per_clip=rows_per_clip,
                          excl_shared=None if shared is None else shared.to(DEV), excl_clip=None if per_clip is None else per_clip.to(DEV),
                          **opts)
    return ids, out, logp, lens, kept


def against_masked_parent(ops, x, E_, hist, shared, per_clip, rows_per_clip, t, what, **opts):
    """the step under exclusions on x against dlsg_sample_filter_embed on x with the banned words at -inf: ids, lens, kept and the
    embedded rows equal, logp within 1e-5 where a word is left (the observed maximum is printed) -> (ids, kept, the ban sets)"""
    rows, V = x.shape
    histories = [hist[:t, r].tolist() for r in range(rows)]
    banned = banned_by_tables(histories, [r // rows_per_clip for r in range(rows)], shared, per_clip, rows // rows_per_clip, V)
    hd = hist.to(DEV)
    Ed = E_.to(DEV)
    kw = dict(t=t, p=0.3, seed=99, row0=128, hist=hd, **opts)
    got = run_excl(ops, x.to(DEV), Ed, shared, per_clip, rows_per_clip, **kw)
    lens = torch.full((rows,), 64, dtype=torch.int64, device=DEV)
    want = run_filter(ops, masked(x, banned).to(DEV), Ed, lens=lens, **kw)
    torch.cuda.synchronize()
    got, want = [a.cpu() for a in got], [a.cpu() for a in want]
    some = want[4] > 0
    err = float((got[2][some] - want[2][some]).abs().max()) if bool(some.any()) else 0.0
    print('%s: banned per row %d..%d, kept %d..%d, max |dlogp| against the masked parent %.3g'
          % (what, min(map(len, banned)), max(map(len, banned)), int(got[4].min()), int(got[4].max()), err))
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3]) and torch.equal(got[4], want[4]), what
    assert torch.equal(got[1], want[1]), what
    assert err <= 1e-5, (what, err)
    assert bool((got[0][~some] == 0).all())
    return got[0], got[4], banned


def word_of(r):
    """the word row r's entries end with (distinct per row, inside every vocabulary used here)"""
    return 100 + 7 * r


@functools.lru_cache(maxsize=None)
def step_case(V, t):
    """Logits (64, V) of tests/test_gpu_sample_filter.py with one word per row lifted so that it is drawn unless banned, histories
    (max(t, 1), 64), and two tables that put every kind of entry in front of some row -> (x, E, hist, shared, per_clip, banned rows,
    free rows): rows whose lifted word the tables ban, and rows whose lifted word no entry bans although one looks like it.
      row 0   a one-word entry, and a second entry (last word, the same word): two entries that ban the same word
      row 1   (last word, word): a two-word entry
      row 2   (last three words, word): a four-word entry -- longer than the history while t < 3, then it bans nothing
      row 4   (word, -1, x, y): cut to one word by -1          row 5   (word, id >= V, x): cut to one word by the id
      row 6   (a word that is NOT its last word, word): the context does not match
      row 7   (last word, word) where the word also repeats a bigram of the history: no_repeat_ngram = 2 bans it as well
      row 8   (last word, <end>): a bad ending, <end> lifted        and an absent entry (-1 first)
      clips of 4 rows from row 12 on: clip c bans 500 + c; its row 4c + 2 lifts that word, its row 4c + 3 the next clip's."""
    x, E_ = inputs(V)
    x = x.clone()
    gen = torch.Generator().manual_seed(1000 * V + t)
    hist = torch.randint(4, 100, (max(t, 1), ROWS), generator=gen)          # (below every word_of)
    if t >= 3:
        hist[0, 7] = hist[t - 1, 7]                                        # row 7: its last word stood at 0, before hist[1, 7]
    last = lambda r, n: hist[t - n:t, r].tolist()                          # noqa: E731
    pad = lambda e: e + [-1] * (P - len(e))                                # noqa: E731
    lifted = {r: word_of(r) for r in (0, 1, 2, 4, 5, 6)}
    shared = [pad([word_of(0)]), pad([word_of(4), -1, 9, 10]), pad([word_of(5), V + 5, 11]), pad([-1, 12, 13, 14])]
    banned_rows, free_rows = [0, 4, 5], []
    if t >= 1:
        shared += [pad(last(0, 1) + [word_of(0)]), pad(last(1, 1) + [word_of(1)]), pad([int(hist[t - 1, 6]) + 1, word_of(6)]),
                   pad(last(8, 1) + [END])]
        lifted[8] = END
        banned_rows += [1, 8]
        free_rows += [6]
    shared.append(last(2, 3) + [word_of(2)] if t >= 3 else [6, 7, 8, word_of(2)])
    (banned_rows if t >= 3 else free_rows).append(2)
    if t >= 3:
        shared.append(pad(last(7, 1) + [int(hist[1, 7])]))
        lifted[7] = int(hist[1, 7])
        banned_rows.append(7)
    clips = ROWS // 4
    per_clip = torch.full((clips, 2, P), -1, dtype=torch.int64)
    per_clip[:, 0, 0] = 500 + torch.arange(clips)
    for c in range(3, clips):
        lifted[4 * c + 2] = 500 + c
        lifted[4 * c + 3] = 500 + (c + 1) % clips
        banned_rows.append(4 * c + 2)
        free_rows.append(4 * c + 3)
        if t >= 1:
            per_clip[c, 1, :2] = torch.tensor([int(hist[t - 1, 4 * c]), word_of(4 * c)])
    for r, w in lifted.items():
        x[r, w] = LIFT
    return x, E_, hist, torch.tensor(shared), per_clip, tuple(banned_rows), tuple(free_rows), tuple(sorted(lifted.items()))


CONTROLS = [dict(), dict(top_k=50, top_p=0.9), dict(no_repeat_ngram=2), dict(min_len=64), dict(top_k=50, top_p=0.9, no_repeat_ngram=2, min_len=2)]


@pytest.mark.parametrize('V', [1000, 10000])
@pytest.mark.parametrize('t', [0, 1, 3, 63])
def test_step_equals_the_filtered_step_on_masked_logits(ops, V, t):
    x, E_, hist, shared, per_clip, banned_rows, free_rows, lifted = step_case(V, t)
    lifted = dict(lifted)
    for tau in (1.0, 0.7, 0.0):
        for opts in CONTROLS:
            ids, kept, banned = against_masked_parent(ops, x, E_, hist, shared, per_clip, 4, t, 'V %d t %d tau %g %s' % (V, t, tau, opts),
                                                      end=END, tau=tau, **opts)
            for r in banned_rows:
                assert lifted[r] in banned[r] and int(ids[r]) != lifted[r], (r, tau, opts)
            for r in free_rows:
                if not (lifted[r] == END and opts.get('min_len', 0) > t):
                    assert lifted[r] not in banned[r] and int(ids[r]) == lifted[r], (r, tau, opts)
            if not opts:
                assert torch.equal(kept.long(), torch.tensor([V - len(b) for b in banned]))
    # vacuity guard: without the tables every lifted word is drawn
    plain = run_filter(ops, x.to(DEV), E_.to(DEV), t=t, end=END, p=0.3, seed=99, row0=128, hist=hist.to(DEV), min_len=0)[0].cpu()
    assert all(int(plain[r]) == w for r, w in lifted.items())


def test_two_entries_and_a_repeated_bigram_ban_one_word(ops):
    x, E_, hist, shared, per_clip, _, _, _ = step_case(1000, 3)
    ids, kept, banned = against_masked_parent(ops, x, E_, hist, shared, per_clip, 4, 3, 'no_repeat_ngram 2 beside the entries', end=END,
                                              no_repeat_ngram=2)
    # row 0: the word stands twice in the kernel's list and is counted out once; row 7: banned by the entry and by the bigram rule
    assert int(kept[0]) == 1000 - len(banned[0]) and int(kept[7]) == 1000 - len(banned[7])
    assert word_of(0) in banned[0] and int(hist[1, 7]) in banned[7]


def test_a_row_with_every_word_banned_takes_word_zero(ops):
    V, rows = 37, 8
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(37)) * 3
    E_ = torch.randn(V, 16, generator=torch.Generator().manual_seed(38))
    shared = torch.tensor([[w, -1] for w in range(5)])
    per_clip = torch.full((4, 32, 2), -1, dtype=torch.int64)
    per_clip[1, :, 0] = torch.arange(5, 37)
    hist = torch.randint(4, V, (2, rows), generator=torch.Generator().manual_seed(39))
    for tau in (1.0, 0.0):
        ids, kept, banned = against_masked_parent(ops, x, E_, hist, shared, per_clip, 2, 2, 'V 37, clip 1 banned whole, tau %g' % tau,
                                                  end=END, tau=tau)
        assert kept.tolist() == [32, 32, 0, 0, 32, 32, 32, 32] and ids[2:4].tolist() == [0, 0]
        assert bool((ids[[0, 1, 4, 5, 6, 7]] >= 5).all())


def test_full_tables_at_the_largest_vocabulary(ops):
    """V = 32768, NS = 64, NC = 32, P = 4: the row's 128 KB beside the tables and the long list, one launch"""
    V, t, rows = 32768, 3, 8
    gen = torch.Generator().manual_seed(32768)
    x = torch.randn(rows, V, generator=gen) * 3
    E_ = torch.randn(V, 8, generator=gen)
    hist = torch.randint(4, V, (t, rows), generator=gen)
    best = x.topk(40)[1]
    shared = torch.full((64, P), -1, dtype=torch.int64)
    per_clip = torch.full((rows // 2, 32, P), -1, dtype=torch.int64)
    for a in range(64):                                              # the best words of row a % 8, behind 0 .. 3 words of its history
        r, n = a % rows, a % P
        shared[a, :n] = hist[t - n:t, r] if n else hist[:0, r]
        shared[a, n] = best[r, a // rows]
    for c in range(rows // 2):
        for a in range(32):
            r, n = 2 * c + a % 2, (a // 2) % P
            per_clip[c, a, :n] = hist[t - n:t, r] if n else hist[:0, r]
            per_clip[c, a, n] = best[r, 8 + a // 2]
    ids, kept, banned = against_masked_parent(ops, x, E_, hist, shared, per_clip, 2, t, 'V 32768 with full tables', end=END, top_k=50,
                                              top_p=0.9)
    assert min(map(len, banned)) >= 20
    ids, kept, banned = against_masked_parent(ops, x, E_, hist, shared, per_clip, 2, t, 'V 32768 with full tables, bans only', end=END)
    assert torch.equal(kept.long(), torch.tensor([V - len(b) for b in banned]))


def test_two_launches_give_equal_bits_and_no_table_gives_the_filtered_step(ops):
    x, E_, hist, shared, per_clip, _, _, _ = step_case(1000, 3)
    kw = dict(t=3, end=END, tau=0.7, p=0.3, seed=5, row0=64, hist=hist.to(DEV), top_k=50, top_p=0.9, no_repeat_ngram=2)
    a = run_excl(ops, x.to(DEV), E_.to(DEV), shared, per_clip, 4, **kw)
    b = run_excl(ops, x.to(DEV), E_.to(DEV), shared, per_clip, 4, **kw)
    c = run_excl(ops, x.to(DEV), E_.to(DEV), None, None, 1, **kw)
    lens = torch.full((ROWS,), 64, dtype=torch.int64, device=DEV)
    d = run_filter(ops, x.to(DEV), E_.to(DEV), lens=lens, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert all(torch.equal(u, v) for u, v in zip(c, d)) and not torch.equal(a[0], c[0])


def test_the_step_refuses_what_it_cannot_run(ops):
    """argument checks of the entry point: DLSG_EINVAL, nothing is launched"""
    EINVAL = abi.defines['DLSG_EINVAL']
    rows, V = 8, 50
    x = torch.randn(rows, V, device=DEV)
    E_ = torch.randn(V, 8, device=DEV)
    ids = torch.zeros(rows, dtype=torch.int64, device=DEV)
    out, logp = torch.zeros(rows, 8, device=DEV), torch.zeros(rows, device=DEV)
    lens = torch.full((rows,), 26, dtype=torch.int64, device=DEV)
    hist = torch.zeros(4, rows, dtype=torch.int64, device=DEV)
    shared = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    clip = torch.zeros(4, 1, 2, dtype=torch.int64, device=DEV)
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())       # noqa: E731

    def call(t=2, top_k=0, top_p=1.0, min_len=0, g=0, hist=hist, stride=rows, sh=shared, NS=2, cl=clip, NC=1, P_=2, rpc=2, tau=1.0):
        args = ops._sample_args(x, E_, ids, out, logp, lens, t, END, tau, 0.0, 1, E.SITE_WORD, E.SITE_SAMPLE, 0)
        return ops.lib.dlsg_sample_excl_embed(*args, top_k, C.c_float(top_p), min_len, g, ptr(hist), C.c_int64(stride), None, ptr(sh), NS,
                                              ptr(cl), NC, P_, rpc, ops._stream())
    assert call() == 0
    for bad in (dict(NS=-1), dict(NS=65), dict(NC=-1), dict(NC=33), dict(sh=None), dict(cl=None), dict(P_=0), dict(P_=5),
                dict(rpc=0), dict(rpc=-2), dict(rpc=3), dict(hist=None), dict(stride=rows - 1), dict(t=-1), dict(t=64), dict(top_k=-1),
                dict(top_p=0.0), dict(top_p=1.5), dict(min_len=-1), dict(g=-1), dict(tau=-1.0)):
        assert call(**bad) == EINVAL, bad
    assert call(hist=None, t=0) == 0                                   # no history is read at step 0
    assert call(hist=None, sh=None, NS=0, cl=None, NC=0, P_=9) == 0    # no entry, no control: nothing reads it
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the stochastic step
def gumbel_case(B, K, V, t, L=26, seed=0):
    """finite logits, ~40 % ended beams behind step 0, histories of random words; tables that match some beams and not others:
    shared -- the best word of row 1 at every step, (last word of row 2, its best word), (last word, <end>) of an ended row, an
    entry longer than the history; per clip -- (last two words of the clip's row 1, its second-best word) and (last word of its
    last row, that row's best word), so that the clips ban different words"""
    R = B * K
    gen = torch.Generator().manual_seed(seed + 100 * t + K)
    lg = torch.randn(R, V, generator=gen) * 3.0
    hist = torch.full((R, L), END, dtype=torch.int64)
    hist[:, :t] = torch.randint(4, V, (R, t), generator=gen)
    last = hist[:, t - 1].clone() if t else torch.full((R,), 1, dtype=torch.int64)
    if t:
        last[torch.rand(R, generator=gen) < 0.4] = END
        last[[1, 2, K + 1, R - 1]] = hist[[1, 2, K + 1, R - 1], t - 1]
        last[3] = END
    lp = -torch.rand(R, generator=gen) * 5
    u = torch.rand(R, generator=gen, dtype=torch.float64).clamp_(1e-9, 1 - 1e-9)
    best = lg.topk(2)[1]
    pad = lambda e: e + [-1] * (P - len(e))                                # noqa: E731
    tail = lambda r, n: hist[r, max(t - n, 0):t].tolist()                  # noqa: E731
    shared = torch.tensor([pad([int(best[1, 0])]), pad(tail(2, 1) + [int(best[2, 0])]), pad(tail(3, 1) + [END]),
                           [4, 5, 6, 7] if t < 3 else pad([int(hist[0, t - 1]) + 1, int(best[0, 0])])])
    per_clip = torch.tensor([[pad(tail(b * K + 1, 2) + [int(best[b * K + 1, 1])]), pad(tail(b * K + K - 1, 1) + [int(best[b * K + K - 1, 0])])]
                             for b in range(B)])
    c = dict(lg=lg, last=last, lp=lp, gin=lp.double() - torch.log(-torch.log(u)), hist=hist, hout=torch.zeros(R, L, dtype=torch.int64),
             pred=torch.zeros(R, dtype=torch.int64), nlp=torch.zeros(R), back=torch.zeros(R, dtype=torch.int64),
             rows=torch.zeros(R, dtype=torch.int64), gout=torch.zeros(R, dtype=torch.float64))
    return c, shared, per_clip


@pytest.mark.parametrize('K', [4, 8])
@pytest.mark.parametrize('t', [0, 1, 5])
def test_gumbel_step_equals_the_step_on_masked_logits(ops, K, t):
    B, V = 3, 1000
    c, shared, per_clip = gumbel_case(B, K, V, t)
    banned = banned_by_tables([c['hist'][r, :t].tolist() for r in range(B * K)], [r // K for r in range(B * K)], shared, per_clip, B, V)
    assert any(banned) and int(c['lg'].topk(1)[1][1]) in banned[1]
    worst = 0.0
    for g, m, temp in ((0, 0, 1.0), (2, t + 1, 0.7)):
        runs = []
        for lg, tables in ((c['lg'], (shared.to(DEV), per_clip.to(DEV))), (masked(c['lg'], banned), None), (c['lg'], None)):
            d = {k: v.to(DEV) for k, v in c.items()}
            args = (lg.to(DEV), d['last'], d['lp'], d['pred'], d['nlp'], d['back'], d['rows'], K, END, d['hist'], d['hout'], t, d['gin'],
                    d['gout'])
            kw = dict(temperature=temp, seed=0x5B5, site_sample=E.SITE_SAMPLE, no_repeat_ngram=g, min_len=m)
            if tables is None:
                ops.beam_select_gumbel(*args, **kw)
            else:
                ops.beam_select_gumbel_excl(*args, *tables, **kw)
            torch.cuda.synchronize()
            runs.append({k: d[k].cpu() for k in ('pred', 'back', 'rows', 'hout', 'nlp', 'gout')})
        got, want, plain = runs
        for o in ('pred', 'back', 'rows', 'hout'):
            assert torch.equal(got[o], want[o]), (K, t, g, o)
        for o in ('nlp', 'gout'):
            fin = want[o] > -INF
            assert torch.equal(got[o][~fin], want[o][~fin]), (K, t, g, o)
            err = float((got[o][fin].double() - want[o][fin].double()).abs().max())
            worst = max(worst, err)
            assert err <= 1e-5, (K, t, g, o, err)
        assert not torch.equal(got['pred'], plain['pred']) or not torch.equal(got['nlp'], plain['nlp'])     # (the tables bite)
        if t:                                                          # an ended beam is untouched: <end> at its own values
            for o in range(B * K):
                par = int(got['rows'][o])
                if int(c['last'][par]) == END:
                    assert int(got['pred'][o]) == END and float(got['nlp'][o]) == float(c['lp'][par])
                    assert float(got['gout'][o]) == float(c['gin'][par])
    print('K %d t %d: largest |new_lp, G_out - the masked parent| %.3g' % (K, t, worst))


def test_gumbel_step_refuses_its_tables(ops):
    c, shared, per_clip = gumbel_case(3, 4, 50, 1)
    d = {k: v.to(DEV) for k, v in c.items()}
    a, hist = ops._hist_step(12, 50, d['last'], d['lp'], d['pred'], d['nlp'], d['back'], d['rows'], 4, END, d['hist'], d['hout'], 1, 0, 0,
                             None, d['lg'])
    sh, pc = shared.to(DEV), per_clip.to(DEV)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())       # noqa: E731

    def call(sh=sh, NS=4, pc=pc, NC=2, P_=P, temp=1.0, gout=d['gout']):
        return ops.lib.dlsg_beam_select_gumbel_excl(C.byref(a), *hist, C.c_float(temp), C.c_uint64(1), None, C.c_uint32(E.SITE_SAMPLE),
                                                    ptr(d['gin']), ptr(gout), ptr(sh), NS, ptr(pc), NC, P_, ops._stream())
    assert call() == 0
    for bad in (dict(NS=65), dict(NS=-1), dict(NC=33), dict(sh=None), dict(pc=None), dict(P_=0), dict(P_=5), dict(temp=0.0),
                dict(gout=d['gin'])):
        assert call(**bad) == abi.defines['DLSG_EINVAL'], bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- through the model
CLIPS, N = 4, 3


def model():
    net, sd, args, vocab, frames, regions, _, _ = gpu_net(n_batch=CLIPS)
    net.decoder.word_restore.bias.data[vocab('<end>')] += 2.0          # captions that end before max_words
    return net, vocab, frames, regions


def exclusions_from(ids, lens, vocab, n):
    """from a draw (B*n, L): per clip the first word of one of its rows; shared, a bigram behind the first word of the longest
    caption and the ending (last word, <end>) of the first caption that ends behind a word; the special tokens, which cannot be
    excluded, are passed over -> (Exclusions, another with the same shapes)"""
    caps = caption_words(ids.cpu(), lens.cpu())
    B = len(caps) // n
    long = max(caps, key=len)
    grams = [tuple(long[i:i + 2]) for i in range(1, len(long) - 1) if min(long[i:i + 2]) >= 4]
    assert len(grams) >= 2
    ending = next(c for c in caps if 2 <= len(c) < ids.shape[1] and c[-2] >= 4 and c[-1] == vocab('<end>'))[-2]
    firsts = [[c[0] for c in caps[b * n:b * n + n] if c[0] >= 4][:1] for b in range(B)]
    ex = pack_exclusions(vocab, phrases=[grams[0]], bad_endings=[vocab.idx2word[ending]], per_clip=[[(w,) for w in f] for f in firsts],
                         device=DEV)
    other = pack_exclusions(vocab, phrases=[grams[-1]], bad_endings=[vocab.idx2word[grams[0][0]]], device=DEV)
    assert other.shared.shape == ex.shared.shape and ex.per_clip.shape[1] == 1
    return ex, other


@pytest.mark.parametrize('share', [False, True])
def test_sample_under_exclusions_and_graph_replay(share):
    net, vocab, frames, regions = model()
    L = net.decoder.max_words
    kw = dict(n=N, share_encoder=share)
    plain = [a.cpu() for a in net.sample(frames, regions, seed=21, **kw)]
    ex, other = exclusions_from(plain[0], plain[2], vocab, N)
    cpu_ex = Exclusions(*[a.cpu() for a in ex])
    hit0 = exclusions_hit(plain[0].view(CLIPS, N, L), plain[2].view(CLIPS, N), cpu_ex).view(-1)
    assert bool((hit0.view(CLIPS, N) > 0).any(1).all())
    got = net.sample(frames, regions, seed=21, exclude=ex, return_kept=True, **kw)
    torch.cuda.synchronize()
    ids, logp, lens, kept = [a.cpu() for a in got]
    assert int(exclusions_hit(ids.view(CLIPS, N, L), lens.view(CLIPS, N), cpu_ex).sum()) == 0
    assert bool(torch.isfinite(logp).all()) and int(kept.max()) <= len(vocab) - 1
    free = [r for r in range(CLIPS * N) if int(hit0[r]) == 0]
    assert free
    for r in free:                                                     # a row whose draw met no entry keeps its words
        n = int(plain[2][r])
        assert ids[r, :n].tolist() == plain[0][r, :n].tolist() and int(lens[r]) == n, r
    sg = dlsg_amd.SampleGraph(net, frames, regions, temperature=1.0, exclude=ex, return_kept=True, **kw)
    for s in (21, 5):
        rep = [a.clone() for a in sg(frames, regions, s)]
        want = net.sample(frames, regions, seed=s, exclude=ex, return_kept=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(rep, want)), s
    sg.exclude.shared.copy_(other.shared)
    rep = [a.clone() for a in sg(frames, regions, 21)]
    want = net.sample(frames, regions, seed=21, exclude=Exclusions(other.shared, ex.per_clip), return_kept=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(rep, want)) and not torch.equal(rep[0], got[0])


def test_sample_without_replacement_under_exclusions_and_graph_replay():
    net, vocab, frames, regions = model()
    L = net.decoder.max_words
    plain = [a.cpu() for a in net.sample_without_replacement(frames, regions, n=N, seed=21)]
    ex, other = exclusions_from(plain[0].view(-1, L), plain[2].view(-1), vocab, N)
    cpu_ex = Exclusions(*[a.cpu() for a in ex])
    assert bool((exclusions_hit(plain[0], plain[2], cpu_ex) > 0).any(1).all())
    got = net.sample_without_replacement(frames, regions, n=N, seed=21, exclude=ex)
    ids, logp, lens = [a.cpu() for a in got]
    finite = logp > -INF
    assert bool(finite[:, 0].all()) and int(exclusions_hit(ids, lens, cpu_ex)[finite].sum()) == 0
    graph = dlsg_amd.StochasticBeamGraph(net, frames, regions, n=N, exclude=ex)
    for s in (21, 5):
        rep = [a.clone() for a in graph(frames, regions, s)]
        want = net.sample_without_replacement(frames, regions, n=N, seed=s, exclude=ex)
        assert all(torch.equal(a, b) for a, b in zip(rep, want)), s
    graph.exclude.shared.copy_(other.shared)
    rep = [a.clone() for a in graph(frames, regions, 21)]
    want = net.sample_without_replacement(frames, regions, n=N, seed=21, exclude=Exclusions(other.shared, ex.per_clip))
    assert all(torch.equal(a, b) for a, b in zip(rep, want)) and not torch.equal(rep[0], got[0])


@pytest.mark.parametrize('use_graphs', [False, True])
def test_scst_step_under_exclusions_equals_the_hand_composed_step(use_graphs):
    """SCSTTrainer(sample_options=dict(exclude=...), baseline='greedy') against sample(exclude=...), the reward, the greedy rows of
    sample(n=1, temperature=0, exclude=...) in eval mode and Trainer.step with those advantages, on a second model with the same
    weights: sampled words, advantages, loss and gradient equal"""
    vids = [str(b) for b in range(CLIPS)]
    res = []
    for composed in (False, True):
        net, sd, args, vocab, frames, regions, _, _ = gpu_net(n_batch=CLIPS, train=True)
        net.decoder.word_restore.bias.data[vocab('<end>')] += 2.0
        L = net.decoder.max_words
        if not composed:
            probe = [a.cpu() for a in net.sample(frames, regions, n=N, seed=3)]
            stops = [c[-2] for c in caption_words(probe[0], probe[2]) if 2 <= len(c) < L and c[-2] >= 4]
            assert stops
            words = sorted(set(stops))[:3]
        vocab = renamed_vocab(net, words)
        ex = pack_exclusions(vocab, suppress_unk=True, bad_endings=True, device=DEV)
        net.seed_counter = 0
        if not composed:
            tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=N, baseline='greedy', sample_options=dict(exclude=ex), lr=0.0,
                                      use_graphs=use_graphs)
            seen = []
            inner = tr.trainer.step
            tr.trainer.step = lambda *a, **k: seen.append((a[2].clone(), a[3].clone(), k['seq_weights'].clone())) or inner(*a, **k)
            out = tr.step(frames, regions, vids)
            torch.cuda.synchronize()
            assert net.training
            ids, lens, adv = seen[0]
            loss = float(out['loss'])
        else:
            seed = net.next_seed()
            ids, _, lens = net.sample(frames, regions, N, 1.0, seed, exclude=ex)
            net.eval()
            greedy = net.sample(frames, regions, 1, 0.0, 0, exclude=ex)
            net.train()
            host_ids, host_greedy = ids.cpu(), greedy[0].cpu()
            r = LengthReward().scores([v for v in vids for _ in range(N)], [net.decoder.decode_tokens(x) for x in host_ids])
            b = np.repeat(LengthReward().scores(vids, [net.decoder.decode_tokens(x) for x in host_greedy]), N)
            adv = torch.from_numpy((r - b).astype(np.float32)).to(DEV)
            trainer = dlsg_amd.Trainer(net, lr=0.0, use_graphs=use_graphs)
            loss = float(trainer.step(expand_rows(frames, N), expand_rows(regions, N), ids, lens, 1.0, max_len=L, seed=seed, seq_weights=adv))
            torch.cuda.synchronize()
            cpu_ex = Exclusions(ex.shared.cpu(), None)
            bad = {vocab(w) for w in BAD_ENDINGS if w in vocab.word2idx}
            assert len(bad) == len(words)
            for rows, ln in ((host_ids, lens.cpu()), (host_greedy, greedy[2].cpu())):
                assert int(exclusions_hit(rows, ln, cpu_ex).sum()) == 0
                for cap in caption_words(rows, ln):
                    assert vocab('<unk>') not in cap and not (len(cap) >= 2 and cap[-1] == vocab('<end>') and cap[-2] in bad)
        res.append((ids.cpu(), lens.cpu(), adv.cpu(), loss, net._gflat.clone().cpu()))
    (i0, l0, a0, loss0, g0), (i1, l1, a1, loss1, g1) = res
    assert torch.equal(i0, i1) and torch.equal(l0, l1) and torch.equal(a0, a1)
    assert loss0 == loss1 and torch.equal(g0, g1) and float(a0.abs().max()) > 0

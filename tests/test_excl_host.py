"""CPU: beam search under exclusions -- the emulated step (tests/emul_excl.py) against an independent restatement on lists, on the
step cases that tests/test_gpu_excl.py runs on the kernel, and that those cases leave few clips out as near-ties; `pack_exclusions`
and its refusals; `exclusions_hit`; and `beam_search(exclude=...)` of a model, an ensemble, the graph classes and `gather_results`
through the emulated ops on a small host model, against a restated whole search and the properties an exclusion owes its caller."""
import collections
import functools
import itertools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import graphs
from dlsg_amd import scoring as S
from dlsg_amd.beam import BAD_ENDINGS, Exclusions, check_exclusions, exclusions_hit, pack_exclusions
from dlsg_amd.hip import normalised_weights
from emul_beam import banned_classes
from emul_excl import NO_CLASS, ExclEmul, excluded_word
from test_beam_nbest_host import close, oracle_stepper, reference_rank, synth_pair, words_of
from test_constrained_host import GAP, build_cons_case, close_lp
from test_sbs_host import END, fresh

INF = float('inf')
DIMS = [(1, 1, 5), (3, 3, 70), (7, 6, 1000), (2, 8, 32768)]
TABLES = ('empty', 'one', 'mixed', 'full')
MEMBERS = [(1, 0), (3, 0), (3, 1)]                                    # (M, mode), taken in turn over the cases (1: either mode is x - lse)
WEIGHTS = {1: [1.0], 3: [0.5, 0.3, 0.2]}
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt')
P_MAX = 4


# ---------------------------------------------------------------------------------------------- step cases (shared with the GPU tests)
def step_keys(dims_list=DIMS, Ls=(26, 64)):
    """(dims, L, g, t, min_len, tables, M, mode) of every step case.  The 32768-word rows (2 MB of logits per member and case) come
    with L = 64 and the two tables that hold more than one entry only."""
    keys = []
    for dims in dims_list:
        big = dims[2] > 10000
        for L in Ls[1:] if big else Ls:
            for g in (0, 2):
                for t in (0, 1, 2, 3, L - 1):
                    for m in (0, t + 1):
                        for tab in TABLES[2:] if big else TABLES:
                            keys.append((dims, L, g, t, m, tab) + MEMBERS[len(keys) % len(MEMBERS)])
    return keys


def build_tables(c, dims, t, tab, gen):
    """The two exclusion tables of a step case -> (shared (NS, P) or None, per_clip (B, NC, P) or None).
      empty  no table at all;
      one    NS = NC = 1: the best class of the last clip's first row for every clip, and per clip a two-word entry whose context
             is the last word of the clip's first row (a one-word entry at step 0);
      full   NS = 64 and NC = 32 one-word entries (P = 2, the second word -1) from a pool of at most 20 words that holds the best
             classes of the clip's rows: every entry matches at once, so a row's list takes all 96 -- with V = 5 the pool is the
             whole vocabulary and every finite word of a row is banned;
      mixed  P = 4.  Shared: a one-word entry; an entry of four words (its context is longer than the history while t < 3); an entry
             cut to one word by an id >= V in the middle; an absent entry (-1 first); the last clip's first row's last two words
             before its second-best class.  Per clip, for each of its first three rows r: (last word, best class) -- a bigram that
             bites --; (last two words, second-best class); (first word of the history, third-best class), whose context stands
             earlier in the row but, where the first word differs from the last, not at its end; (last word, <end>), a bad ending;
             and (last word, an id >= V, best class), cut to the last word alone."""
    B, k, V = dims
    if tab == 'empty':
        return None, None
    x = c['lg'][:, 1:V + 1]
    best = torch.where(torch.isnan(x), torch.full((), -INF), x).topk(min(3, V))[1].tolist()
    hist = c['hist'].tolist()
    last_clip = (B - 1) * k

    def words(r, n):
        return hist[r][t - n:t] if n <= t else hist[r][:t]
    if tab == 'one':
        shared = torch.tensor([[best[last_clip][0], -1]])
        per_clip = torch.tensor([[words(b * k, 1) + [best[b * k][0]] + [-1] * (1 - min(t, 1))] for b in range(B)])
        return shared, per_clip
    if tab == 'full':
        def pool(rows):
            ws = [w for r in rows for w in best[r]] + [int(v) for v in torch.randint(0, V, (20,), generator=gen)]
            ws = list(range(V)) if V <= 20 else list(dict.fromkeys(ws))[:20]
            return [ws[i % len(ws)] for i in range(64)]
        shared = torch.tensor([[w, -1] for w in pool(range(last_clip, last_clip + k))])
        per_clip = torch.tensor([[[w, -1] for w in pool(range(b * k, b * k + k))[:32]] for b in range(B)])
        return shared, per_clip
    pad = lambda e: e + [-1] * (P_MAX - len(e))                        # noqa: E731
    r0 = last_clip
    rnd = [int(v) for v in torch.randint(min(3, V - 1), V, (8,), generator=gen)]
    shared = [pad([best[r0][-1]]), (words(r0, 3) + rnd[:4])[:4], pad([rnd[4], V + 5, rnd[5]]), pad([-1, rnd[6], rnd[7]]),
              pad(words(r0, 2) + [best[r0][min(1, len(best[r0]) - 1)]])]
    per_clip = []
    for b in range(B):
        own = []
        for r in range(b * k, b * k + min(k, 3)):
            own += [pad(words(r, 1) + [best[r][0]]), pad(words(r, 2) + [best[r][min(1, len(best[r]) - 1)]]),
                    pad(hist[r][:min(t, 1)] + [best[r][-1]]), pad(words(r, 1) + [END]) if t else pad([-1]),
                    pad(words(r, 1) + [V + 9, best[r][0]]) if t else pad([V + 9, best[r][0]])]
        per_clip.append(own + [pad([-1])] * (15 - len(own)))
    return torch.tensor(shared), torch.tensor(per_clip)


def build_excl_case(key, seed):
    """`build_cons_case` of tests/test_constrained_host.py without constraints (its logits behind a strided view, -inf entries, a NaN in
    the last row of every odd clip but the last, ~40 % ended rows, clip 0 ended altogether, histories whose last g - 1 words repeat
    their first) for member 0, that case's logits seeded + 1000 m for member m, and the tables of `build_tables`"""
    dims, L, g, t, m, tab, M, mode = key
    c = build_cons_case(dims, L, t, g, (0, 1), seed)
    del c['cons'], c['met']
    lgs = [c.pop('lg')] + [build_cons_case(dims, L, t, g, (0, 1), seed + 1000 * i)['lg'] for i in range(1, M)]
    shared, per_clip = build_tables(dict(c, lg=lgs[0]), dims, t, tab, torch.Generator().manual_seed(seed + 55))
    return c, lgs, shared, per_clip


def run_excl(ops, c, lgs, shared, per_clip, key):
    dims, L, g, t, m, tab, M, mode = key
    V = dims[2]
    ops.beam_select_excl([x[:, 1:V + 1] for x in lgs], WEIGHTS[M], mode, c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'],
                         dims[1], END, c['hist'], c['hout'], t, shared, per_clip, no_repeat_ngram=g, min_len=m, ended_count=c['cnt'])


# ---------------------------------------------------------------------------------------------- the step, restated with lists
def restated_values(lgs, weights, mode):
    """the combined log-probs (R, V) float64 in numpy, and per row whether a member's row holds a NaN"""
    w = normalised_weights(weights)
    logp = []
    for x in lgs:
        x = x.double().numpy()
        with np.errstate(invalid='ignore'):
            mx = np.nanmax(x, axis=1, keepdims=True)
            logp.append(x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True))))
    dead = np.isnan(np.stack(logp)).any(2).any(0)
    if mode == 0:
        a = np.stack([l + np.log(wm) for l, wm in zip(logp, w)])
        with np.errstate(invalid='ignore'):
            mx = a.max(0)
            c = np.where(np.isinf(mx), -INF, mx + np.log(np.exp(a - mx).sum(0)))
    else:
        c = sum(wm * l for l, wm in zip(logp, w))
    return c, dead


def restated_row(vals, h, t, k, g, min_len, entries, V):
    """a live row on lists: its k best (value, class) that are not banned -- by the two bans of the history step and by
    `excluded_word` of every entry -- and the smallest gap between two neighbours of its k + 1 best finite values"""
    banned = banned_classes(list(h), t, g, min_len, END) | {excluded_word(list(h), e, V) for e in entries}
    vals = np.array(vals)
    vals[[b for b in banned if b is not None]] = -INF
    order = np.argsort(-vals, kind='stable')[:k + 1].tolist()                    # ties to the lower class
    fin = [float(vals[i]) for i in order if vals[i] > -INF]
    return [(float(vals[i]), i) for i in order[:k]], min([INF] + [a - b for a, b in zip(fin, fin[1:])])


def restated_step(c, lgs, shared, per_clip, key):
    """the step case on lists -> pred, nlp, back, hout (lists over the B*k slots), the number of <end>, gap per clip"""
    dims, L, g, t, m, tab, M, mode = key
    B, k, V = dims
    vals, dead = restated_values([x[:, 1:V + 1] for x in lgs], WEIGHTS[M], mode)
    sh = [] if shared is None else shared.tolist()
    out = dict(pred=[], nlp=[], back=[], hout=[], gap=[])
    for b in range(B):
        entries = sh + ([] if per_clip is None else per_clip[b].tolist())
        cands, gap = [], INF                                             # (value, parent, class) in candidate-index order
        for j in range(k if t else 1):
            r = b * k + j
            h = c['hist'][r, :t].tolist()
            lp = float(c['lp'][r]) if t else 0.0
            if t and int(c['last'][r]) == END:
                cands += [(lp, j, END)] + [(-INF, j, q - 1 if q - 1 < END else q) for q in range(1, k)]
            elif dead[r]:
                cands += [(-INF, j, NO_CLASS)] * k
            else:
                top, row_gap = restated_row(vals[r], h, t, k, g, m, entries, V)
                gap = min(gap, row_gap)
                cands += [(v + lp, j, cls) for v, cls in top]
        order = sorted(range(len(cands)), key=lambda i: (-cands[i][0], i))
        fin = [cands[i][0] for i in order[:k + 1] if cands[i][0] > -INF]
        gap = min([gap] + [x - y for x, y in zip(fin, fin[1:])])
        for i in order[:k]:
            v, j, cls = cands[i]
            out['pred'].append(cls); out['nlp'].append(v); out['back'].append(j)
            out['hout'].append(c['hist'][b * k + j, :t].tolist() + [cls] + [END] * (L - t - 1))
        out['gap'].append(gap)
    return out


@functools.lru_cache(maxsize=None)
def step_case(key):
    """(inputs c, member logits, shared, per_clip, emulated outputs, emulated gap (B,), restated outputs, input seeds tried) of a step
    case, computed once and never modified.  The inputs are seeded 100 g + t, then + 1000, + 2000 ... until at least nine tenths of
    the clips have a deciding gap of GAP or more in the restatement: a condition on the inputs, which the kernel is never asked
    about."""
    dims, L, g, t, m, tab, M, mode = key
    for tries in itertools.count(1):
        c, lgs, shared, per_clip = build_excl_case(key, 100 * g + t + 5000 * (tries - 1))
        want = restated_step(c, lgs, shared, per_clip, key)
        if 10 * sum(x >= GAP for x in want['gap']) >= 9 * dims[0]:
            break
    emul, e = ExclEmul(), fresh(c)
    run_excl(emul, e, lgs, shared, per_clip, key)
    return c, lgs, shared, per_clip, {o: e[o] for o in OUTPUTS}, emul.gap, want, tries


def test_step_cases_leave_few_clips_out():
    """by the restatement alone: every case keeps at least nine tenths of its clips"""
    keys = step_keys()
    assert len(keys) == 3 * 2 * 2 * 5 * 2 * 4 + 2 * 5 * 2 * 2
    assert {key[6:] for key in keys} == set(MEMBERS)
    tries, out, clips = 0, 0, 0
    for key in keys:
        want, n = step_case(key)[6:]
        assert 10 * sum(x >= GAP for x in want['gap']) >= 9 * key[0][0], key
        tries, out, clips = max(tries, n), out + sum(x < GAP for x in want['gap']), clips + len(want['gap'])
    print('%d of %d clips below %g; at most %d input seeds tried' % (out, clips, GAP, tries))
    assert tries <= 6


def test_the_emulated_step_is_the_restated_step():
    compared = 0
    for key in step_keys():
        c, _, _, _, out, gap, want, _ = step_case(key)
        B, k, V = key[0]
        for b in range(B):
            assert (gap[b] >= GAP) == (want['gap'][b] >= GAP) or abs(float(gap[b]) - want['gap'][b]) <= 1e-5, (key, b)
            if gap[b] < GAP or want['gap'][b] < GAP:
                continue
            s = slice(b * k, (b + 1) * k)
            assert out['pred'][s].tolist() == want['pred'][s] and out['back'][s].tolist() == want['back'][s], (key, b)
            assert out['hout'][s].tolist() == want['hout'][s], (key, b)
            assert out['rows'][s].tolist() == [b * k + j for j in want['back'][s]], (key, b)
            close_lp(out['nlp'][s].numpy(), want['nlp'][s])
            compared += 1
        if all(x >= GAP for x in want['gap']):
            assert int(out['cnt']) == sum(p == END for p in want['pred']), key
    assert compared > 1500


def test_the_step_cases_bite():
    """an exclusion changes the picks of the ensemble step in many cases of every kind of table; a context that stands earlier in
    the row but not at its end bans nothing; the lists take all 96 entries; with V = 5 every word of a live row is banned"""
    changed = collections.Counter()
    earlier, filled, all_banned = 0, 0, 0
    for key in step_keys():
        dims, L, g, t, m, tab, M, mode = key
        B, k, V = dims
        c, lgs, shared, per_clip, out, _, _, _ = step_case(key)
        if tab == 'empty':
            continue
        e = fresh(c)
        ExclEmul().beam_select_ens([x[:, 1:V + 1] for x in lgs], WEIGHTS[M], mode, e['last'], e['lp'], e['pred'], e['nlp'], e['back'],
                                   e['rows'], k, END, e['hist'], e['hout'], t, g, m, ended_count=e['cnt'])
        changed[tab] += int(not torch.equal(e['pred'], out['pred']))
        for b in range(B):
            for r in range(b * k, b * k + (k if t else 1)):
                if t and int(c['last'][r]) == END:
                    continue
                h = c['hist'][r, :t].tolist()
                rows = shared.tolist() + per_clip[b].tolist()
                hit = [excluded_word(h, row, V) for row in rows]
                if tab == 'mixed' and t >= 2:
                    earlier += sum(w is None and len(row) > 1 and row[0] in h[:-1] and row[1] >= 0 and row[2] < 0 for w, row in zip(hit, rows))
                if tab == 'full':
                    filled += sum(w is not None for w in hit) == 96
                    all_banned += V == 5 and {w for w in hit} >= set(range(V))
    print(dict(changed), earlier, filled, all_banned)
    assert all(changed[tab] >= 40 for tab in ('one', 'mixed', 'full')), changed
    assert earlier >= 50 and filled >= 200 and all_banned >= 10


def test_excluded_word():
    V = 10
    assert excluded_word([], [4, -1, -1, -1], V) == 4 and excluded_word([1, 2], [4, -1, 7, 7], V) == 4
    assert excluded_word([1, 2], [2, 4, -1, -1], V) == 4 and excluded_word([2, 1], [2, 4, -1, -1], V) is None
    assert excluded_word([], [2, 4, -1, -1], V) is None and excluded_word([3], [1, 2, 3, 4], V) is None
    assert excluded_word([9, 1, 2, 3], [1, 2, 3, 4], V) == 4 and excluded_word([1, 2, 3, 9], [1, 2, 3, 4], V) is None
    assert excluded_word([1, 2], [2, V, 4, -1], V) == 2 and excluded_word([1], [2, V, 4, -1], V) == 2
    assert excluded_word([1], [-1, 4, 5, 6], V) is None and excluded_word([1], [V, 1, 1, 1], V) is None


# ---------------------------------------------------------------------------------------------- packing
def named_vocab(words):
    vocab = dlsg_amd.make_vocab(4)
    for w in words:
        vocab.add_word(w)
    return vocab


def test_pack_exclusions_layouts():
    vocab = dlsg_amd.make_vocab(50)
    w = vocab.idx2word
    end, unk = vocab('<end>'), vocab('<unk>')
    ex = pack_exclusions(vocab, words=[w[10], 11], phrases=['%s %s' % (w[12], w[13]), (14, w[15], 16), 17, w[10]], suppress_unk=True)
    assert isinstance(ex, Exclusions) and ex.per_clip is None and ex.shared.dtype == torch.int64
    assert ex.shared.tolist() == [[10, -1, -1], [11, -1, -1], [12, 13, -1], [14, 15, 16], [17, -1, -1], [unk, -1, -1]]
    ex = pack_exclusions(vocab, bad_endings=[w[20], 21], per_clip=[[(w[22], w[23], w[24], w[25])], [], ['<unk>', w[26], w[26]]])
    assert ex.shared.tolist() == [[20, end, -1, -1], [21, end, -1, -1]]
    assert ex.per_clip.tolist() == [[[22, 23, 24, 25], [-1] * 4], [[-1] * 4] * 2, [[unk, -1, -1, -1], [26, -1, -1, -1]]]
    empty = pack_exclusions(vocab)
    assert empty == Exclusions(None, None)
    only = pack_exclusions(vocab, per_clip=[[], []])
    assert only.shared is None and only.per_clip.shape == (2, 0, 1)
    assert pack_exclusions(vocab, words=[7], device='cpu').shared.tolist() == [[7]]
    assert pack_exclusions(vocab, words=[(w[30], '<end>')]).shared.tolist() == [[30, end]]


def test_pack_exclusions_bad_endings():
    assert len(BAD_ENDINGS) == 17 and len(set(BAD_ENDINGS)) == 17 and BAD_ENDINGS[:3] == ('a', 'an', 'the') and BAD_ENDINGS[-1] == 'am'
    vocab = named_vocab(['man', 'a', 'with', 'dog', 'the', 'of'])
    end = vocab('<end>')
    ex = pack_exclusions(vocab, bad_endings=True)
    assert ex.shared.tolist() == [[vocab(x), end] for x in ('a', 'the', 'of', 'with')]          # (the list's order; the others are absent)
    assert pack_exclusions(named_vocab(['man']), bad_endings=True) == Exclusions(None, None)
    full = pack_exclusions(named_vocab(BAD_ENDINGS), bad_endings=True, suppress_unk=True)
    assert full.shared.shape == (18, 2)
    with pytest.raises(ValueError, match='not in the vocabulary'):
        pack_exclusions(vocab, bad_endings=['a', 'upon'])
    assert pack_exclusions(vocab, bad_endings=['a', 'upon'], skip_unknown=True).shared.tolist() == [[vocab('a'), end]]


def test_pack_exclusions_refusals():
    vocab = dlsg_amd.make_vocab(200)
    w = vocab.idx2word
    with pytest.raises(ValueError, match='65 shared exclusions, at most 64'):
        pack_exclusions(vocab, words=list(range(10, 75)))
    assert pack_exclusions(vocab, words=list(range(10, 74))).shared.shape == (64, 1)
    assert pack_exclusions(vocab, words=list(range(10, 74)) + [10, 11]).shared.shape == (64, 1)       # equal entries are folded
    with pytest.raises(ValueError, match='clip 1: 33 exclusions, at most 32 per clip'):
        pack_exclusions(vocab, per_clip=[[], list(range(10, 43))])
    assert pack_exclusions(vocab, per_clip=[[], list(range(10, 42))]).per_clip.shape == (2, 32, 1)
    with pytest.raises(ValueError, match='has 5 words, at most 4 per phrase'):
        pack_exclusions(vocab, phrases=[(10, 11, 12, 13, 14)])
    for empty in ('', '  ', ()):
        with pytest.raises(ValueError, match='an empty phrase'):
            pack_exclusions(vocab, phrases=[empty])
    with pytest.raises(ValueError, match='clip 0: an empty phrase'):
        pack_exclusions(vocab, per_clip=[['']])
    for word in ('<start>', '<pad>', vocab('<start>'), vocab('<pad>')):
        with pytest.raises(ValueError, match='cannot be excluded'):
            pack_exclusions(vocab, phrases=[(w[10], word)])
        with pytest.raises(ValueError, match='cannot be excluded'):
            pack_exclusions(vocab, words=[word])
    for bad in ('<end>', ('<end>', w[10]), (w[10], '<end>', w[11]), (vocab('<end>'),)):
        with pytest.raises(ValueError, match='<end> can only be the last of at least two words'):
            pack_exclusions(vocab, phrases=[bad])
    for bad in (dict(words=['no such word']), dict(words=[200]), dict(words=[-1]), dict(phrases=['%s nor this' % w[10]]),
                dict(per_clip=[[(10, 'nope')]])):
        with pytest.raises(ValueError, match='is not in the vocabulary'):
            pack_exclusions(vocab, **bad)
    got = pack_exclusions(vocab, words=['no such word', w[10]], phrases=['%s nor this' % w[11], (12, 13)], per_clip=[[(10, 'nope')], [14]],
                          skip_unknown=True)
    assert got.shared.tolist() == [[10, -1], [12, 13]] and got.per_clip.tolist() == [[[-1, -1]], [[14, -1]]]
    assert pack_exclusions(vocab, words=['<unk>']).shared.tolist() == [[vocab('<unk>')]]


def test_check_exclusions_refusals():
    cpu = torch.device('cpu')
    sh, pc = torch.full((3, 2), 5, dtype=torch.int64), torch.full((4, 2, 2), 6, dtype=torch.int64)
    got = check_exclusions(Exclusions(sh, pc), 4, cpu)
    assert got[0] is sh and got[1] is pc
    assert check_exclusions(Exclusions(None, None), 4, cpu) == [None, None]
    assert check_exclusions(Exclusions(sh[:0], pc[:, :0]), 4, cpu) == [None, None]
    assert check_exclusions(Exclusions(sh, torch.zeros(4, 0, 3, dtype=torch.int64)), 4, cpu)[1] is None
    with pytest.raises(ValueError, match='holds 4 clips, the batch 3'):
        check_exclusions(Exclusions(None, pc), 3, cpu)
    with pytest.raises(ValueError, match='not covered in diverse beam search'):
        check_exclusions(Exclusions(sh, None), 4, cpu, num_groups=2)
    for bad in (Exclusions(sh.int(), None), Exclusions(sh[0], None), Exclusions(None, pc[0]), Exclusions(sh.tolist(), None),
                Exclusions(torch.zeros(65, 1, dtype=torch.int64), None), Exclusions(None, torch.zeros(4, 33, 1, dtype=torch.int64)),
                Exclusions(torch.zeros(2, 5, dtype=torch.int64), None), Exclusions(sh, torch.zeros(4, 2, 3, dtype=torch.int64)),
                [sh], sh, 'a word'):
        with pytest.raises(ValueError, match='exclude'):
            check_exclusions(bad, 4, cpu)
    with pytest.raises(ValueError, match='the clips on meta'):
        check_exclusions(Exclusions(sh, None), 4, torch.device('meta'))


# ---------------------------------------------------------------------------------------------- exclusions_hit
def hits_by_lists(row, n_tokens, entries):
    """positions p < n_tokens at which an entry ends, counted once each"""
    count = 0
    for p in range(n_tokens):
        count += any(e and len(e) <= p + 1 and row[p + 1 - len(e):p + 1] == e for e in entries)
    return count


def test_exclusions_hit_against_lists():
    gen = torch.Generator().manual_seed(4)
    B, n, L, V = 5, 3, 12, 6
    ids = torch.randint(0, V, (B, n, L), generator=gen)
    lens = torch.randint(1, L + 1, (B, n), generator=gen)
    shared = torch.randint(-1, V, (7, 3), generator=gen)
    per_clip = torch.randint(-1, V + 2, (B, 4, 3), generator=gen)
    per_clip[2] = -1

    def cut(row, top):
        ok = [0 <= i < top for i in row]
        return row[:ok.index(False)] if False in ok else row
    for sh, pc, top in ((shared, per_clip, V), (shared, None, None), (None, per_clip, None), (None, None, None), (shared[:0], per_clip[:, :0], V)):
        got = exclusions_hit(ids, lens, Exclusions(sh, pc), vocab_size=top)
        assert got.shape == (B, n) and got.dtype == torch.int64
        for b in range(B):
            entries = [cut(r, top or 10 ** 9) for r in ([] if sh is None else sh.tolist()) + ([] if pc is None else pc[b].tolist())]
            for i in range(n):
                assert int(got[b, i]) == hits_by_lists(ids[b, i].tolist(), int(lens[b, i]), entries), (b, i)
        assert torch.equal(exclusions_hit(ids[:, 0], lens[:, 0], Exclusions(sh, pc), vocab_size=top), got[:, 0])
    assert int(exclusions_hit(ids, lens, Exclusions(shared, per_clip)).sum()) >= 15
    with pytest.raises(ValueError, match='holds 5 clips, ids 4'):
        exclusions_hit(ids[:4], lens[:4], Exclusions(None, per_clip))
    # a bad ending ends at the <end> that lens counts; behind lens nothing is counted
    row = torch.tensor([[[5, 4, 2, 2, 2]]])
    bad = Exclusions(torch.tensor([[4, 2]]), None)
    assert exclusions_hit(row, torch.tensor([[3]]), bad).tolist() == [[1]] and exclusions_hit(row, torch.tensor([[2]]), bad).tolist() == [[0]]
    assert exclusions_hit(row, torch.tensor([[5]]), Exclusions(torch.tensor([[2, 2]]), None)).tolist() == [[2]]


# ---------------------------------------------------------------------------------------------- the whole search
# the host model, and the model of the GPU tests (8 clips): chosen by the restated search alone, so that at most one clip in six
# (in eight) has a near-tie in any of SEARCHES
SEED, BATCH, BIAS = 144, 6, 1.0
SEARCHES = [(1, 0, 2, 0.0), (3, 2, 4, 0.7), (5, 0, 3, 0.7), (5, 3, 4, 0.0)]
GPU_CASE = dict(seed=189, batch=8, bias=2.0)                           # with (5, 2, 4, 0.7): captions of four and five words


def reference_excl_search(step_fn, start, state, end, L, k, g, min_len, entries, V):
    """`reference_search` of tests/test_beam_nbest_host.py with the bans of `excluded_word` added: every step of the search on
    Python lists; entries[b]: the clip's table rows, shared and its own"""
    B = start.numel()
    beams = [[dict(toks=[], lp=np.float32(0.0))] for _ in range(B)]
    gap = [INF] * B
    last = start
    for t in range(L):
        n = len(beams[0])
        logp, state = step_fn(last, state)
        logp = logp.numpy()
        parents = []
        for b in range(B):
            cands = []                                                    # (value, parent, class), in candidate-index order
            for j, bm in enumerate(beams[b]):
                if bm['toks'] and bm['toks'][-1] == end:
                    cands.append((bm['lp'], j, end))
                    continue
                banned = banned_classes(bm['toks'], t, g, min_len, end) | {excluded_word(bm['toks'], e, V) for e in entries[b]}
                row = logp[b * n + j]
                order = sorted((c for c in range(row.shape[0]) if c not in banned), key=lambda c: (-row[c], c))[:k]
                cands += [(np.float32(row[c] + bm['lp']), j, c) for c in order]
            ranked = sorted(range(len(cands)), key=lambda i: (-cands[i][0], i))
            assert len(ranked) >= k
            if len(ranked) > k and cands[ranked[k]][0] > -INF:
                gap[b] = min(gap[b], float(cands[ranked[k - 1]][0]) - float(cands[ranked[k]][0]))
            new = [dict(toks=beams[b][cands[i][1]]['toks'] + [cands[i][2]], lp=cands[i][0]) for i in ranked[:k]]
            parents += [b * n + cands[i][1] for i in ranked[:k]]
            beams[b] = new
        idx = torch.tensor(parents)
        state = {key: v[idx] for key, v in state.items()}
        last = torch.tensor([bm['toks'][-1] for bs in beams for bm in bs])
    return [[bm['toks'] for bm in bs] for bs in beams], [[bm['lp'] for bm in bs] for bs in beams], gap


def exclusions_from(free, end, vocab):
    """Exclusions that bite, from the captions `free` [B][k][L] of the search without them: the two words that stand in the best
    caption of most clips, for every clip; the words those captions stop behind, as the caller's own bad endings; and per clip
    the first two words of its second caption (its best caption's, with one beam), as ids -- clip 1 has none."""
    best = [words_of(clip[0], end) for clip in free]
    count = collections.Counter(w for words in best for w in set(words) if w >= 4)          # (<start> and <pad> cannot be excluded)
    common = [w for w, _ in sorted(count.items(), key=lambda x: (-x[1], x[0]))[:2]]
    endings = sorted({words[-1] for words in best if words and words[-1] >= 4} - set(common))
    per_clip = []
    for b, clip in enumerate(free):
        words = words_of(clip[min(1, len(clip) - 1)], end)
        per_clip.append([tuple(words[:2])] if len(words) >= 2 and min(words[:2]) >= 4 and b != 1 else [])
    ex = pack_exclusions(vocab, words=common, bad_endings=[vocab.idx2word[w] for w in endings], per_clip=per_clip)
    return ex, common, endings


@functools.lru_cache(maxsize=None)
def restated_search(k, g, min_len, alpha, seed=SEED, batch=BATCH, bias=BIAS):
    """(exclusions, ids, scores, lens, gap, the captions without exclusions, the shared words, the endings) by lists alone"""
    net, orc, frames, regions = synth_pair(seed, batch, end_bias=bias)
    step_fn, start, state, end, L = oracle_stepper(orc, frames, regions)
    V = net.decoder.vocab_size
    free = reference_excl_search(step_fn, start, state, end, L, k, g, min_len, [[]] * batch, V)[0]
    ex, common, endings = exclusions_from(free, end, net.decoder.vocab)
    entries = [ex.shared.tolist() + ex.per_clip[b].tolist() for b in range(batch)]
    toks, lps, gap = reference_excl_search(step_fn, start, state, end, L, k, g, min_len, entries, V)
    ids, sc, ln, rank_gap = reference_rank(toks, lps, end, alpha, k)
    return ex, ids, sc, ln, [min(a, b) for a, b in zip(gap, rank_gap)], free, common, endings


@functools.lru_cache(maxsize=None)
def emulated_search(k, g, min_len, alpha):
    net, orc, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ExclEmul())
    ex = restated_search(k, g, min_len, alpha)[0]
    return net.beam_search(frames, regions, beam_size=k, length_penalty=alpha, no_repeat_ngram=g, min_len=min_len, exclude=ex)


@pytest.mark.parametrize('k,g,min_len,alpha', SEARCHES)
def test_beam_search_with_exclusions_matches_the_restated_search(k, g, min_len, alpha):
    ex, want_ids, want_sc, want_len, gap = restated_search(k, g, min_len, alpha)[:5]
    ids, scores, lens = emulated_search(k, g, min_len, alpha)
    L = ids.shape[2]
    assert ids.shape == (BATCH, k, L) and scores.shape == (BATCH, k) and lens.shape == (BATCH, k)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and lens.dtype == torch.int64
    keep = [b for b in range(BATCH) if gap[b] >= GAP]
    assert len(keep) >= BATCH - 1, gap
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b], b
        close(scores[b].numpy(), want_sc[b])


def check_excluded(ids, scores, lens, ex, endings, end):
    """what the search owes: no caption of finite score holds an excluded entry or stops behind a listed ending"""
    hit = exclusions_hit(ids, lens, ex)
    finite = scores > -INF
    assert bool(finite[:, 0].all()) and not bool(hit[finite].any()), hit
    for b in range(ids.shape[0]):
        for i in range(ids.shape[1]):
            words = words_of(ids[b, i].tolist(), end)
            if bool(finite[b, i]) and words and len(words) < ids.shape[2]:
                assert words[-1] not in endings, (b, i)


@pytest.mark.parametrize('k,g,min_len,alpha', SEARCHES)
def test_no_caption_holds_what_is_excluded(k, g, min_len, alpha):
    ex, _, _, _, _, free, common, endings = restated_search(k, g, min_len, alpha)
    ids, scores, lens = emulated_search(k, g, min_len, alpha)
    assert endings and len(common) == 2
    check_excluded(ids, scores, lens, ex, endings, END)
    # vacuity guard: the search without them holds an excluded entry in the best caption of most clips
    free_ids = torch.tensor(free)
    free_lens = torch.tensor([[len(words_of(r, END)) + (END in r) for r in clip] for clip in free])
    assert 2 * int((exclusions_hit(free_ids, free_lens, ex)[:, 0] > 0).sum()) > BATCH


def test_bad_endings_of_the_projects_list():
    """a vocabulary that has some of the seventeen words: `bad_endings=True` keeps the captions from stopping behind them"""
    net, orc, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ExclEmul())
    vocab = net.decoder.vocab
    free = net.beam_search(frames, regions, beam_size=3, min_len=2)
    stops = collections.Counter(words_of(r, END)[-1] for r in free[0].view(-1, free[0].shape[2]).tolist() if words_of(r, END))
    for word, (i, _) in zip(('the', 'of', 'with'), stops.most_common(3)):          # rename the words the captions stop behind
        old = vocab.idx2word[i]
        vocab.idx2word[i] = word
        vocab.word2idx[word] = vocab.word2idx.pop(old)
    ex = pack_exclusions(vocab, bad_endings=True)
    assert ex.shared.shape[0] == min(3, len(stops)) >= 2
    ids, scores, lens = net.beam_search(frames, regions, beam_size=3, min_len=2, exclude=ex)
    listed = {vocab(w) for w in BAD_ENDINGS if w in vocab.word2idx}
    check_excluded(ids, scores, lens, ex, listed, END)
    assert not torch.equal(ids, free[0])


@pytest.mark.parametrize('k', [1, 3, 5])
def test_empty_exclusions_give_the_bits_of_the_search_without(k):
    net, _, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ExclEmul())
    opts = dict(beam_size=k, length_penalty=0.7, no_repeat_ngram=2, min_len=3)
    want = net.beam_search(frames, regions, **opts)
    for ex in (Exclusions(None, None), pack_exclusions(net.decoder.vocab, per_clip=[[]] * BATCH),
               Exclusions(torch.full((3, 2), -1, dtype=torch.int64), torch.full((BATCH, 2, 2), 50, dtype=torch.int64))):
        got = dlsg_amd.beam_search(net, frames, regions, exclude=ex, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(net.beam_search(frames, regions, exclude=None, **opts), want))


class Noting(ExclEmul):
    """ExclEmul that notes which step it was asked for, and the tables"""

    def __init__(self):
        super().__init__()
        self.steps, self.tables = collections.Counter(), []

    def __getattribute__(self, name):
        if name.startswith('beam_select'):
            object.__getattribute__(self, 'steps')[name] += 1
        return object.__getattribute__(self, name)

    def beam_select_excl(self, *a, **kw):
        self.tables.append(a[14:16])
        return super().beam_select_excl(*a, **kw)


def test_exclude_none_launches_what_it_launched_and_exclude_launches_the_new_step():
    ops = Noting()
    net, _, frames, regions = synth_pair(SEED, 2, ops=ops)
    L = net.decoder.max_words
    ex = pack_exclusions(net.decoder.vocab, words=[10], per_clip=[[(11, 12)], []])
    net.beam_search(frames, regions, beam_size=3)
    assert ops.steps == {'beam_select_hist': L}
    net.beam_search(frames, regions, beam_size=3, exclude=ex)
    assert ops.steps == {'beam_select_hist': L, 'beam_select_excl': L}
    assert all(sh is ex.shared and pc is ex.per_clip for sh, pc in ops.tables) and len(ops.tables) == L
    ens = dlsg_amd.Ensemble([net, net], weights=[0.6, 0.4])
    ens.beam_search(frames, regions, beam_size=3)
    assert ops.steps == {'beam_select_hist': L, 'beam_select_excl': L, 'beam_select_ens': L}
    ens.beam_search(frames, regions, beam_size=3, exclude=ex)
    assert ops.steps['beam_select_excl'] == 2 * L and ops.steps['beam_select_ens'] == L


def test_an_ensemble_of_the_model_twice_is_the_model():
    """weights 0.6 : 0.4 on one model, both modes: the captions of the model's own search under the same exclusions"""
    net, _, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ExclEmul())
    ex = restated_search(3, 2, 4, 0.7)[0]
    opts = dict(beam_size=3, length_penalty=0.7, no_repeat_ngram=2, min_len=4, exclude=ex)
    want = net.beam_search(frames, regions, **opts)
    for mode in ('prob', 'logprob'):
        got = dlsg_amd.Ensemble([net, net], weights=[0.6, 0.4], mode=mode).beam_search(frames, regions, **opts)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
        close(got[1].numpy(), want[1].numpy())


def test_what_is_not_covered_raises():
    net, _, frames, regions = synth_pair(SEED, 2, ops=ExclEmul())
    ex = pack_exclusions(net.decoder.vocab, words=[10])
    with pytest.raises(ValueError, match='not covered in diverse beam search'):
        net.beam_search(frames, regions, beam_size=4, num_groups=2, exclude=ex)
    with pytest.raises(ValueError, match='not covered in diverse beam search'):
        dlsg_amd.Ensemble([net]).beam_search(frames, regions, beam_size=4, num_groups=2, exclude=ex)
    with pytest.raises(TypeError, match='exclude'):
        net.constrained_beam_search(frames, regions, [[10], []], exclude=ex)
    with pytest.raises(TypeError, match='exclude'):
        net.sample_without_replacement(frames, regions, n=2, exclude=ex)
    with pytest.raises(TypeError, match='exclude'):
        net.sample(frames, regions, exclude=ex)
    with pytest.raises(ValueError, match="unknown keys \\['exclude'\\]"):
        dlsg_amd.SCSTTrainer(net, None, sample_options=dict(exclude=ex))
    from dlsg_amd.consensus import consensus_search
    with pytest.raises(TypeError, match='exclude'):
        consensus_search(net, frames, regions, None, stochastic=dict(n=2, exclude=ex))
    with pytest.raises(ValueError, match='holds 3 clips, the batch 2'):
        net.beam_search(frames, regions, exclude=pack_exclusions(net.decoder.vocab, per_clip=[[10], [], []]))
    with pytest.raises(ValueError, match='exclude: an Exclusions'):
        net.beam_search(frames, regions, exclude=[10])
    loader = [(frames, regions, None, ['v0', 'v1'])]
    with pytest.raises(ValueError, match='exclude and constraints cannot be combined'):
        S.gather_results(net, loader, decode=dict(beam_size=3, exclude=ex, constraints=lambda vids: [[10], []]))
    with pytest.raises(ValueError, match='without a per-clip part'):
        S.gather_results(net, loader, decode=dict(beam_size=3, exclude=pack_exclusions(net.decoder.vocab, per_clip=[[10], []])))


def test_every_entry_point_takes_the_keyword():
    import inspect
    for cls in (dlsg_amd.CapGnnModel, dlsg_amd.CapBaseline1, dlsg_amd.CapBaselineModel, dlsg_amd.Ensemble):
        assert inspect.signature(cls.beam_search).parameters['exclude'].default is None
    for fn in (dlsg_amd.beam_nbest, dlsg_amd.beam.ensemble_nbest):
        assert inspect.signature(fn).parameters['exclude'].default is None
    from dlsg_amd import abi
    assert len(abi.functions['dlsg_beam_select_excl'][1]) == 19
    assert abi.defines['DLSG_EXCL_SHARED'] == 64 and abi.defines['DLSG_EXCL_CLIP'] == 32 and abi.defines['DLSG_ABI_VERSION'] == 8
    for name in ('pack_exclusions', 'exclusions_hit', 'Exclusions', 'BAD_ENDINGS'):
        assert hasattr(dlsg_amd, name)


def test_gather_results_exclude_option():
    net, _, frames, regions = synth_pair(SEED, 3, end_bias=BIAS, ops=ExclEmul())
    vocab = net.decoder.vocab
    loader = [(frames, regions, None, ['v0', 'v1', 'v2'])]
    plain = S.gather_results(net, loader, decode=dict(beam_size=3, min_len=3))
    first = {vid: sent.split()[:2] for vid, sent in plain.items()}
    assert all(len(words) == 2 for words in first.values())
    common = collections.Counter(w for sent in plain.values() for w in set(sent.split())).most_common(1)[0][0]
    shared = pack_exclusions(vocab, words=[common])
    got = S.gather_results(net, loader, decode=dict(beam_size=3, min_len=3, exclude=shared))
    assert list(got) == ['v0', 'v1', 'v2'] and all(common not in sent.split() for sent in got.values())
    fn = lambda vids: pack_exclusions(vocab, per_clip=[[tuple(first[v])] if v != 'v1' else [] for v in vids])      # noqa: E731
    got = S.gather_results(net, loader, decode=dict(beam_size=3, min_len=3, exclude=fn))
    assert got['v1'] == plain['v1']
    for vid in ('v0', 'v2'):
        words = got[vid].split()
        assert all(words[i:i + 2] != first[vid] for i in range(len(words))), (vid, got[vid])
    assert S.gather_results(net, loader, decode=dict(beam_size=3, min_len=3, exclude=None)) == plain
    # consensus and rescore searches hand the keyword to their beam search
    from emul_seqscore import SeqScoreEmul
    net.set_ops(type('BothEmul', (ExclEmul, SeqScoreEmul), {})())
    ids = dlsg_amd.rescore_search(net, net, frames, regions, n_best=3, beam_size=3, min_len=3, exclude=shared)[0]
    assert not bool((ids == vocab(common)).any())


# ---------------------------------------------------------------------------------------------- the graph classes
class ReplayStub(object):
    def replay(self):
        pass


def test_the_graph_classes_keep_their_own_exclusions(monkeypatch):
    """without a capture (the body runs once, eagerly): `graph.exclude` holds copies of the two tables, the search runs on those very
    tensors, the other options stay `graph.options`, and a graph without the keyword runs what it ran"""
    monkeypatch.setattr(graphs, 'capture', lambda dev, body, warmup=None: (ReplayStub(), body()))
    ops = Noting()
    net, _, frames, regions = synth_pair(SEED, 2, end_bias=BIAS, ops=ops)
    L = net.decoder.max_words
    ex = pack_exclusions(net.decoder.vocab, words=[10, 11], per_clip=[[(12, 13)], [14]])
    opts = dict(beam_size=3, length_penalty=0.7)
    for make, eager in ((lambda **kw: dlsg_amd.NBestBeamGraph(net, frames, regions, **kw), net.beam_search),
                        (lambda **kw: dlsg_amd.EnsembleBeamGraph(dlsg_amd.Ensemble([net]), frames, regions, **kw),
                         dlsg_amd.Ensemble([net]).beam_search)):
        del ops.tables[:]
        graph = make(exclude=ex, **opts)
        assert graph.options == opts and isinstance(graph.exclude, Exclusions)
        for mine, theirs in zip(graph.exclude, ex):
            assert torch.equal(mine, theirs) and mine.data_ptr() != theirs.data_ptr()
        assert len(ops.tables) == L and all(sh is graph.exclude.shared and pc is graph.exclude.per_clip for sh, pc in ops.tables)
        assert all(torch.equal(a, b) for a, b in zip(graph.out, eager(frames, regions, exclude=ex, **opts)))
        n = ops.steps['beam_select_excl']
        plain = make(**opts)
        assert plain.exclude is None and plain.options == opts and ops.steps['beam_select_excl'] == n
        assert all(torch.equal(a, b) for a, b in zip(plain.out, eager(frames, regions, **opts)))
        only_shared = make(exclude=Exclusions(ex.shared, None), **opts)
        assert only_shared.exclude.per_clip is None and torch.equal(only_shared.exclude.shared, ex.shared)

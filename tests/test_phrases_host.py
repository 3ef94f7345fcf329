"""CPU: constrained beam search with multi-word phrases -- the emulated step (tests/emul_phrases.py) against an independent
restatement on Python lists (brute-force substring and border search, the banks by sorting), on the step cases that
tests/test_gpu_phrases.py runs on the kernel; that those cases bite; the reductions to `beam_select_cons` (one-word phrases) and
`beam_select_hist` (no constraints) and the invariance under padding; the guarantee; `beam.constrained_nbest` with phrases through
the emulated ops on a small host model against a restated whole search; `pack_phrases`, the dispatch, `phrases_met` and the graph's
staging rule."""
import functools
import heapq
import itertools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.beam import check_phrase_options, has_phrases, pack_constraints, pack_phrases, phrases_met
from emul_beam import BeamEmul, banned_classes
from emul_constrained import INF, ConsEmul
from emul_phrases import PHRASE_MAX, PhraseEmul
from test_beam_nbest_host import close, has_repeat, oracle_stepper, reference_rank, synth_pair, words_of
from test_constrained_host import GAP, SEARCHES, build_cons_case, close_lp, run_cons
from test_sbs_host import DIMS, END, fresh, steps_of

CWP = [(0, 1, 1), (1, 1, 2), (3, 2, 3), (8, 8, 4)]
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt', 'met', 'bank')
KINDS = ('completes', 'inside', 'overlap', 'share_a', 'share_b', 'lengths', 'dead', 'banned_next', 'junk_behind')


# ---------------------------------------------------------------------------------------------- step cases (shared with the GPU tests)
def step_keys(dims_list=DIMS, Ls=(26, 64)):
    """(dims, L, g, t, min_len, (C, W, P)) of every step case"""
    return [(dims, L, g, t, m, cwp) for dims in dims_list for L in Ls for g in (0, 2) for t in steps_of(L, g) for m in (0, t + 1)
            for cwp in CWP]


def build_phrase_case(dims, L, t, g, cwp, seed):
    """`build_cons_case` of tests/test_constrained_host.py -- its logits, histories and NaN rows -- with phrases.  Constraint c of
    clip b is of kind (c + b) % 8 and is built on row r = b k + c % k; where the step is too early or P too small for a kind it is a
    random phrase.  The kinds, also listed per case in c['kinds'] as (clip, constraint, name):
      0 completes    the first n - 1 words are the row's last tokens, so the next word completes the phrase; that word is the row's
                     best class on even clips (inside list A) and a random one on odd clips (list B only)
      1 inside       n consecutive tokens of the row's history: met by that row (the rows of a clip start with different tokens)
      2 overlap      "x x y" where the row's history is made to end "x x x": the progress is 2, not 0
      3 share_a      "u v" with u the row's last token, and
      4 share_b      "v w" with the v of the constraint before it: one word serves two constraints
      5 lengths      alternatives of 1, 2 and P words (as many as W allows); the 2-word one starts with the row's last token
      6 dead         a phrase whose first word is -inf in every row of the clip: never met, `end` stays banned
      7 banned_next  with g = 2 and t >= 3: the row's history is made "b c ... b" and the phrase is "c x", so the next word c is banned
                     by the bigram "b c" though "c x" does not occur; else junk_behind: "w, -1, junk" is the one-word phrase w, and
                     with W >= 2 a second alternative starts with an id >= V and is absent
    Rows whose history is rewritten are made live.  Clip B - 2 (where B >= 3) has no constraint."""
    B, k, V = dims
    C, W, P = cwp
    c = build_cons_case(dims, L, t, g, (C, W), seed)
    del c['cons']
    gen = torch.Generator().manual_seed(seed + 177)
    lg, hist, last = c['lg'], c['hist'], c['last']
    phr = torch.full((B, C, W, P), -1, dtype=torch.int64)
    lo = min(3, V - 1)
    x = lg[:, 1:V + 1]
    best = torch.where(torch.isnan(x), torch.full((), -INF), x).topk(min(3, V))[1]
    kinds, fixed, touched = [], {}, set()

    def rnd(n):
        return [int(v) for v in torch.randint(lo, V, (n,), generator=gen)]

    def live(r):
        if t and r >= k:
            last[r] = hist[r, t - 1]
    clips = [b for b in range(B) if C and not (B >= 3 and b == B - 2)]
    for b in clips:                                                   # pass 1: the kinds that rewrite a history
        for ci in range(C):
            kind, r = (ci + b) % 8, b * k + ci % k
            if r in touched:
                continue
            if kind == 2 and P >= 3 and t >= 3:
                xw, yw = rnd(2)
                hist[r, t - 3:t] = xw
                fixed[b, ci] = ('overlap', [[xw, xw, yw]])
            elif kind == 7 and g == 2 and t >= 3:
                bw, cw_ = rnd(2)
                after = [bw, cw_] + [int(v) for v in hist[r, 2:t - 1]] + [bw]
                free = [v for v in range(lo, V) if v not in (bw, cw_) and not any(p == cw_ and n == v for p, n in zip(after, after[1:]))]
                if bw == cw_ or not free:
                    continue
                hist[r, :t] = torch.tensor(after)
                fixed[b, ci] = ('banned_next', [[cw_, free[int(torch.randint(0, len(free), (1,), generator=gen))]]])
            else:
                continue
            touched.add(r)
            live(r)
    for b in clips:                                                   # pass 2: the phrases, on the histories as they are now
        for ci in range(C):
            kind, r = (ci + b) % 8, b * k + ci % k
            h = [int(v) for v in hist[r, :t]]
            name, alts = fixed.get((b, ci), (None, None))
            if name is None:
                if kind == 0:
                    n = min(P, t + 1)
                    cand = [int(v) for v in best[r] if int(v) != END]
                    name, alts = 'completes', [h[t - (n - 1):] + ([cand[0]] if b % 2 == 0 else rnd(1))]
                    live(r)
                elif kind == 1 and t >= 2:
                    n = min(P, t)
                    s = int(torch.randint(0, t - n + 1, (1,), generator=gen))
                    name, alts = 'inside', [h[s:s + n]]
                elif kind == 3 and t >= 1:
                    name, alts = 'share_a', [[h[-1]] + rnd(1)]
                    live(r)
                elif kind == 4 and ci > 0 and kinds and kinds[-1] == (b, ci - 1, 'share_a'):
                    name, alts = 'share_b', [[int(phr[b, ci - 1, 0, 1])] + rnd(1)]
                elif kind == 5 and t >= 1:
                    name, alts = 'lengths', ([rnd(1), [h[-1]] + rnd(1), rnd(P)] if W >= 3 else [rnd(1), [h[-1]] + rnd(P - 1)][:W])
                elif kind == 6:
                    words = rnd(P)
                    lg[b * k:(b + 1) * k, 1 + words[0]] = -INF
                    name, alts = 'dead', [words]
                elif kind == 7:
                    name, alts = 'junk_behind', [rnd(1) + [-1] + rnd(P - 2)] + ([[V + 5] + rnd(P - 1)] if W >= 2 else [])
                else:
                    alts = [rnd(1 + int(torch.randint(0, P, (1,), generator=gen)))]
            for w_, a in enumerate(alts[:W]):
                phr[b, ci, w_, :len(a)] = torch.tensor(a)
            if W >= 4 and name in (None, 'completes', 'inside'):      # further alternatives: a random phrase, padding, an id >= V
                extra = rnd(2)
                phr[b, ci, 1, :len(extra[:P])] = torch.tensor(extra[:P])
                phr[b, ci, 3, 0] = V + 5
            if name:
                kinds.append((b, ci, name))
    c['phr'] = phr
    c['met'] = torch.zeros(B * k, dtype=torch.int32)
    c['bank'] = torch.zeros(B * k, dtype=torch.int32)
    c['kinds'] = kinds
    return c


def tensors(c):
    return {o: v for o, v in c.items() if torch.is_tensor(v)}


def run_phrases(ops, c, key, phr='case'):
    dims, L, g, t, m, cwp = key
    V = dims[2]
    ops.beam_select_phrases(c['lg'][:, 1:V + 1], c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'], dims[1], END, c['hist'],
                            c['hout'], t, c['phr'] if isinstance(phr, str) else phr, no_repeat_ngram=g, min_len=m,
                            ended_count=c['cnt'], met_out=c['met'], bank_out=c['bank'])


@functools.lru_cache(maxsize=None)
def emulated_step(key):
    """(inputs, emulated outputs, gap (B,), stats, input seeds tried) of a step case, computed once and never modified.  The inputs
    are seeded 100 g + t, then + 1000, + 2000 ... until at least 90 % of the clips have a gap of GAP or more in the emulation: a
    condition on the inputs, which the kernel is never asked about."""
    dims, L, g, t, m, cwp = key
    emul = PhraseEmul()
    for tries in itertools.count(1):
        c = build_phrase_case(dims, L, t, g, cwp, 100 * g + t + 1000 * (tries - 1))
        e = fresh(tensors(c))
        run_phrases(emul, e, key)
        if 10 * int((emul.gap >= GAP).sum()) >= 9 * dims[0]:
            return c, {o: e[o] for o in OUTPUTS}, emul.gap, emul.stats, tries


def test_step_cases_leave_few_clips_out():
    keys = step_keys()
    assert len(keys) == 6 * 2 * 7 * 2 * 4
    tries, out, clips = 0, 0, 0
    for key in keys:
        _, _, gap, _, n = emulated_step(key)
        assert 10 * int((gap >= GAP).sum()) >= 9 * key[0][0], key
        tries, out, clips = max(tries, n), out + int((gap < GAP).sum()), clips + gap.numel()
    print('%d of %d clips below %g; at most %d input seeds tried' % (out, clips, GAP, tries))
    assert tries <= 6


# ---------------------------------------------------------------------------------------------- the step, restated with lists
def contains(toks, a):
    """brute-force substring search"""
    return any(list(toks[i:i + len(a)]) == list(a) for i in range(len(toks) - len(a) + 1))


def border(toks, a):
    """the longest proper prefix of a, at most len(toks) long, that the tokens end with"""
    return max(j for j in range(min(len(a) - 1, len(toks)) + 1) if list(toks[len(toks) - j:]) == list(a[:j]))


def state_of(toks, alts):
    """(the set of constraints met, the row's progress)"""
    met = frozenset(c for c, al in enumerate(alts) if any(contains(toks, a) for a in al))
    return met, max([border(toks, a) for c, al in enumerate(alts) if c not in met for a in al] + [0])


def phrase_lists(phr_b, V):
    """a clip's constraints as lists of phrases: the ids up to the first one outside [0, V)"""
    out = []
    for con in phr_b:
        al = [list(itertools.takewhile(lambda i: 0 <= i < V, row)) for row in con]
        out.append([a for a in al if a])
    return out


def restated_clip_step(beams, raw, logp, t, k, end, g, min_len, alts, P, neighbours=True):
    """One clip's step on Python lists, as `restated_clip_step` of tests/test_constrained_host.py states the word step.  beams:
    [(tokens, log-prob, ended)] of the rows that are read; raw / logp: per row the values the classes are ranked by and their
    log-probs.  -> (picks [(value, parent, class, met, progress)] in output order, the classes of the first row's list A, the
    smallest gap: of a row's k-th to its next unbanned value, of a slot's best to its second-best proposal of the largest gain, of a
    bank's last pick to the best candidate left in it (with `neighbours`: of every pick, of any two neighbouring values of a bank
    and of every row's k-th))"""
    C, V = len(alts), len(raw[0])
    A, Bs, states, gap, row_gap = [], [], [], INF, {}
    for j, (toks, lp, ended) in enumerate(beams):
        met, q = state_of(toks, alts)
        states.append((met, q))
        if ended:
            A.append([(lp, end)] + [(-INF, i - 1 if i - 1 < end else i) for i in range(1, k)])
            Bs.append([None] * C)
            continue
        unmet = [c for c in range(C) if alts[c] and c not in met]
        banned = banned_classes(list(toks), t, g, min_len, end) | ({end} if unmet else set())
        nan = {c for c in range(V) if raw[j][c] != raw[j][c]}
        vals = [-INF if c in nan or c in banned else raw[j][c] for c in range(V)]
        top = heapq.nlargest(min(V, k + 1 + len(nan)), zip(vals, range(0, -V, -1)))
        top = [(v, -i) for v, i in top if -i not in nan][:k + 1]
        assert len(top) >= k
        whole = logp[j][0] == logp[j][0]                             # no NaN in the row: one makes every log-prob of the row NaN
        if whole and len(top) > k and top[k - 1][0] > -INF:
            row_gap[j, top[k - 1][1]] = top[k - 1][0] - top[k][0]
        A.append([(np.float32(-INF) if v == -INF and whole else np.float32(np.float32(logp[j][c]) + lp), c) for v, c in top[:k]])
        offered, slots = {c for _, c in top[:k]}, []
        for c in range(C):
            props = []                                                # (-gain, -logit, class)
            for a in alts[c] if c in unmet else []:
                p = border(toks, a)
                if a[p] not in banned and raw[j][a[p]] > -INF:
                    props.append((-(P if p + 1 == len(a) else p + 1), -raw[j][a[p]], a[p]))
            props = sorted(set(props))
            words = [pr for pr in props if pr[0] == props[0][0]]
            if whole and len(words) > 1:
                gap = min(gap, words[1][1] - words[0][1])
            if words and words[0][2] not in offered:
                offered.add(words[0][2])
                slots.append((np.float32(np.float32(logp[j][words[0][2]]) + lp), words[0][2]))
            else:
                slots.append(None)
        Bs.append(slots)
    cands = []                                                        # in candidate-index order: (value, parent, class, met, q)
    for lists in (A, Bs):
        for j, lst in enumerate(lists):
            for e in lst:
                if e is not None and e[0] > -INF:
                    st = states[j] if e[1] == end else state_of(tuple(beams[j][0]) + (e[1],), alts)
                    cands.append((float(e[0]), j, e[1]) + st)
    bank = [(len(cd[3]), cd[4]) for cd in cands]
    left = list(range(len(cands)))
    if neighbours:
        for bk in set(bank):
            vals = sorted(cands[i][0] for i in left if bank[i] == bk)
            gap = min([gap] + [y - x for x, y in zip(vals, vals[1:])])
    picks, last_gap = [], {}
    while len(picks) < k and left:
        for bk in sorted({bank[i] for i in left}, reverse=True):      # the banks by sorting: (met, progress), highest first
            inb = sorted((i for i in left if bank[i] == bk), key=lambda i: (-cands[i][0], i))
            if len(picks) < k:
                if len(inb) > 1:
                    last_gap[bk] = cands[inb[0]][0] - cands[inb[1]][0]
                    gap = min(gap, last_gap[bk]) if neighbours else gap
                picks.append(cands[inb[0]])
                left.remove(inb[0])
    gap = min([gap] + ([] if neighbours else list(last_gap.values())) +
              [v for (j, c), v in row_gap.items() if neighbours or any(p[1] == j and p[2] == c for p in picks)])
    return picks, [c for _, c in A[0]], gap


def restated_step(c, key):
    """the step case on lists, log-softmax in float64 -> (pred, new_lp, back, met, bank, hist rows, gap per clip)"""
    dims, L, g, t, m, cwp = key
    B, k, V = dims
    x = c['lg'][:, 1:V + 1].double().numpy()
    mx = np.nanmax(np.where(np.isinf(x), np.nan, x), axis=1, keepdims=True)
    logp = x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))
    out = dict(pred=[], nlp=[], back=[], met=[], bank=[], hout=[], gap=[])
    for b in range(B):
        alts = phrase_lists(c['phr'][b].tolist(), V)
        rows = range(b * k, b * k + (k if t else 1))
        beams = [(tuple(c['hist'][r, :t].tolist()), np.float32(c['lp'][r]) if t else np.float32(0), bool(t) and int(c['last'][r]) == END)
                 for r in rows]
        picks, first_a, gap = restated_clip_step(beams, [x[r].tolist() for r in rows], [logp[r].tolist() for r in rows], t, k, END, g,
                                                 m, alts, cwp[2])
        for i in range(k):
            v, j, cls, mask, q = picks[i] if i < len(picks) else (-INF, 0, first_a[i], (), 0)
            out['pred'].append(cls); out['nlp'].append(v); out['back'].append(j); out['met'].append(sum(1 << n for n in mask))
            out['bank'].append(len(mask) * PHRASE_MAX + q)
            out['hout'].append(list(beams[j][0]) + [cls] + [END] * (L - t - 1))
        out['gap'].append(gap)
    return out


def test_the_emulated_step_is_the_restated_step():
    compared = 0
    for key in step_keys():
        c, out, gap, _, _ = emulated_step(key)
        B, k, V = key[0]
        want = restated_step(c, key)
        for b in range(B):
            assert (gap[b] >= GAP) == (want['gap'][b] >= GAP) or abs(float(gap[b]) - want['gap'][b]) <= 1e-5, (key, b)
            if gap[b] < GAP:
                continue
            s = slice(b * k, (b + 1) * k)
            assert out['pred'][s].tolist() == want['pred'][s] and out['back'][s].tolist() == want['back'][s], (key, b)
            assert out['met'][s].tolist() == want['met'][s] and out['hout'][s].tolist() == want['hout'][s], (key, b)
            assert out['bank'][s].tolist() == want['bank'][s], (key, b)
            assert out['rows'][s].tolist() == [b * k + j for j in want['back'][s]], (key, b)
            close_lp(out['nlp'][s].numpy(), want['nlp'][s])
            compared += 1
        if all(g >= GAP for g in want['gap']):
            assert int(out['cnt']) == sum(p == END for p in want['pred']), key
    assert compared > 2000


def test_the_step_cases_bite():
    """every kind of phrase changes some output against the step without that constraint, and the paths of the step -- list-B picks,
    de-duplication, several banks in one step, banks that differ by progress alone, a pick that completes a phrase, a slot decided
    by the gain, `end` kept from an unmet row, left-over slots -- are each taken in many cases"""
    total = dict(list_b=0, dedup=0, multi_bank=0, end_blocked=0, leftover=0, completes=0, progress_bank=0, gain_decides=0)
    bites = dict.fromkeys(KINDS, 0)
    for key in step_keys():
        c, out, _, stats, _ = emulated_step(key)
        for name in total:
            total[name] += int(stats[name] > 0)
        k = key[0][1]
        for b, ci, name in c['kinds']:
            if bites[name] >= 3:
                continue
            without = c['phr'].clone()
            without[b, ci] = -1
            e = fresh(tensors(c))
            run_phrases(PhraseEmul(), e, key, without)
            bites[name] += any(not torch.equal(e[o][b * k:(b + 1) * k], out[o][b * k:(b + 1) * k]) for o in ('pred', 'back', 'met', 'bank'))
    print(total, bites)
    assert min(total.values()) >= 20, total
    assert min(bites.values()) >= 3, bites


def test_the_crafted_kinds_are_what_they_claim():
    """on the inputs alone: the progress of "x x y" behind "x x x" is 2; the next word of a banned_next phrase is banned although the
    phrase does not occur; a completes phrase is one word short; an inside phrase occurs"""
    seen = dict.fromkeys(('overlap', 'banned_next', 'completes', 'inside'), 0)
    for key in step_keys(Ls=(26,)):
        dims, L, g, t, m, cwp = key
        c = emulated_step(key)[0]
        k, V = dims[1], dims[2]
        alts_all = [phrase_lists(c['phr'][b].tolist(), V) for b in range(dims[0])]
        for b, ci, name in c['kinds']:
            if name not in seen:
                continue
            h = c['hist'][b * k + ci % k, :t].tolist()
            a = alts_all[b][ci][0]
            if name == 'overlap':
                assert border(h, a) == 2 and a[0] == a[1]
            elif name == 'banned_next':
                assert border(h, a) == 0 and a[0] in banned_classes(h, t, g, 0, END) and not contains(h, a)
            elif name == 'completes':
                assert border(h, a) == len(a) - 1
            else:
                assert contains(h, a)
            seen[name] += 1
    assert min(seen.values()) >= 4, seen


# ---------------------------------------------------------------------------------------------- reductions
def test_one_word_phrases_give_the_word_step():
    """P = 1: the outputs of ConsEmul.beam_select_cons on the word cases' inputs, and a bank that is 4 times the count"""
    for key in step_keys(Ls=(26,)):
        dims, L, g, t, m, cwp = key
        if cwp[2] != 3:
            continue
        for cw in ((3, 2), (8, 8)):
            c = build_cons_case(dims, L, t, g, cw, 100 * g + t)
            want, got = fresh(c), fresh(c)
            run_cons(ConsEmul(), want, (dims, L, g, t, m, cw))
            got['phr'], got['bank'] = got.pop('cons').unsqueeze(3), torch.zeros_like(got['met'])
            run_phrases(PhraseEmul(), got, key)
            for o in ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt', 'met'):
                assert torch.equal(got[o], want[o]) or (o == 'nlp' and torch.equal(got[o].view(torch.int32), want[o].view(torch.int32))), (key, cw, o)
            count = torch.tensor([bin(int(v)).count('1') for v in got['met']], dtype=torch.int32)
            assert torch.equal(got['bank'], count * PHRASE_MAX)


def test_without_constraints_the_step_is_beam_select_hist():
    for key in step_keys(Ls=(26,)):
        dims, L, g, t, m, cwp = key
        if cwp != (8, 8, 4):
            continue
        B, k, V = dims
        c = build_cons_case(dims, L, t, g, (8, 8), 100 * g + t, nan=False)
        del c['cons']
        c['bank'] = torch.zeros_like(c['met'])
        want = fresh(c)
        BeamEmul().beam_select_hist(want['lg'][:, 1:V + 1], want['last'], want['lp'], want['pred'], want['nlp'], want['back'],
                                    want['rows'], k, END, want['hist'], want['hout'], t, g, m, ended_count=want['cnt'])
        for phr in (None, torch.zeros(B, 0, 1, 1, dtype=torch.int64), torch.full((B, 3, 2, 2), -1, dtype=torch.int64),
                    torch.full((B, 2, 2, 4), V, dtype=torch.int64)):
            got = fresh(c)
            run_phrases(PhraseEmul(), got, key, phr)
            real = want['nlp'] > -INF                                   # (a left-over slot names a class among -inf ties: topk's choice)
            assert torch.equal(got['nlp'], want['nlp']), key
            for o in ('pred', 'back', 'rows', 'hout'):
                assert torch.equal(got[o][real], want[o][real]), (key, o)
            assert not bool(real.all()) or torch.equal(got['cnt'], want['cnt']), key
            assert not bool(got['met'].any()) and not bool(got['bank'].any())


def widened(phr, C, W, P):
    wide = torch.full((phr.shape[0], C, W, P), -1, dtype=torch.int64)
    wide[:, :phr.shape[1], :phr.shape[2], :phr.shape[3]] = phr
    return wide


def test_padding_changes_nothing():
    for key in step_keys(Ls=(26,)):
        if key[5] not in ((1, 1, 2), (3, 2, 3)):
            continue
        c, out, _, _, _ = emulated_step(key)
        got = fresh(tensors(c))
        run_phrases(PhraseEmul(), got, key, widened(c['phr'], 8, 8, 4))
        for o in OUTPUTS:
            assert torch.equal(got[o], out[o]) or o == 'nlp' and torch.equal(got[o].view(torch.int32), out[o].view(torch.int32)), (key, o)


# ---------------------------------------------------------------------------------------------- the whole search
SEED, BATCH, BIAS = 147, 6, 2.0


def clip_phrases(n_max, seed=5, batch=BATCH):
    """per clip 0 .. n_max constraints (clip b has b % (n_max + 1)) of 1 or 2 alternative phrases of 1 to 3 word ids of the 50-word
    vocabulary"""
    rng = np.random.RandomState(seed)
    return [[[tuple(int(v) for v in rng.choice(np.arange(4, 50), size=1 + (b + c + a) % 3, replace=False)) for a in range(1 + (b + c) % 2)]
             for c in range(b % (n_max + 1))] for b in range(batch)]


def reference_phrase_search(step_fn, start, state, end, L, k, g, min_len, per_clip):
    """`reference_constrained_search` of tests/test_constrained_host.py with the phrase step: every step on Python lists"""
    B = start.numel()
    alts = [[[list(a) for a in con] for con in clip] for clip in per_clip]
    P = max([len(a) for clip in alts for con in clip for a in con] + [1])
    beams = [[((), np.float32(0.0), False)] for _ in range(B)]
    gap = [INF] * B
    last = start
    for t in range(L):
        n = len(beams[0])
        logp, state = step_fn(last, state)
        logp = logp.double().numpy()
        parents = []
        for b in range(B):
            rows = [logp[b * n + j].tolist() for j in range(n)]
            picks, _, gp = restated_clip_step(beams[b], rows, rows, t, k, end, g, min_len, alts[b], P, neighbours=False)
            assert len(picks) == k
            gap[b] = min(gap[b], gp)
            parents += [b * n + p[1] for p in picks]
            beams[b] = [(beams[b][p[1]][0] + (p[2],), np.float32(p[0]), p[2] == end) for p in picks]
        idx = torch.tensor(parents)
        state = {key: v[idx] for key, v in state.items()}
        last = torch.tensor([bm[0][-1] for bs in beams for bm in bs])
    return [[list(bm[0]) for bm in bs] for bs in beams], [[bm[1] for bm in bs] for bs in beams], gap


def count_met(row, clip, end):
    """constraints with a phrase among the caption's words, as contiguous words"""
    return sum(any(contains(words_of(row, end), a) for a in con) for con in clip)


def ranked_by_met(toks, lps, gap, per_clip, end, alpha, k):
    """the ranking by score, then the stable sort by constraints met -> (ids, scores, lens, met, gap)"""
    ids, sc, ln, rank_gap = reference_rank(toks, lps, end, alpha, k)
    out = [], [], [], []
    for b in range(len(per_clip)):
        met = [count_met(row, per_clip[b], end) for row in ids[b]]
        order = sorted(range(k), key=lambda i: (-met[i], i))
        for dst, src in zip(out, (ids[b], sc[b], ln[b], met)):
            dst.append([src[i] for i in order])
    return out + ([min(a, b) for a, b in zip(gap, rank_gap)],)


@functools.lru_cache(maxsize=None)
def restated_search(k, g, min_len, alpha, n_max):
    net, orc, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS)
    per_clip = clip_phrases(n_max)
    step_fn, start, state, end, L = oracle_stepper(orc, frames, regions)
    toks, lps, gap = reference_phrase_search(step_fn, start, state, end, L, k, g, min_len, per_clip)
    return ranked_by_met(toks, lps, gap, per_clip, end, alpha, k)


@functools.lru_cache(maxsize=None)
def emulated_search(k, g, min_len, alpha, n_max):
    net, orc, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=PhraseEmul())
    phr = pack_phrases(clip_phrases(n_max), net.decoder.vocab)
    return net.constrained_beam_search(frames, regions, phr, beam_size=k, length_penalty=alpha, no_repeat_ngram=g, min_len=min_len,
                                       return_met=True)


@pytest.mark.parametrize('k,g,min_len,alpha,n_max', SEARCHES)
def test_constrained_nbest_with_phrases_matches_the_restated_search(k, g, min_len, alpha, n_max):
    want_ids, want_sc, want_len, want_met, gap = restated_search(k, g, min_len, alpha, n_max)
    ids, scores, lens, met = emulated_search(k, g, min_len, alpha, n_max)
    L = ids.shape[2]
    assert ids.shape == (BATCH, k, L) and scores.shape == (BATCH, k) and lens.shape == (BATCH, k) and met.shape == (BATCH, k)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and lens.dtype == torch.int64 and met.dtype == torch.int64
    keep = [b for b in range(BATCH) if gap[b] >= GAP]
    assert len(keep) >= BATCH - 1, gap
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b] and met[b].tolist() == want_met[b], b
        close(scores[b].numpy(), want_sc[b])


def check_search_properties(ids, scores, lens, met, per_clip, end, g, min_len, complete=True):
    """`check_search_properties` of the word tests with phrase containment in place of word membership: met is the number of
    constraints with a phrase in the row; a row that ends before L has met them all; rows in order of met, then score; no repeated
    g-gram, at least min_len words, <end>-padded; `complete` (the guarantee holds: g = 0): row 0 meets every constraint"""
    ids, scores, lens, met = ids.cpu(), scores.cpu(), lens.cpu(), met.cpu()
    B, n, L = ids.shape
    for b in range(B):
        Cb = len(per_clip[b])
        assert not complete or int(met[b, 0]) == Cb, b
        for i in range(n):
            row = ids[b, i].tolist()
            words = words_of(row, end)
            assert int(met[b, i]) == count_met(row, per_clip[b], end) <= Cb, (b, i)
            assert len(words) == L or int(met[b, i]) == Cb, (b, i)
            assert int(lens[b, i]) == min(len(words) + 1, L)
            assert (g == 0 or not has_repeat(words, g)) and len(words) >= min_len and all(w == end for w in row[len(words):]), (b, i)
        for i in range(n - 1):
            assert (int(met[b, i]), float(scores[b, i])) >= (int(met[b, i + 1]), float(scores[b, i + 1])), (b, i)


@pytest.mark.parametrize('k,g,min_len,alpha,n_max', SEARCHES)
def test_phrase_search_properties(k, g, min_len, alpha, n_max):
    check_search_properties(*emulated_search(k, g, min_len, alpha, n_max), clip_phrases(n_max), END, g, min_len, complete=g == 0)


@pytest.mark.parametrize('k', [1, 3, 5])
def test_the_guarantee(k):
    """random finite logits from the host model, no n-gram ban, up to 3 constraints of up to 3-word phrases: row 0 contains a phrase
    of every constraint; with k = 1 only the order of the banks can bring that about"""
    per_clip = clip_phrases(3, seed=11)
    net, _, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=PhraseEmul())
    ids, scores, lens, met = net.constrained_beam_search(frames, regions, pack_phrases(per_clip, net.decoder.vocab), beam_size=k,
                                                         return_met=True)
    for b in range(BATCH):
        assert int(met[b, 0]) == len(per_clip[b]) == count_met(ids[b, 0].tolist(), per_clip[b], END), b
    free = net.beam_search(frames, regions, beam_size=k, n_best=1)[0][:, 0]
    have = [b for b in range(BATCH) if per_clip[b]]
    assert 2 * sum(count_met(free[b].tolist(), per_clip[b], END) == len(per_clip[b]) for b in have) < len(have)


# ---------------------------------------------------------------------------------------------- interface
def test_pack_phrases():
    vocab = dlsg_amd.make_vocab(50)
    w = vocab.idx2word
    got = pack_phrases([[w[10] + ' ' + w[11], [w[12], (13, w[14], 15)]], [], [[' %s  %s ' % (w[16], w[17]), 18]]], vocab)
    assert got.dtype == torch.int64 and got.shape == (3, 2, 2, 3)
    assert got[0].tolist() == [[[10, 11, -1], [-1] * 3], [[12, -1, -1], [13, 14, 15]]]
    assert got[1].tolist() == [[[-1] * 3] * 2] * 2 and got[2].tolist() == [[[16, 17, -1], [18, -1, -1]], [[-1] * 3] * 2]
    assert pack_phrases([[], []], vocab).shape == (2, 0, 1, 1)
    assert pack_phrases([[7]], vocab, device='cpu').tolist() == [[[[7]]]]
    assert pack_phrases([[[(10, 11), '%s %s' % (w[10], w[11]), (10, 12)]]], vocab).tolist() == [[[[10, 11], [10, 12]]]]     # folded
    for bad in ('no such word', w[10] + ' nope', 50, (10, 50)):
        with pytest.raises(ValueError, match='not in the vocabulary'):
            pack_phrases([[bad]], vocab)
    assert pack_phrases([[w[10] + ' nope', [w[9], 'nor this', (9, 50)]]], vocab, skip_unknown=True).tolist() == [[[[-1]], [[9]]]]
    with pytest.raises(ValueError, match='at most 8'):
        pack_phrases([list(range(10, 19))], vocab)
    with pytest.raises(ValueError, match='at most 8'):
        pack_phrases([[list(range(10, 19))]], vocab)
    with pytest.raises(ValueError, match='at most 4'):
        pack_phrases([[' '.join(w[10:15])]], vocab)
    with pytest.raises(ValueError, match='at most 4'):
        pack_phrases([[(10, 11, 12, 13, 14)]], vocab)
    assert pack_phrases([[(10, 11, 12, 13)]], vocab).shape == (1, 1, 1, 4)
    with pytest.raises(ValueError, match='empty phrase'):
        pack_phrases([['  ']], vocab)
    for word in ('<end>', '<start>', '<pad>'):
        with pytest.raises(ValueError, match='cannot be required'):
            pack_phrases([[w[10] + ' ' + word]], vocab)
    with pytest.raises(ValueError, match='cannot be required'):
        pack_phrases([[(10, vocab('<end>'))]], vocab)
    # pack_constraints is unchanged: there a tuple stays a set of alternatives
    assert pack_constraints([[(10, 11)]], vocab).tolist() == [[[10, 11]]]
    assert has_phrases([[w[10]], [[w[11], w[12] + ' ' + w[13]]]]) and not has_phrases([[w[10], (11, 12)], [[w[11], 13]]])


def test_word_lists_pack_alike():
    """lists of words -- no tuple, which the two packers read differently -- give `pack_phrases` the tensor of `pack_constraints`
    with a trailing axis of one, and what both refuse they refuse in the same words"""
    vocab = dlsg_amd.make_vocab(50)
    w = vocab.idx2word
    lists = [[w[10], 11, [w[12], 13, w[12], 12], {14, 15}], [], [[w[16], 16, 17, 21], frozenset([18])], [19]]
    got = pack_phrases(lists, vocab)
    assert got.shape == (4, 4, 3, 1) and torch.equal(got[..., 0], pack_constraints(lists, vocab))
    assert got[0, :3, :, 0].tolist() == [[10, -1, -1], [11, -1, -1], [12, 13, -1]] and sorted(got[0, 3, :, 0].tolist()) == [-1, 14, 15]
    assert got[1:, :, :, 0].tolist() == [[[-1] * 3] * 4, [[16, 17, 21], [18, -1, -1]] + [[-1] * 3] * 2, [[19, -1, -1]] + [[-1] * 3] * 3]
    unknown = [['no such word', [w[9], 'nor', 50, -1]], [[60], w[20]]]
    got = pack_phrases(unknown, vocab, skip_unknown=True)
    assert torch.equal(got[..., 0], pack_constraints(unknown, vocab, skip_unknown=True))
    assert got[..., 0].tolist() == [[[-1], [9]], [[-1], [20]]]
    empty = pack_phrases([[], []], vocab)
    assert empty.shape == (2, 0, 1, 1) and torch.equal(empty[..., 0], pack_constraints([[], []], vocab))
    refused = [[list(range(10, 19))], [[10], [list(range(10, 19))]], [['nope']], [[10, [11, 50]]], [[w[10]], ['<end>']], [[[10, vocab('<pad>')]]],
               [[vocab('<start>')]]]
    for bad in refused:
        said = []
        for pack in (pack_constraints, pack_phrases):
            with pytest.raises(ValueError) as err:
                pack(bad, vocab)
            said.append(str(err.value))
        assert said[0] == said[1], said


@pytest.mark.parametrize('C', [0, 1, 3])
@pytest.mark.parametrize('W', [1, 2])
def test_the_word_count_of_met_is_phrases_met(C, W):
    """what `constrained_nbest` counts on a (B, C, W) tensor is `phrases_met` of the same words as one-word phrases, and both are
    the count by a loop; with -1 padding, ids outside the vocabulary and a constraint without a valid word"""
    from dlsg_amd.beam import _constraints_met
    B, k, L, V = 3, 3, 8, 12
    gen = torch.Generator().manual_seed(10 * C + W)
    ids = torch.randint(0, V, (B, k, L), generator=gen)
    cons = torch.randint(-1, V + 2, (B, C, W), generator=gen)
    if C:
        cons[1, 0] = torch.tensor([-1, V + 1][:W])
        cons[0, C - 1, 0] = ids[0, 1, 3]
    got = _constraints_met(ids, cons, V)
    assert got.shape == (B, k) and got.dtype == torch.int64
    assert torch.equal(got, phrases_met(ids, cons.unsqueeze(3), V))
    want = [[sum(any(0 <= a < V and a in row for a in con) for con in clip) for row in rows] for rows, clip in zip(ids.tolist(), cons.tolist())]
    assert got.tolist() == want
    assert C == 0 or 0 < sum(map(sum, want)) < B * k * C


class Logged(PhraseEmul):
    """PhraseEmul that notes the name of every op called"""
    def __init__(self):
        super().__init__()
        self.log = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if not name.startswith('_') and callable(v) and name != 'log':
            object.__getattribute__(self, 'log').append(name)
        return v


def test_the_dispatch():
    """a string with whitespace, or a 4-D tensor, runs the phrase launch; everything else the launches it always ran: the phrase
    search's log is the word search's with beam_select_phrases in place of beam_select_cons"""
    net, _, frames, regions = synth_pair(SEED, 2, ops=Logged())
    w = net.decoder.vocab.idx2word

    def log_of(cons):
        net.ops.log.clear()
        out = net.constrained_beam_search(frames, regions, cons, beam_size=3)
        return list(net.ops.log), out
    words, out_w = log_of([[w[10], [w[11], 12]], [(13, 14)]])
    assert 'beam_select_cons' in words and 'beam_select_phrases' not in words
    assert log_of(pack_constraints([[w[10], [w[11], 12]], [(13, 14)]], net.decoder.vocab))[0] == words
    for cons in ([[w[10] + ' ' + w[11]], [13]], pack_phrases([[10, [11, 12]], [[13, 14]]], net.decoder.vocab)):
        got, _ = log_of(cons)
        assert 'beam_select_phrases' in got and [nm.replace('beam_select_phrases', 'beam_select_cons') for nm in got] == words
    # one-word phrases as a 4-D tensor: the captions of the word search
    _, out_p = log_of(pack_phrases([[w[10], [w[11], 12]], [[13, 14]]], net.decoder.vocab))
    assert all(torch.equal(a, b) for a, b in zip(out_p, out_w))
    assert net.ops.log.count('beam_select_phrases') == net.decoder.max_words


def test_option_checks():
    ok = torch.full((4, 2, 3, 2), -1, dtype=torch.int64)
    cpu = torch.device('cpu')
    assert check_phrase_options(5, 26, 4, ok, cpu) == 5 and check_phrase_options(5, 26, 4, ok, cpu, n_best=2) == 2
    for bad in (ok.int(), ok[0], ok[:3], torch.full((4, 9, 1, 1), -1), torch.full((4, 2, 9, 1), -1), torch.full((4, 2, 2, 5), -1),
                torch.full((4, 2, 2, 0), -1), ok.tolist(), None):
        with pytest.raises(ValueError):
            check_phrase_options(5, 26, 4, bad, cpu)
    with pytest.raises(ValueError, match='do not fit'):
        check_phrase_options(5, 8, 4, torch.full((4, 8, 1, 1), -1), cpu)
    assert check_phrase_options(5, 9, 4, torch.full((4, 8, 1, 4), -1), cpu) == 5     # a tensor: only C + 1 <= max_words is checked
    with pytest.raises(ValueError, match='constraints on'):
        check_phrase_options(5, 26, 4, ok, torch.device('meta'))
    # lists: C_b * n_max_b + 1 <= max_words (26 here), per clip
    net, _, frames, regions = synth_pair(11, 2, ops=PhraseEmul())
    fits = [[(10 + c, 20 + c, 30 + c) for c in range(8)] + [], [(10, 11, 12, 13)]]         # 8 * 3 + 1 = 25, 1 * 4 + 1
    assert net.constrained_beam_search(frames, regions, [[' '.join(net.decoder.vocab.idx2word[i] for i in a) for a in clip]
                                                         for clip in fits], beam_size=2)[0].shape == (2, 2, 26)
    tight = [['%s %s' % tuple(net.decoder.vocab.idx2word[i] for i in (10, 11))], [(10 + c, 20 + c, 30 + c, 40 + c) for c in range(7)]]
    with pytest.raises(ValueError, match='clip 1: 7 phrase constraints of up to 4 words'):
        net.constrained_beam_search(frames, regions, tight, beam_size=2)
    with pytest.raises(ValueError):
        net.constrained_beam_search(frames, regions, [['a b']], beam_size=2)


def test_phrases_met_against_a_loop():
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 6, (5, 3, 12), generator=gen)
    phr = torch.randint(-1, 7, (5, 4, 3, 3), generator=gen)
    phr[4] = -1
    for V in (None, 6):
        got = phrases_met(ids, phr, V)
        assert got.shape == (5, 3) and got.dtype == torch.int64
        for b in range(5):
            alts = phrase_lists(phr[b].tolist(), 7 if V is None else V)
            for i in range(3):
                assert int(got[b, i]) == sum(any(contains(ids[b, i].tolist(), a) for a in con) for con in alts), (V, b, i)
        assert torch.equal(phrases_met(ids[:, 0], phr, V), got[:, 0])
    assert int(phrases_met(torch.tensor([[[1, 2, 3]]]), torch.tensor([[[[2, 3, 1]], [[3, -1, 1]], [[2, 3, -1]]]])).sum()) == 2
    assert dlsg_amd.phrases_met is phrases_met and dlsg_amd.pack_phrases is pack_phrases
    with pytest.raises(ValueError):
        phrases_met(ids, phr[:4])


def test_every_model_class_has_the_call():
    import inspect
    for cls in (dlsg_amd.CapGnnModel, dlsg_amd.CapBaseline1, dlsg_amd.CapBaselineModel):
        assert list(inspect.signature(cls.constrained_beam_search).parameters)[:4] == ['self', 'visual_feats', 'region_feats', 'constraints']
        assert 'phrases' in cls.constrained_beam_search.__doc__
    from dlsg_amd import abi
    assert 'dlsg_beam_select_phrases' in abi.functions and len(abi.functions['dlsg_beam_select_phrases'][1]) == 14
    assert abi.defines['DLSG_PHRASE_MAX'] == PHRASE_MAX == dlsg_amd.beam.MAX_PHRASE


def test_gather_results_with_phrases():
    net, _, frames, regions = synth_pair(SEED, 3, ops=PhraseEmul())
    w = net.decoder.vocab.idx2word
    need = {'v0': ['%s %s' % (w[20], w[21])], 'v1': [['%s %s %s' % (w[22], w[23], w[24]), w[25]], w[26]], 'v2': []}
    loader = [(frames, regions, None, ['v0', 'v1', 'v2'])]
    plain = S.gather_results(net, loader, decode=dict(beam_size=3))
    got = S.gather_results(net, loader, decode=dict(beam_size=3, constraints=lambda vids: [need[v] for v in vids]))
    assert got['v2'] == plain['v2'] and list(got) == ['v0', 'v1', 'v2']
    for vid, cons in need.items():
        for con in cons:
            assert any(' %s ' % a in ' %s ' % got[vid] for a in (con if isinstance(con, list) else [con])), (vid, got[vid])


def test_constrained_graph_fits_phrases_to_the_captured_shape():
    """the staging rule of ConstrainedBeamGraph with a 4-D static tensor, without a capture"""
    net, _, frames, regions = synth_pair(SEED, 2)
    w = net.decoder.vocab.idx2word
    graph = dlsg_amd.ConstrainedBeamGraph.__new__(dlsg_amd.ConstrainedBeamGraph)
    graph.model, graph.cons = net, torch.full((2, 2, 2, 3), -1, dtype=torch.int64)
    assert graph._fitted([['%s %s' % (w[10], w[11])], [[(11, 12, 13), 14], 15]]).tolist() == \
        [[[[10, 11, -1], [-1] * 3], [[-1] * 3] * 2], [[[11, 12, 13], [14, -1, -1]], [[15, -1, -1], [-1] * 3]]]
    assert graph._fitted([[10], [(11, 12)]]).tolist() == [[[[10, -1, -1], [-1] * 3], [[-1] * 3] * 2], [[[11, 12, -1], [-1] * 3], [[-1] * 3] * 2]]
    same = torch.full((2, 2, 2, 3), 7, dtype=torch.int64)
    assert graph._fitted(same) is same
    for bad in (torch.full((2, 2, 2), -1, dtype=torch.int64), torch.full((2, 2, 2, 2), -1, dtype=torch.int64), same.int(), [[10]],
                [[10, 11, 12], []], [[[10, 11, 12]], []], [[(10, 11, 12, 13)], []]):
        with pytest.raises(ValueError):
            graph._fitted(bad)
    graph.cons = torch.full((2, 3, 2), -1, dtype=torch.int64)            # a 3-D capture takes words, and refuses a phrase tensor
    with pytest.raises(ValueError):
        graph._fitted(torch.full((2, 3, 2, 1), -1, dtype=torch.int64))

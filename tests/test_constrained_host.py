"""CPU: lexically constrained beam search -- the emulated step (tests/emul_constrained.py) against an independent restatement on
Python lists, on the step cases that tests/test_gpu_constrained.py runs on the kernel; that those cases bite; the reduction to
`beam_select_hist` without constraints; `pack_constraints` and the option checks; and `beam.constrained_nbest` through the emulated
ops on a small host model against a restated whole search, with the properties a constrained search owes its caller."""
import functools
import heapq
import itertools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import scoring as S
from dlsg_amd.beam import check_constrained_options, pack_constraints
from emul_beam import BeamEmul, banned_classes
from emul_constrained import INF, ConsEmul
from test_beam_nbest_host import close, has_repeat, oracle_stepper, reference_rank, synth_pair, words_of
from test_sbs_host import DIMS, END, build_case, fresh, steps_of

# Ten float32 steps at the magnitudes of the step's values (the GAP of the stochastic step's tests): log-probs stay below about 40 in
# magnitude, where one float32 step is 3.8e-6
GAP = 1e-4
CW = [(0, 1), (1, 1), (3, 2), (8, 8)]
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt', 'met')


# ---------------------------------------------------------------------------------------------- step cases (shared with the GPU tests)
def step_keys(dims_list=DIMS, Ls=(26, 64)):
    """(dims, L, g, t, min_len, (C, W)) of every step case"""
    return [(dims, L, g, t, m, cw) for dims in dims_list for L in Ls for g in (0, 2) for t in steps_of(L, g) for m in (0, t + 1)
            for cw in CW]


def build_cons_case(dims, L, t, g, cw, seed, nan=True):
    """`build_case` of tests/test_sbs_host.py (a strided logit view, -inf and NaN entries, ~40 % ended rows, clip 0 ended altogether,
    the last clip live) with constraints.  One change to its logits: the step takes the log-softmax of the whole row, as
    dlsg_beam_select_hist does, so one NaN makes every value of its row NaN and the row offers nothing; build_case puts a NaN into
    every row, which would leave no live row at all.  Here the NaN stays in the last row of every odd clip but the last one (that
    path runs, and with one beam whole clips are left over) and is a finite draw elsewhere.
    The constraints of clip b, constraint c, by kind (c + b) % 8, so that small C sees every kind on some clip:
      0, 7  the best / second-best class of one of the clip's rows: inside that row's list A (de-duplication), a list-B word for the
            other rows, and -- the histories are drawn from the rows' best classes -- met by some rows and not by others;
      1, 6  a word drawn from the whole vocabulary: far down the row, reachable only through list B;
      2     the first word of the constraint before it and another one: two constraints share a word;
      3, 5  the first token of one row's history (the rows of a clip start with different tokens): met by that row only;
      4     one word whose logit is -inf in every row of the clip: a constraint that cannot be met.
    With W >= 2 the further alternatives are random words, a -1 pad and one id >= V.  Clip B - 2 (where B >= 3) has no constraint."""
    B, k, V = dims
    C, W = cw
    c = build_case(dims, L, t, g, seed)
    gen = torch.Generator().manual_seed(seed + 77)
    lg = c['lg']
    isnan = torch.isnan(lg)
    keep = torch.zeros_like(isnan)
    if nan:
        for b in range(1, B - 1, 2):
            keep[b * k + k - 1] = True
    fill = torch.randn(lg.shape, generator=gen) * 3.0
    lg[isnan & ~keep] = fill[isnan & ~keep]
    cons = torch.full((B, C, W), -1, dtype=torch.int64)
    lo = min(3, V - 1)
    x = lg[:, 1:V + 1]
    best = torch.where(torch.isnan(x), torch.full((), -INF), x).topk(min(3, V))[1]
    for b in range(B):
        if C == 0 or (B >= 3 and b == B - 2):
            continue
        for ci in range(C):
            kind = (ci + b) % 8
            r = b * k + ci % k
            rnd = [int(v) for v in torch.randint(lo, V, (W + 1,), generator=gen)]
            if kind in (0, 7):
                cand = [int(v) for v in best[r] if int(v) != END]
                first = cand[min(1 if kind == 7 else 0, len(cand) - 1)]
            elif kind == 2 and ci > 0:
                first = int(cons[b, ci - 1, 0])
            elif kind in (3, 5) and t > 0:
                first = int(c['hist'][r, 0])
            elif kind == 4:
                first = rnd[W]
                lg[b * k:(b + 1) * k, 1 + first] = -INF
            else:
                first = rnd[W]
            row = [first] + ([] if kind == 4 else rnd[1:W])
            if W >= 2 and kind != 4:
                row[W - 1] = V + 5 if ci % 2 == 0 else -1
                if W >= 4:
                    row[2] = -1
            cons[b, ci, :len(row)] = torch.tensor(row)
    c['cons'] = cons
    c['met'] = torch.zeros(B * k, dtype=torch.int32)
    return c


def run_cons(ops, c, key, cons='case'):
    dims, L, g, t, m, cw = key
    V = dims[2]
    ops.beam_select_cons(c['lg'][:, 1:V + 1], c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'], dims[1], END, c['hist'],
                         c['hout'], t, c['cons'] if isinstance(cons, str) else cons, no_repeat_ngram=g, min_len=m,
                         ended_count=c['cnt'], met_out=c['met'])


@functools.lru_cache(maxsize=None)
def emulated_step(key):
    """(inputs, emulated outputs, gap (B,), stats, input seeds tried) of a step case, computed once and never modified.  The inputs
    are seeded 100 g + t, then + 1000, + 2000 ... until at least 90 % of the clips have a gap of GAP or more in the emulation: a
    condition on the inputs, which the kernel is never asked about."""
    dims, L, g, t, m, cw = key
    emul = ConsEmul()
    for tries in itertools.count(1):
        c = build_cons_case(dims, L, t, g, cw, 100 * g + t + 1000 * (tries - 1))
        e = fresh(c)
        run_cons(emul, e, key)
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
def restated_clip_step(beams, raw, logp, t, k, end, g, min_len, sets, neighbours=True):
    """One clip's step on Python lists.  beams: [(tokens, log-prob, ended)] of the rows that are read; raw / logp: per row the values
    the classes are ranked by and their log-probs (lists of float, NaN allowed).  -> (picks [(value, parent, class, mask)] in
    output order -- fewer than k when the candidates run out --, the classes of the first row's list A, the smallest gap: of a row's
    k-th to its next unbanned value, of a constraint's best to its second-best word, of a bank's last pick to the best candidate left in it (with `neighbours`: of every pick)
    and, with `neighbours`, of any two neighbouring values of a bank and of every row's k-th, which is more than the picks rest on)"""
    C, V = len(sets), len(raw[0])
    A, Bs, masks, gap, row_gap = [], [], [], INF, {}
    for j, (toks, lp, ended) in enumerate(beams):
        mask = frozenset(c for c in range(C) if sets[c] & set(toks))
        masks.append(mask)
        if ended:
            A.append([(lp, end)] + [(-INF, q - 1 if q - 1 < end else q) for q in range(1, k)])
            Bs.append([None] * C)
            continue
        unmet = [c for c in range(C) if sets[c] and c not in mask]
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
            words = sorted((-raw[j][i], i) for i in sets[c] if i not in banned and raw[j][i] > -INF) if c in unmet else []
            if whole and len(words) > 1:
                gap = min(gap, words[1][0] - words[0][0])
            if words and words[0][1] not in offered:
                offered.add(words[0][1])
                slots.append((np.float32(np.float32(logp[j][words[0][1]]) + lp), words[0][1]))
            else:
                slots.append(None)
        Bs.append(slots)
    cands = []                                                        # in candidate-index order: (value, parent, class, mask)
    for lists in (A, Bs):
        for j, lst in enumerate(lists):
            cands += [(float(e[0]), j, e[1], masks[j] | {c for c in range(C) if e[1] in sets[c]}) for e in lst
                      if e is not None and e[0] > -INF]
    left = list(range(len(cands)))
    for bank in range(C + 1 if neighbours else 0):
        vals = sorted(cands[i][0] for i in left if len(cands[i][3]) == bank)
        gap = min([gap] + [y - x for x, y in zip(vals, vals[1:])])
    picks, last_gap = [], {}
    while len(picks) < k and left:
        for bank in range(C, -1, -1):
            inb = sorted((i for i in left if len(cands[i][3]) == bank), key=lambda i: (-cands[i][0], i))
            if inb and len(picks) < k:
                if len(inb) > 1:                                      # (the bank's last pick against its best rejected candidate:
                    last_gap[bank] = cands[inb[0]][0] - cands[inb[1]][0]      # the order among a bank's picks only breaks later ties)
                    gap = min(gap, last_gap[bank]) if neighbours else gap
                picks.append(cands[inb[0]])
                left.remove(inb[0])
    # a row's k-th against its next value: with `neighbours` always, else where the row's k-th candidate was picked
    gap = min([gap] + ([] if neighbours else list(last_gap.values())) + [v for (j, c), v in row_gap.items() if neighbours or any(p[1] == j and p[2] == c for p in picks)])
    return picks, [c for _, c in A[0]], gap


def restated_step(c, key):
    """the step case on lists, log-softmax in float64 -> (pred, new_lp, back, met, hist rows, number of <end>, gap per clip)"""
    dims, L, g, t, m, cw = key
    B, k, V = dims
    x = c['lg'][:, 1:V + 1].double().numpy()
    mx = np.nanmax(np.where(np.isinf(x), np.nan, x), axis=1, keepdims=True)
    logp = x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))
    out = dict(pred=[], nlp=[], back=[], met=[], hout=[], gap=[])
    for b in range(B):
        sets = [{int(i) for i in row if 0 <= int(i) < V} for row in c['cons'][b].tolist()]
        rows = range(b * k, b * k + (k if t else 1))
        beams = [(tuple(c['hist'][r, :t].tolist()), np.float32(c['lp'][r]) if t else np.float32(0), bool(t) and int(c['last'][r]) == END)
                 for r in rows]
        picks, first_a, gap = restated_clip_step(beams, [x[r].tolist() for r in rows], [logp[r].tolist() for r in rows], t, k, END, g,
                                                 m, sets)
        for q in range(k):
            v, j, cls, mask = picks[q] if q < len(picks) else (-INF, 0, first_a[q], ())
            out['pred'].append(cls); out['nlp'].append(v); out['back'].append(j); out['met'].append(sum(1 << i for i in mask))
            out['hout'].append(list(beams[j][0]) + [cls] + [END] * (L - t - 1))
        out['gap'].append(gap)
    return out


def close_lp(got, want, tol=1e-5):
    """`close`, which wants a finite value to scale by, or all of a clip's slots left over"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if np.isfinite(want).any():
        close(got, want, tol)
    else:
        assert np.array_equal(got, want)


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
            assert out['rows'][s].tolist() == [b * k + j for j in want['back'][s]], (key, b)
            close_lp(out['nlp'][s].numpy(), want['nlp'][s])
            compared += 1
        if all(g >= GAP for g in want['gap']):
            assert int(out['cnt']) == sum(p == END for p in want['pred']), key
    assert compared > 2000


def test_the_step_cases_bite():
    """list-B candidates are chosen, de-duplication happens, one step serves several banks, rows of a clip differ in what they have
    met, `end` is kept from rows with an unmet constraint, slots are left over -- each in many cases"""
    total = dict(list_b=0, dedup=0, multi_bank=0, end_blocked=0, leftover=0, mixed_met=0)
    for key in step_keys():
        stats = emulated_step(key)[3]
        for name in total:
            total[name] += int(stats[name] > 0)
    print(total)
    assert min(total.values()) >= 20, total


def check_step_rules(c, out, key):
    """what a step owes its inputs whatever the rounding: the parents' histories extended by the chosen word, parents inside the
    clip, no banned word and no dead logit chosen, no `end` from a live row with an unmet constraint, masks that are those of the
    new histories, and no (parent, class) twice"""
    dims, L, g, t, m, cw = key
    B, k, V = dims
    x = c['lg'][:, 1:V + 1]
    for b in range(B):
        sets = [{int(i) for i in row if 0 <= int(i) < V} for row in c['cons'][b].tolist()]
        present = sum(1 << i for i, s in enumerate(sets) if s)
        seen = set()
        for q in range(k):
            o = b * k + q
            parent, cls, lp = int(out['rows'][o]), int(out['pred'][o]), float(out['nlp'][o])
            assert parent == b * k + int(out['back'][o]) and b * k <= parent < (b + 1) * k and (t or parent == b * k), (key, o)
            h = c['hist'][parent, :t].tolist()
            assert out['hout'][o].tolist() == h + [cls] + [END] * (L - t - 1), (key, o)
            if lp == -INF:
                assert int(out['met'][o]) == 0, (key, o)
                continue
            assert lp == lp and (parent, cls) not in seen, (key, o)
            seen.add((parent, cls))
            mask = sum(1 << i for i, s in enumerate(sets) if s & set(h + [cls]))
            assert int(out['met'][o]) == mask, (key, o)
            if t and int(c['last'][parent]) == END:
                assert cls == END and lp == float(c['lp'][parent]), (key, o)
                continue
            assert cls not in banned_classes(h, t, g, m, END) and float(x[parent, cls]) > -INF, (key, o)
            assert cls != END or mask == present, (key, o)


def test_the_emulated_step_keeps_the_rules():
    for key in step_keys():
        c, out, _, _, _ = emulated_step(key)
        check_step_rules(c, out, key)


def test_without_constraints_the_step_is_beam_select_hist():
    """C = 0, cons = None and a tensor of padding only, on the step cases' inputs (without the NaN rows: BeamEmul ranks with
    torch.topk, which puts a NaN first, where the kernels never choose one)"""
    for key in step_keys(Ls=(26,)):
        dims, L, g, t, m, cw = key
        if cw != (8, 8):
            continue
        B, k, V = dims
        c = build_cons_case(dims, L, t, g, cw, 100 * g + t, nan=False)
        want = fresh(c)
        BeamEmul().beam_select_hist(want['lg'][:, 1:V + 1], want['last'], want['lp'], want['pred'], want['nlp'], want['back'],
                                    want['rows'], k, END, want['hist'], want['hout'], t, g, m, ended_count=want['cnt'])
        for cons in (None, torch.zeros(B, 0, 1, dtype=torch.int64), torch.full((B, 3, 2), -1, dtype=torch.int64),
                     torch.full((B, 2, 2), V, dtype=torch.int64)):
            got = fresh(c)
            run_cons(ConsEmul(), got, key, cons)
            real = want['nlp'] > -INF                                   # (a left-over slot names a class among -inf ties: topk's choice)
            assert torch.equal(got['nlp'], want['nlp']), key
            for o in ('pred', 'back', 'rows', 'hout'):
                assert torch.equal(got[o][real], want[o][real]), (key, o)
            assert bool(real.all()) or V == 8
            assert not bool(real.all()) or torch.equal(got['cnt'], want['cnt']), key
            assert not bool(got['met'].any())


# ---------------------------------------------------------------------------------------------- packing and option checks
def test_pack_constraints():
    vocab = dlsg_amd.make_vocab(50)
    w = vocab.idx2word
    got = pack_constraints([[w[10], [w[11], 12]], [], [[w[13], w[14], w[15]]]], vocab)
    assert got.dtype == torch.int64 and got.tolist() == [[[10, -1, -1], [11, 12, -1]], [[-1] * 3] * 2, [[13, 14, 15], [-1] * 3]]
    assert pack_constraints([[], []], vocab).shape == (2, 0, 1)
    assert pack_constraints([[7]], vocab, device='cpu').tolist() == [[[7]]]
    with pytest.raises(ValueError, match='not in the vocabulary'):
        pack_constraints([['no such word']], vocab)
    with pytest.raises(ValueError, match='not in the vocabulary'):
        pack_constraints([[50]], vocab)
    assert pack_constraints([['no such word', [w[9], 'nor this']]], vocab, skip_unknown=True).tolist() == [[[-1], [9]]]
    with pytest.raises(ValueError, match='at most 8'):
        pack_constraints([list(range(10, 19))], vocab)
    with pytest.raises(ValueError, match='at most 8'):
        pack_constraints([[list(range(10, 19))]], vocab)
    for word in ('<end>', '<start>', '<pad>'):
        with pytest.raises(ValueError, match='cannot be required'):
            pack_constraints([[[w[10], word]]], vocab)
    with pytest.raises(ValueError, match='cannot be required'):
        pack_constraints([[vocab('<end>')]], vocab)


def test_check_constrained_options_value_errors():
    ok = torch.full((4, 2, 3), -1, dtype=torch.int64)
    cpu = torch.device('cpu')
    assert check_constrained_options(5, 26, 4, ok, cpu) == 5 and check_constrained_options(5, 26, 4, ok, cpu, n_best=2) == 2
    for bad in (ok.int(), ok[0], ok[:3], torch.full((4, 9, 1), -1), torch.full((4, 2, 9), -1), ok.tolist(), None):
        with pytest.raises(ValueError):
            check_constrained_options(5, 26, 4, bad, cpu)
    with pytest.raises(ValueError, match='do not fit'):
        check_constrained_options(5, 8, 4, torch.full((4, 8, 1), -1), cpu)
    assert check_constrained_options(5, 9, 4, torch.full((4, 8, 1), -1), cpu) == 5
    with pytest.raises(ValueError, match='constraints on'):
        check_constrained_options(5, 26, 4, ok, torch.device('meta'))
    for opts in (dict(n_best=6), dict(min_len=26), dict(no_repeat_ngram=-1)):          # and what check_nbest_options refuses
        with pytest.raises(ValueError):
            check_constrained_options(5, 26, 4, ok, cpu, **opts)
    net, _, frames, regions = synth_pair(11, 2, ops=ConsEmul())
    with pytest.raises(ValueError):
        net.constrained_beam_search(frames, regions, [[10]])                           # one clip's list for two clips
    with pytest.raises(ValueError):
        net.constrained_beam_search(frames, regions, [[10], [11]], beam_size=9)


# ---------------------------------------------------------------------------------------------- the whole search
# the model: chosen by the restated search alone, so that at most one clip in six (in eight, on the GPU) has a near-tie in any of SEARCHES
SEED, BATCH, BIAS = 147, 6, 2.0


def clip_constraints(n_max, seed=5):
    """per clip 0 .. n_max constraints (clip b has b % (n_max + 1)) of 1 to 3 alternative word ids of the 50-word vocabulary"""
    rng = np.random.RandomState(seed)
    return [[[int(v) for v in rng.choice(np.arange(4, 50), size=1 + (b + c) % 3, replace=False)] for c in range(b % (n_max + 1))]
            for b in range(BATCH)]


def reference_constrained_search(step_fn, start, state, end, L, k, g, min_len, per_clip):
    """`reference_search` of tests/test_beam_nbest_host.py with the constrained step: every step of the search on Python lists"""
    B = start.numel()
    sets = [[set(con) for con in clip] for clip in per_clip]
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
            picks, _, gp = restated_clip_step(beams[b], rows, rows, t, k, end, g, min_len, sets[b], neighbours=False)
            assert len(picks) == k
            gap[b] = min(gap[b], gp)
            parents += [b * n + j for _, j, _, _ in picks]
            beams[b] = [(beams[b][j][0] + (cls,), np.float32(v), cls == end) for v, j, cls, _ in picks]
        idx = torch.tensor(parents)
        state = {key: v[idx] for key, v in state.items()}
        last = torch.tensor([bm[0][-1] for bs in beams for bm in bs])
    return [[list(bm[0]) for bm in bs] for bs in beams], [[bm[1] for bm in bs] for bs in beams], gap


def count_met(row, clip, end):
    return sum(bool(set(con) & set(words_of(row, end))) for con in clip)


@functools.lru_cache(maxsize=None)
def restated_search(k, g, min_len, alpha, n_max):
    """(ids, scores, lens, met, gap) by lists alone: the search, the ranking by score, then the stable sort by constraints met"""
    net, orc, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS)
    per_clip = clip_constraints(n_max)
    step_fn, start, state, end, L = oracle_stepper(orc, frames, regions)
    toks, lps, gap = reference_constrained_search(step_fn, start, state, end, L, k, g, min_len, per_clip)
    ids, sc, ln, rank_gap = reference_rank(toks, lps, end, alpha, k)
    out = [], [], [], []
    for b in range(BATCH):
        met = [count_met(row, per_clip[b], end) for row in ids[b]]
        order = sorted(range(k), key=lambda i: (-met[i], i))
        for dst, src in zip(out, (ids[b], sc[b], ln[b], met)):
            dst.append([src[i] for i in order])
    return out + ([min(a, b) for a, b in zip(gap, rank_gap)],)


@functools.lru_cache(maxsize=None)
def emulated_search(k, g, min_len, alpha, n_max):
    net, orc, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ConsEmul())
    return net.constrained_beam_search(frames, regions, clip_constraints(n_max), beam_size=k, length_penalty=alpha, no_repeat_ngram=g,
                                       min_len=min_len, return_met=True)


SEARCHES = [(1, 0, 0, 0.0, 3), (3, 2, 4, 0.7, 3), (5, 0, 0, 0.7, 3), (5, 3, 4, 0.0, 3), (5, 2, 0, 1.0, 2)]


@pytest.mark.parametrize('k,g,min_len,alpha,n_max', SEARCHES)
def test_constrained_nbest_matches_the_restated_search(k, g, min_len, alpha, n_max):
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


@pytest.mark.parametrize('k,g,min_len,alpha,n_max', SEARCHES)
def test_constrained_search_properties(k, g, min_len, alpha, n_max):
    check_search_properties(*emulated_search(k, g, min_len, alpha, n_max), clip_constraints(n_max), END, g, min_len)


def check_search_properties(ids, scores, lens, met, per_clip, end, g, min_len):
    """a row with met == C_b holds a word of every set; row 0 meets every constraint; a row that ends before L has met them all;
    rows in order of met, then score; no repeated g-gram, at least min_len words, <end>-padded"""
    ids, scores, lens, met = ids.cpu(), scores.cpu(), lens.cpu(), met.cpu()
    B, n, L = ids.shape
    for b in range(B):
        Cb = len(per_clip[b])
        assert int(met[b, 0]) == Cb, b
        for i in range(n):
            row = ids[b, i].tolist()
            words = words_of(row, end)
            assert int(met[b, i]) == count_met(row, per_clip[b], end) <= Cb, (b, i)
            assert len(words) == L or int(met[b, i]) == Cb, (b, i)
            assert int(lens[b, i]) == min(len(words) + 1, L)
            assert (g == 0 or not has_repeat(words, g)) and len(words) >= min_len and all(w == end for w in row[len(words):]), (b, i)
        for i in range(n - 1):
            assert (int(met[b, i]), float(scores[b, i])) >= (int(met[b, i + 1]), float(scores[b, i + 1])), (b, i)


def test_constraints_change_the_search():
    """vacuity guard: the unconstrained best caption meets every constraint in fewer than half of the constrained clips"""
    per_clip = clip_constraints(3)
    net, _, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ConsEmul())
    free = net.beam_search(frames, regions, beam_size=5, n_best=1)[0][:, 0]
    have = [b for b in range(BATCH) if per_clip[b]]
    assert 2 * sum(count_met(free[b].tolist(), per_clip[b], END) == len(per_clip[b]) for b in have) < len(have)


@pytest.mark.parametrize('k', [1, 3, 5])
def test_empty_constraints_give_the_bits_of_beam_nbest(k):
    net, _, frames, regions = synth_pair(SEED, BATCH, end_bias=BIAS, ops=ConsEmul())
    opts = dict(beam_size=k, length_penalty=0.7, no_repeat_ngram=2, min_len=3)
    want = net.beam_search(frames, regions, **opts)
    for cons in ([[]] * BATCH, torch.full((BATCH, 2, 3), -1, dtype=torch.int64)):
        got = dlsg_amd.constrained_beam_search(net, frames, regions, cons, **opts)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(net.constrained_beam_search(frames, regions, [[]] * BATCH, n_best=1, **opts),
                                                 net.beam_search(frames, regions, n_best=1, **opts)))


def test_every_model_class_has_the_call_and_the_others_keep_their_signatures():
    import inspect
    for cls in (dlsg_amd.CapGnnModel, dlsg_amd.CapBaseline1, dlsg_amd.CapBaselineModel):
        assert list(inspect.signature(cls.constrained_beam_search).parameters)[:4] == ['self', 'visual_feats', 'region_feats', 'constraints']
        assert 'constraints' not in inspect.signature(cls.beam_search).parameters
    from dlsg_amd import abi
    assert 'dlsg_beam_select_cons' in abi.functions and len(abi.functions['dlsg_beam_select_cons'][1]) == 12


def test_gather_results_constraints_option():
    net, _, frames, regions = synth_pair(SEED, 3, ops=ConsEmul())
    vocab = net.decoder.vocab
    need = {'v0': [vocab.idx2word[20]], 'v1': [[vocab.idx2word[21], vocab.idx2word[22]], vocab.idx2word[23]], 'v2': []}
    loader = [(frames, regions, None, ['v0', 'v1', 'v2'])]
    plain = S.gather_results(net, loader, decode=dict(beam_size=3))
    got = S.gather_results(net, loader, decode=dict(beam_size=3, constraints=lambda vids: [need[v] for v in vids]))
    assert got['v2'] == plain['v2'] and list(got) == ['v0', 'v1', 'v2']
    for vid, cons in need.items():
        for con in cons:
            assert set(con if isinstance(con, list) else [con]) & set(got[vid].split()), (vid, got[vid])
    assert plain == S.gather_results(net, loader, decode=dict(beam_size=3, n_best=1))


def test_constrained_graph_fits_constraints_to_the_captured_shape():
    """the staging rule of ConstrainedBeamGraph, without a capture: lists are packed and padded to the captured (B, C, W), a tensor
    of another shape or dtype raises"""
    net, _, frames, regions = synth_pair(SEED, 2)
    graph = dlsg_amd.ConstrainedBeamGraph.__new__(dlsg_amd.ConstrainedBeamGraph)
    graph.model, graph.cons = net, torch.full((2, 3, 2), -1, dtype=torch.int64)
    assert graph._fitted([[10], [[11, 12], 13]]).tolist() == [[[10, -1], [-1, -1], [-1, -1]], [[11, 12], [13, -1], [-1, -1]]]
    same = torch.full((2, 3, 2), 7, dtype=torch.int64)
    assert graph._fitted(same) is same
    for bad in (torch.full((2, 2, 2), -1, dtype=torch.int64), same.int(), [[10]], [[10, 11, 12, 13], []], [[[10, 11, 12]], []]):
        with pytest.raises(ValueError):
            graph._fitted(bad)


class ReplayStub(object):
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append('replay')


def hand_built_graph(cls, net, frames, regions, log, **extra):
    """a graph object of `cls` without a capture: zeroed static inputs, the extra buffer given, a `graph` that notes its replays"""
    graph = cls.__new__(cls)
    graph.model, graph.held = net, []
    graph.frames, graph.regions = torch.zeros_like(frames), torch.zeros_like(regions)
    graph.graph, graph.out = ReplayStub(log), ('the', 'outputs')
    for name, buf in extra.items():
        setattr(graph, name, buf)
    return graph


def test_the_graph_base_stages_the_extra_static_input(monkeypatch):
    """_SeededGraph, ConstrainedBeamGraph and ScoreGraph replay through the one `__call__` of their base: a call copies frames,
    regions and the third input into their buffers, each once and before the replay, and returns `out`; an input that does not fit
    raises the class's message and copies nothing"""
    from dlsg_amd import graphs, hip
    net, _, frames, regions = synth_pair(SEED, 2)
    log, live = [], []

    def noting(copy):
        def noted(dst, src, *rest):
            g = live[0]
            log.append([nm for nm in ('frames', 'regions', g.extra) if getattr(g, nm) is dst][0])
            return copy(dst, src, *rest)
        return noted
    monkeypatch.setattr(graphs, 'stage', noting(graphs.stage))
    monkeypatch.setattr(hip, 'copy_to_device', noting(hip.copy_to_device))
    ids = torch.arange(30).view(2, 3, 5)
    cases = [(dlsg_amd.StochasticBeamGraph, 'seed', torch.zeros(1, dtype=torch.int64), 7, torch.tensor([7])),
             (dlsg_amd.SampleGraph, 'seed', torch.zeros(1, dtype=torch.int64), torch.tensor(9), torch.tensor([9])),
             (dlsg_amd.ConstrainedBeamGraph, 'cons', torch.full((2, 3, 2), -1, dtype=torch.int64), [[10], [[11, 12], 13]],
              torch.tensor([[[10, -1], [-1, -1], [-1, -1]], [[11, 12], [13, -1], [-1, -1]]])),
             (dlsg_amd.ConstrainedBeamGraph, 'cons', torch.full((2, 1, 1, 2), -1, dtype=torch.int64), torch.tensor([[[[4, 5]]], [[[6, -1]]]]),
              torch.tensor([[[[4, 5]]], [[[6, -1]]]])),
             (dlsg_amd.ScoreGraph, 'ids', torch.zeros(2, 3, 5, dtype=torch.int64), ids, ids)]
    for cls, name, buf, value, want in cases:
        assert cls.extra == name
        graph = hand_built_graph(cls, net, frames, regions, log, **{name: buf})
        live[:] = [graph]
        del log[:]
        assert graph(frames, regions, value) is graph.out
        assert log == ['frames', 'regions', name, 'replay'], (cls.__name__, log)
        assert torch.equal(graph.frames, frames) and torch.equal(graph.regions, regions) and torch.equal(getattr(graph, name), want)
        assert getattr(graph, name) is buf
        del log[:]
        for args in ((frames, regions), (frames, regions, value, value)):
            with pytest.raises(TypeError):
                graph(*args)
        assert log == []
    refusals = [(dlsg_amd.ConstrainedBeamGraph, 'cons', torch.full((2, 3, 2), -1, dtype=torch.int64), torch.full((2, 2, 2), 5, dtype=torch.int64),
                 'ConstrainedBeamGraph: constraints of shape (2, 2, 2) torch.int64 on cpu, captured with (2, 3, 2) int64 on cpu -- build a new graph'),
                (dlsg_amd.ConstrainedBeamGraph, 'cons', torch.full((2, 3, 2), -1, dtype=torch.int64), torch.full((2, 3, 2, 1), 5, dtype=torch.int64),
                 'ConstrainedBeamGraph: constraints of shape (2, 3, 2, 1) torch.int64 on cpu, captured with (2, 3, 2) int64 on cpu -- build a new graph'),
                (dlsg_amd.ScoreGraph, 'ids', torch.zeros(2, 3, 5, dtype=torch.int64), ids[:, :2],
                 'ScoreGraph: ids of shape (2, 2, 5) torch.int64 on cpu, captured with (2, 3, 5) int64 on cpu -- build a new graph'),
                (dlsg_amd.ScoreGraph, 'ids', torch.zeros(2, 3, 5, dtype=torch.int64), ids.int(),
                 'ScoreGraph: ids of shape (2, 3, 5) torch.int32 on cpu, captured with (2, 3, 5) int64 on cpu -- build a new graph')]
    for cls, name, buf, value, message in refusals:
        graph = hand_built_graph(cls, net, frames, regions, log, **{name: buf})
        live[:] = [graph]
        kept = buf.clone()
        del log[:]
        with pytest.raises(ValueError) as err:
            graph(frames, regions, value)
        assert str(err.value) == message
        assert log == [] and torch.equal(buf, kept) and not bool(graph.frames.any())
    with pytest.raises(ValueError, match='takes no lens'):
        dlsg_amd.ScoreGraph(net, frames, regions, ids, lens=None)

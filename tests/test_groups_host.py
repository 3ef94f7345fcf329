"""CPU: diverse (group) beam search -- `num_groups` / `diversity_penalty` of `beam_search` -- through the emulated step
(tests/emul_groups.py) against `group_search`, a list-based restatement of the whole search over the oracles' ensemble
step of tests/test_ensemble_host.py; the step cases that tests/test_gpu_groups.py runs on the kernel,
checked here on the emulator alone so that they leave few clips out and the penalty bites; and the public forms."""
import functools

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd.synth import synth_batch, synth_state_dict
from emul_beam import banned_classes
from emul_groups import GroupsEmul
from test_beam_nbest_host import MODELS, close, reference_rank, reference_search, synth_pair
from test_ensemble_host import CLIPS, NEAR_TIE, SETTINGS, build_members, ensemble_stepper, member_specs
from test_gpu_beam_nbest import END, check_properties, step_case, steps_of

INF = float('inf')
DIMS = [(3, 4, 50), (7, 6, 1000), (4, 8, 10007), (2, 2, 40)]
# Ten times the float32 error of a key.  Finite penalties are at most 2.0 and a class is counted at most k - k' <= 7 times, so with
# log-probs down to about -25 a key stays below 40 in magnitude, where one float32 step is 3.8e-6 and a key is a few roundings.
GAP = 1e-4
PENALTIES = (0.5, 2.0, INF)
ENSEMBLES = {1: [1.0], 3: [1.0, 1.0, 1.0]}
OUTPUTS = ('pred', 'nlp', 'back', 'rows', 'hout', 'cnt')


# ---------------------------------------------------------------------------------------------- step cases (shared with the GPU tests)
def step_keys():
    """(dims, G, L, g, t, min_len) of every step case: every divisor G > 1 of k"""
    return [(dims, G, L, g, t, m) for dims in DIMS for G in range(2, dims[1] + 1) if dims[1] % G == 0
            for L in (26, 64) for g in (0, 2) for t in steps_of(L, g) for m in (0, t + 1)]


def base_case(key):
    dims, G, L, g, t, m = key
    return step_case(dims, L, t, g, 100 * g + t)


def member_logits(key, M):
    """member m's logits: those of the step case with seed 100 g + t + 1000 m"""
    dims, G, L, g, t, m = key
    return [step_case(dims, L, t, g, 100 * g + t + 1000 * i)['lg'] for i in range(M)]


def run_groups(ops, c, lgs, weights, mode, key, penalty, G=None):
    dims, G_, L, g, t, m = key
    V = dims[2]
    ops.beam_select_groups([x[:, 1:V + 1] for x in lgs], weights, mode, c['last'], c['lp'], c['pred'], c['nlp'], c['back'], c['rows'],
                           dims[1], END, c['hist'], c['hout'], t, g, m, G_ if G is None else G, penalty, ended_count=c['cnt'])


@functools.lru_cache(maxsize=None)
def emulated_steps(mode, M, penalty):
    """the emulator on every step case of one (mode, M, penalty), computed once and never modified:
    {key: (outputs, gap (B,), [(clip, group, changed by the penalty)])}"""
    emul, out = GroupsEmul(), {}
    for key in step_keys():
        c = base_case(key)
        run_groups(emul, c, member_logits(key, M), ENSEMBLES[M], mode, key, penalty)
        out[key] = ({o: c[o] for o in OUTPUTS}, emul.gap, emul.changed)
    return out


@pytest.mark.parametrize('penalty', PENALTIES)
@pytest.mark.parametrize('M', list(ENSEMBLES))
@pytest.mark.parametrize('mode', [0, 1])
def test_step_cases_leave_few_clips_out_and_the_penalty_bites(mode, M, penalty):
    """on the emulator alone, over all step cases of a (mode, M, penalty): at most 10 % of the clips have a gap below GAP, and at
    least 10 % of the groups after the first choose differently than they would with penalty 0"""
    steps = emulated_steps(mode, M, penalty)
    gaps = torch.cat([gap for _, gap, _ in steps.values()])
    out = int((gaps < GAP).sum())
    changed = [c for _, _, ch in steps.values() for _, _, c in ch]
    print('mode %d M %d penalty %g: %d of %d clips below %g, %d of %d later groups changed'
          % (mode, M, penalty, out, gaps.numel(), GAP, sum(changed), len(changed)))
    assert gaps.numel() == 1148 and 10 * out <= gaps.numel()
    assert 10 * sum(changed) >= len(changed) > 0


def test_the_emulated_step_keeps_the_rules():
    """the emulator against the rules it restates, read off its outputs: parents inside the group, new_lp without the penalty
    (it is a candidate's lp), nothing banned, and with penalty inf no word from a live parent twice across groups"""
    for key, (out, gap, _) in emulated_steps(0, 1, INF).items():
        check_step_rules(base_case(key), out, key, exclusive=True)


def check_step_rules(c, out, key, exclusive):
    dims, G, L, g, t, m = key
    B, k, V = dims
    kg = k // G
    for b in range(B):
        seen = set()
        for y in range(G):
            mine = set()
            for q in range(kg):
                o = b * k + y * kg + q
                parent = int(out['rows'][o])
                assert parent == b * k + int(out['back'][o]) and b * k + y * kg <= parent < b * k + (y + 1) * kg, (key, o)
                live = t == 0 or int(c['last'][parent]) != END
                cls, lp = int(out['pred'][o]), float(out['nlp'][o])
                if live and lp > -INF:
                    assert cls not in banned_classes(c['hist'][parent, :t].tolist(), t, g, m, END), (key, o)
                    assert not exclusive or cls not in seen, (key, o, cls)
                    mine.add(cls)
                elif lp > -INF:
                    assert cls == END                                   # an ended beam goes on with <end>
            seen |= mine


# ---------------------------------------------------------------------------------------------- the whole search, restated with lists
def group_search(step_fn, start, state, end, L, k, G, penalty, g=0, min_len=0):
    """`reference_search` of tests/test_beam_nbest_host.py with beam groups: per clip every live beam offers its k best unbanned
    classes, an ended beam <end> at 0; the groups choose in order, each its k / G best keys among its own beams' candidates (step 0:
    the one beam's), key = value - penalty * (number of picks of that class by earlier groups at this step from live beams) for a
    live parent, float32; the new beam keeps the value.  Returns (tokens [B][k][L], log-probs [B][k], gap [B]: the smallest
    difference over steps and groups between the last chosen key and the best rejected one)."""
    B, kg = start.numel(), k // G
    beams = [[dict(toks=[], lp=np.float32(0.0))] for _ in range(B)]
    gap = [INF] * B
    last = start
    for t in range(L):
        n = len(beams[0])
        logp, state = step_fn(last, state)
        logp = logp.numpy()
        parents = []
        for b in range(B):
            lists = []                                                       # per beam: [(value, parent, class, live)]
            for j, bm in enumerate(beams[b]):
                if bm['toks'] and bm['toks'][-1] == end:
                    lists.append([(bm['lp'], j, end, False)])
                    continue
                banned = banned_classes(bm['toks'], t, g, min_len, end)
                row = logp[b * n + j]
                order = sorted((c for c in range(row.shape[0]) if c not in banned), key=lambda c: (-row[c], c))[:k]
                lists.append([(np.float32(row[c] + bm['lp']), j, c, True) for c in order])
            cnt, new = {}, []
            for y in range(G):
                cands = [c for j in (range(y * kg, (y + 1) * kg) if t else [0]) for c in lists[j]]
                keys = [v if not live or not cnt.get(c, 0) else np.float32(v - np.float32(penalty * cnt[c])) for v, j, c, live in cands]
                ranked = [i for i in sorted(range(len(cands)), key=lambda i: (-keys[i], i)) if keys[i] > -INF]
                assert len(ranked) >= kg
                if len(ranked) > kg:
                    gap[b] = min(gap[b], float(keys[ranked[kg - 1]]) - float(keys[ranked[kg]]))
                for i in ranked[:kg]:
                    v, j, c, live = cands[i]
                    new.append(dict(toks=beams[b][j]['toks'] + [c], lp=v))
                    parents.append(b * n + j)
                for i in ranked[:kg]:
                    if cands[i][3]:
                        cnt[cands[i][2]] = cnt.get(cands[i][2], 0) + 1
            beams[b] = new
        idx = torch.tensor(parents)
        state = {key: v[idx] for key, v in state.items()}
        last = torch.tensor([bm['toks'][-1] for bs in beams for bm in bs])
    return [[bm['toks'] for bm in bs] for bs in beams], [[bm['lp'] for bm in bs] for bs in beams], gap


# The cases: the three small members of tests/test_ensemble_host.py (vocabulary 50, <end> lifted by 1.0, 8 clips) as an ensemble in
# both modes, with that file's weights, and the issue's penalty 0.5.  A grouped search has G boundaries per word where a plain one has
# one, and these members' combined distributions are flat, so with that file's own seed 15 three to six clips of eight have a gap
# below NEAR_TIE somewhere.  The seeds were searched (0 .. 699, every case on its own, the restatement alone): 104 leaves 8, 7 and 7
# clips in for the first three cases and 5 for the last, 169 leaves 7 in for the last.
ALPHA, NGRAM, MIN_LEN = 0.7, 2, 4
PENALTY = 0.5
SEARCHES = {'k4g2': dict(beam_size=4, num_groups=2), 'k6g3': dict(beam_size=6, num_groups=3)}
SEEDS = {('k4g2', 'prob'): 104, ('k4g2', 'logprob'): 104, ('k6g3', 'prob'): 104, ('k6g3', 'logprob'): 169}


def build_seeded(seed, ops=None, oracles=False):
    """`build_members` of tests/test_ensemble_host.py -- the same three configurations and the same lift of <end> -- with the
    members' weights seeded seed, seed + 1000, seed + 2000 and the clips seed + 1: (nets or oracles, frames, regions)"""
    vocab = dlsg_amd.make_vocab(50)
    out = []
    for i, (kind, args, _) in enumerate(member_specs()):
        torch.manual_seed(0)
        net = MODELS[kind][0](args, vocab).eval()
        sd = synth_state_dict(net.state_dict(), seed + 1000 * i)
        sd['decoder.word_restore.bias'][net.decoder.vocab('<end>')] += 1.0
        if oracles:
            net = MODELS[kind][1](args, vocab).eval()
        net.load_state_dict(sd)
        if ops is not None:
            net.set_ops(ops)
        out.append(net)
    frames, regions, _, _ = synth_batch(member_specs()[0][1], 50, CLIPS, seed + 1)
    return out, frames, regions


def search_opts(name):
    return dict(SEARCHES[name], diversity_penalty=PENALTY, length_penalty=ALPHA, no_repeat_ngram=NGRAM, min_len=MIN_LEN)


@functools.lru_cache(maxsize=None)
def restated(name, setting):
    """the restated grouped search of a (search, ensemble setting), computed once and never modified: ids, scores, lens, gap per
    clip, end, L, and the ids of the plain search with as many beams"""
    k, G = SEARCHES[name]['beam_size'], SEARCHES[name]['num_groups']
    orcs, frames, regions = build_seeded(SEEDS[name, setting], oracles=True)
    step_fn, start, state, end, L = ensemble_stepper(orcs, SETTINGS[setting], setting, frames, regions)
    toks, lps, gap = group_search(step_fn, start, state, end, L, k, G, PENALTY, NGRAM, MIN_LEN)
    ids, sc, lens, rank_gap = reference_rank(toks, lps, end, ALPHA, k)
    ptoks, plps, _ = reference_search(step_fn, start, state, end, L, k, NGRAM, MIN_LEN)
    plain = reference_rank(ptoks, plps, end, ALPHA, k)[0]
    return ids, sc, lens, [min(a, b) for a, b in zip(gap, rank_gap)], end, L, plain


def kept(name, setting):
    return [b for b in range(CLIPS) if restated(name, setting)[3][b] >= NEAR_TIE]


def check_against_restated(name, setting, ids, scores, lens):
    """what both the emulated and the HIP search owe the restatement: kept clips exact (scores to 1e-4), every clip well-formed"""
    want_ids, want_sc, want_len, gap, end, L, _ = restated(name, setting)
    k = SEARCHES[name]['beam_size']
    assert ids.shape == (CLIPS, k, L) and scores.shape == (CLIPS, k) and lens.shape == (CLIPS, k)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and lens.dtype == torch.int64
    for b in kept(name, setting):
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b], b
        close(scores[b].numpy(), want_sc[b], 1e-4)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    check_properties(ids, end, NGRAM, MIN_LEN)


CASES = [(name, setting) for name in SEARCHES for setting in SETTINGS]


@pytest.mark.parametrize('name, setting', CASES)
def test_restated_case_is_decisive_and_diverse(name, setting):
    """on the restatement alone: at most one clip in eight is a near-tie, and in at least half of the clips the grouped n-best set
    is not the plain n-best set of as many beams"""
    ids, _, _, gap, end, L, plain = restated(name, setting)
    differ = sum({tuple(r) for r in ids[b]} != {tuple(r) for r in plain[b]} for b in range(CLIPS))
    print(name, setting, 'smallest gaps', ['%.1e' % x for x in gap], 'sets differ in', differ)
    assert len(kept(name, setting)) >= CLIPS - 1
    assert 2 * differ >= CLIPS


@functools.lru_cache(maxsize=None)
def emulated(name, setting):
    nets, frames, regions = build_seeded(SEEDS[name, setting], ops=GroupsEmul())
    return dlsg_amd.Ensemble(nets, SETTINGS[setting], setting).beam_search(frames, regions, **search_opts(name))


@pytest.mark.parametrize('name, setting', CASES)
def test_grouped_search_matches_the_restated_search(name, setting):
    check_against_restated(name, setting, *emulated(name, setting))


# ---------------------------------------------------------------------------------------------- penalty 0 and the public forms
@pytest.mark.parametrize('k, G', [(4, 2), (6, 3), (6, 6)])
def test_penalty_zero_repeats_the_smaller_search(k, G):
    """num_groups = G without a penalty: every group runs the beam_size = k / G search, so each of its hypotheses comes G times"""
    net, orc, frames, regions = synth_pair(11, 6, ops=GroupsEmul())
    opts = dict(length_penalty=ALPHA, no_repeat_ngram=NGRAM, min_len=MIN_LEN)
    ids, scores, lens = net.beam_search(frames, regions, beam_size=k, num_groups=G, diversity_penalty=0.0, **opts)
    # the smaller search through the emulation of dlsg_beam_select_ens, whose float64 arithmetic the grouped emulation shares
    # (that of dlsg_beam_select_hist works in float32: its scores differ in the last bits, on the emulators only)
    want = dlsg_amd.Ensemble([net]).beam_search(frames, regions, beam_size=k // G, **opts)
    for i in range(k):
        assert torch.equal(ids[:, i], want[0][:, i // G]) and torch.equal(lens[:, i], want[2][:, i // G]), i
    assert torch.equal(scores[:, ::G], want[1])
    own = net.beam_search(frames, regions, beam_size=k // G, **opts)
    assert torch.equal(own[0], want[0]) and torch.equal(own[2], want[2])
    close(own[1].numpy(), want[1].numpy(), 1e-6)


def test_one_group_is_todays_search_launch_for_launch():
    from launch_trace import fresh, traced
    opts = dict(beam_size=3, n_best=2, length_penalty=ALPHA, no_repeat_ngram=NGRAM, min_len=2)
    out, traces = [], []
    for kw in (dict(), dict(num_groups=1), dict(num_groups=1, diversity_penalty=0.0)):
        net, args, vocab, frames, regions, caps, lens = fresh('capgnn')      # (a fresh net each: a call moves the dropout seed on)
        traces.append(traced(net, lambda: out.append(net.beam_search(frames, regions, **dict(opts, **kw)))))
    assert traces[0] == traces[1] == traces[2] and 'beam_select_hist' in {c[0] for c in traces[0]}
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(*out))
    nets, frames, regions = build_members(ops=GroupsEmul())
    ens = dlsg_amd.Ensemble(nets, SETTINGS['prob'], 'prob')
    opts = dict(beam_size=3, length_penalty=ALPHA, no_repeat_ngram=NGRAM, min_len=MIN_LEN)
    a, b = ens.beam_search(frames, regions, **opts), ens.beam_search(frames, regions, num_groups=1, **opts)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('mode', ['prob', 'logprob'])
def test_an_ensemble_of_one_is_the_models_grouped_search(mode):
    net, orc, frames, regions = synth_pair(11, 6, ops=GroupsEmul())
    opts = dict(beam_size=6, num_groups=3, diversity_penalty=PENALTY, length_penalty=ALPHA, no_repeat_ngram=NGRAM, min_len=MIN_LEN)
    want = net.beam_search(frames, regions, **opts)
    got = dlsg_amd.Ensemble([net], mode=mode).beam_search(frames, regions, **opts)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    close(got[1].numpy(), want[1].numpy(), 1e-6)
    plain = net.beam_search(frames, regions, beam_size=6, length_penalty=ALPHA, no_repeat_ngram=NGRAM, min_len=MIN_LEN)
    assert not torch.equal(plain[0], want[0])
    assert net.decoder.beam_size == 5


def test_evaluate_and_gather_results_take_the_keywords():
    from dlsg_amd import scoring as S
    net, orc, frames, regions = synth_pair(11, 3, ops=GroupsEmul())
    loader = [(frames, regions, None, ['v0', 'v1', 'v2'])]
    opts = dict(beam_size=6, num_groups=3, diversity_penalty=0.5)
    got = S.gather_results(net, loader, decode=opts)
    ids = net.beam_search(frames, regions, n_best=1, **opts)[0][:, 0]
    assert got == {'v%d' % i: net.decoder.decode_tokens(ids[i]) for i in range(3)}
    refs = {'v%d' % i: [{u'video_id': 'v%d' % i, u'cap_id': 0, u'caption': got['v%d' % i]}] for i in range(3)}
    scores, result = S.evaluate(net, loader, refs, decode=opts)
    assert result == got and scores['Bleu_1'] == pytest.approx(1.0)


def test_value_errors():
    net, orc, frames, regions = synth_pair(11, 2, ops=GroupsEmul())
    ens = dlsg_amd.Ensemble([net])
    for bad in (dict(beam_size=6, num_groups=4), dict(beam_size=6, num_groups=0), dict(beam_size=6, num_groups=-2),
                dict(beam_size=4, num_groups=8), dict(beam_size=6, num_groups=3, diversity_penalty=-0.5),
                dict(beam_size=6, num_groups=3, diversity_penalty=float('nan')), dict(beam_size=6, diversity_penalty=0.5),
                dict(beam_size=6, num_groups=1, diversity_penalty=INF), dict(beam_size=9, num_groups=3)):
        for search in (net.beam_search, ens.beam_search):
            with pytest.raises(ValueError):
                search(frames, regions, **bad)
    for fine in (dict(beam_size=6, num_groups=6, diversity_penalty=INF, n_best=1), dict(beam_size=4, num_groups=2, n_best=3)):
        ids = net.beam_search(frames, regions, **fine)[0]
        assert ids.shape[:2] == (2, fine['n_best'])

"""CPU: decoding under a forced prefix -- `pack_prefix`, `check_prefix` and every refusal; the emulated force launches
(tests/emul_prefix.py) on hand-made steps; `beam_search(prefix=...)`, with exclusions and with constraints, of a small host model
through the emulated ops against an independent search on Python lists that teacher-forces the prefix on ONE beam and then searches
on as the plain search does; the samplers; the launch sequences; the graph classes and `gather_results`."""
import functools
import inspect

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import graphs
from dlsg_amd import scoring as S
from dlsg_amd.beam import PrefixNotCovered, check_prefix, exclusions_hit, pack_exclusions, pack_prefix
from dlsg_amd.synth import synth_batch, synth_state_dict
from emul_beam import BeamEmul, banned_classes
from emul_excl import excluded_word
from emul_prefix import PrefixEmul, prefix_lens
from helpers import small_args
from launch_trace import TraceEmul, fresh, traced
from oracle import torch_ref as R
from test_beam_nbest_host import close, oracle_stepper, reference_rank, words_of
from test_constrained_host import restated_clip_step

INF = float('inf')
GAP = 1e-4
V, L, END = 9, 6, 2


# ---------------------------------------------------------------------------------------------- pack_prefix, check_prefix
def test_pack_prefix_pads_and_reads_every_kind_of_item():
    vocab = dlsg_amd.make_vocab(V)
    got = pack_prefix(['w0 w1  w2', ('w3', 5), [8], None, '', ()], vocab)
    assert got.dtype == torch.int64 and got.tolist() == [[4, 5, 6], [7, 5, -1], [8, -1, -1], [-1] * 3, [-1] * 3, [-1] * 3]
    assert pack_prefix([None, ''], vocab).shape == (2, 0) and pack_prefix([], vocab).shape == (0, 0)
    assert pack_prefix(['<unk> w0'], vocab).tolist() == [[3, 4]]
    assert pack_prefix(['zebra w0', (77,)], vocab, allow_unk=True).tolist() == [[3, 4], [3, -1]]
    assert pack_prefix(['w0 w1 w2 w3 w4'], vocab, max_words=6).shape == (1, 5)
    assert prefix_lens(got, V) == [3, 2, 1, 0, 0, 0]


@pytest.mark.parametrize('item,match', [('w0 <end>', 'cannot stand in a prefix'), (('<start>',), 'cannot stand in a prefix'),
                                        ([0], 'cannot stand in a prefix'), ('zebra', 'not in the vocabulary'),
                                        ((9,), 'not in the vocabulary'), ((-1,), 'not in the vocabulary'), (4, 'a prefix is a string')])
def test_pack_prefix_value_errors(item, match):
    with pytest.raises(ValueError, match=match):
        pack_prefix([None, item], dlsg_amd.make_vocab(V))


def test_pack_prefix_refuses_a_prefix_that_leaves_no_room_for_end():
    vocab = dlsg_amd.make_vocab(V)
    with pytest.raises(ValueError, match='clip 1: a prefix of 6 words and <end> do not fit into max_words 6'):
        pack_prefix(['w0', 'w0 w1 w2 w3 w4 w0'], vocab, max_words=6)
    assert pack_prefix(['w0 w1 w2 w3 w4 w0'], vocab).shape == (1, 6)


def test_check_prefix():
    vocab = dlsg_amd.make_vocab(V)
    dev = torch.device('cpu')
    px = pack_prefix(['w0 w1', None, 'w2'], vocab)
    assert check_prefix(px, 3, dev, L) is px
    assert check_prefix(px.t().contiguous().t(), 3, dev, L).is_contiguous()
    assert check_prefix(px[:, :0], 3, dev, L) is None
    assert torch.equal(check_prefix(['w0 w1', None, 'w2'], 3, dev, L, vocab), px)
    for bad, match in ((px.tolist(), 'an int64 tensor'), (px.int(), 'an int64 tensor'), (px[0], 'an int64 tensor'),
                       (px.float(), 'an int64 tensor'), (px[:2], 'holds 2 clips, the batch 3'),
                       (torch.full((3, L), 4, dtype=torch.int64), 'prefix of 6 words and <end> do not fit into max_words 6')):
        with pytest.raises(ValueError, match=match):
            check_prefix(bad, 3, dev, L)
    with pytest.raises(ValueError, match='prefix on meta, the clips on cpu'):
        check_prefix(px.to('meta'), 3, dev, L)
    with pytest.raises(ValueError, match='do not fit into max_words 6'):
        check_prefix(['w0 w1 w2 w3 w4 w0', None, None], 3, dev, L, vocab)


# ---------------------------------------------------------------------------------------------- the emulated launches
def test_the_emulated_beam_launch_on_a_hand_made_step():
    gen = torch.Generator().manual_seed(3)
    B, k, t = 3, 3, 1
    lgs = [torch.randn(B * k, V, generator=gen) for _ in range(2)]
    last_lp = -torch.rand(B * k, generator=gen)
    hist_in = torch.randint(4, V, (B * k, L), generator=gen)
    prefix = torch.tensor([[5, 7], [6, -1], [-1, 4]])
    keep = dict(pred=torch.full((B * k,), 99), nlp=torch.full((B * k,), 9.0), back=torch.full((B * k,), 99),
                rows=torch.full((B * k,), 99), hout=torch.full((B * k, L), 99))
    out = {key: v.clone() for key, v in keep.items()}
    ops = PrefixEmul()
    ops.beam_force_prefix(lgs, [0.25, 0.75], 0, None, last_lp, out['pred'], out['nlp'], out['back'], out['rows'], k, END, hist_in,
                          out['hout'], t, prefix)
    for key in keep:                                                   # clips 1 (p = 1) and 2 (p = 0): untouched
        assert torch.equal(out[key][k:], keep[key][k:]), key
    assert out['pred'][:k].tolist() == [7] * k and out['back'][:k].tolist() == [0] * k and out['rows'][:k].tolist() == [0] * k
    assert out['hout'][:k].tolist() == [[int(hist_in[0, 0]), 7, END, END, END, END]] * k
    p = 0.25 * torch.softmax(lgs[0][0].double(), 0)[7] + 0.75 * torch.softmax(lgs[1][0].double(), 0)[7]
    assert abs(float(out['nlp'][0]) - (float(p.log()) + float(last_lp[0]))) <= 1e-6 and out['nlp'][1:k].tolist() == [-INF] * (k - 1)
    # step 0 reads no history and no log-prob; mode 1 is the weighted mean log-probability
    ops.beam_force_prefix(lgs, [0.25, 0.75], 1, None, None, out['pred'], out['nlp'], out['back'], out['rows'], k, END, None, out['hout'],
                          0, prefix)
    want = 0.25 * torch.log_softmax(lgs[0][k].double(), 0)[6] + 0.75 * torch.log_softmax(lgs[1][k].double(), 0)[6]
    assert abs(float(out['nlp'][k]) - float(want)) <= 1e-6 and out['hout'][k].tolist() == [6] + [END] * (L - 1)
    assert torch.equal(out['pred'][2 * k:], keep['pred'][2 * k:]) and ops.force_calls == [('beam', 1), ('beam', 0)]


def test_the_emulated_sampler_launch_on_a_hand_made_step():
    gen = torch.Generator().manual_seed(4)
    rows, n, W, t = 6, 2, 5, 1
    logits, E = torch.randn(rows, V, generator=gen), torch.randn(V, W, generator=gen)
    prefix = torch.tensor([[5, 7], [6, -1], [4, 8]])
    ids, out, logp = torch.full((rows,), 3), torch.full((rows, W), 9.0), torch.full((rows,), 9.0)
    lens, kept = torch.tensor([L, 2, L, L, L, 1]), torch.full((rows,), 7, dtype=torch.int32)
    PrefixEmul().sample_force_prefix(logits, E, ids, out, logp, lens, t, prefix, L, temperature=0.7, rows_per_clip=n, kept=kept)
    assert ids.tolist() == [7, 7, 3, 3, 8, 8] and lens.tolist() == [L, L, L, L, L, L] and kept.tolist() == [1, 1, 7, 7, 1, 1]
    lp = torch.log_softmax(logits.double() / 0.7, 1)
    for r, w in ((0, 7), (1, 7), (4, 8), (5, 8)):
        assert abs(float(logp[r]) - float(lp[r, w])) <= 1e-6 and torch.equal(out[r], E[w])
    assert logp[2:4].tolist() == [9.0, 9.0] and bool((out[2:4] == 9.0).all())
    PrefixEmul().sample_force_prefix(logits, E, ids, out, logp, lens, 0, prefix, L, temperature=0.0, rows_per_clip=n)
    assert ids.tolist() == [5, 5, 6, 6, 4, 4] and abs(float(logp[2]) - float(torch.log_softmax(logits.double(), 1)[2, 6])) <= 1e-6


# ---------------------------------------------------------------------------------------------- the whole search, on lists
SEED, BIAS = 21, 0.5
PREFIXES = [(), (5,), (7, 4), (4, 8, 5, 6, 7)]                         # lengths 0, 1, 2 and L - 1 in one batch


def tiny_pair(ops=None, seed=SEED, batch=len(PREFIXES)):
    """a CapGnnModel of 9 words and max_words 6 with seeded weights and the oracle with the same weights, on `batch` clips"""
    args = small_args(dropout=0.0, max_words=L)
    vocab = dlsg_amd.make_vocab(V)
    torch.manual_seed(0)
    net = dlsg_amd.CapGnnModel(args, vocab).eval()
    sd = synth_state_dict(net.state_dict(), seed)
    sd['decoder.word_restore.bias'][vocab('<end>')] += BIAS
    net.load_state_dict(sd)
    if ops is not None:
        net.set_ops(ops)
    orc = R.CapGnnModelRef(args, vocab).eval()
    orc.load_state_dict(sd)
    frames, regions, _, _ = synth_batch(args, V, batch, seed + 1)
    assert net.decoder.max_words == L and net.decoder.vocab_size == V and vocab('<end>') == END
    return net, orc, frames, regions


def clip_search(orc, frames, regions, k, prefix, g=0, min_len=0, entries=(), sets=None):
    """One clip's search on Python lists, by itself: the prefix is teacher-forced on ONE beam -- its words' log-probs are summed,
    no ban is looked at -- and from the first free step on the search is the plain one, which expands that one beam as step 0
    expands the start: per live beam the k best classes that are not banned (n-gram, min_len, `excluded_word` of every entry), an
    ended beam offers <end> at 0, the k best candidates become the beams; with `sets` (a list of sets of word ids) the step is
    the constrained one (`restated_clip_step`).  -> (tokens [k][L], log-probs [k], gap)"""
    step_fn, start, state, end, _ = oracle_stepper(orc, frames, regions)
    beams, gap, last = [((), np.float32(0.0))], INF, start
    for t in range(L):
        logp, state = step_fn(last, state)
        logp = logp.numpy()
        if t < len(prefix):
            assert len(beams) == 1
            picks = [(np.float32(logp[0][prefix[t]] + beams[0][1]), 0, prefix[t])]
        elif sets is not None:
            rows = [logp[j].astype(np.float64).tolist() for j in range(len(beams))]
            picks, _, gp = restated_clip_step([(toks, lp, bool(toks) and toks[-1] == end) for toks, lp in beams], rows, rows, t, k, end,
                                              g, min_len, sets, neighbours=False)
            gap = min(gap, gp)
            picks = [(np.float32(v), j, cls) for v, j, cls, _ in picks]
            assert len(picks) == k
        else:
            cands = []                                                  # (value, parent, class), in candidate-index order
            for j, (toks, lp) in enumerate(beams):
                if toks and toks[-1] == end:
                    cands.append((lp, j, end))
                    continue
                banned = banned_classes(list(toks), t, g, min_len, end) | {excluded_word(list(toks), list(e), V) for e in entries}
                order = sorted((c for c in range(V) if c not in banned), key=lambda c: (-logp[j][c], c))[:k]
                cands += [(np.float32(logp[j][c] + lp), j, c) for c in order]
            ranked = sorted(range(len(cands)), key=lambda i: (-cands[i][0], i))
            assert len(ranked) >= k
            if len(ranked) > k and cands[ranked[k]][0] > -INF:
                gap = min(gap, float(cands[ranked[k - 1]][0]) - float(cands[ranked[k]][0]))
            picks = [cands[i] for i in ranked[:k]]
        state = {key: v[torch.tensor([j for _, j, _ in picks])] for key, v in state.items()}
        beams = [(beams[j][0] + (cls,), v) for v, j, cls in picks]
        last = torch.tensor([toks[-1] for toks, _ in beams])
    assert len(beams) == k                                               # (P <= L - 1: the last step is free)
    return [list(toks) for toks, _ in beams], [lp for _, lp in beams], gap


@functools.lru_cache(maxsize=None)
def restated(k, g, min_len, alpha, kind='plain'):
    """(ids, scores, lens, gap per clip, the exclusions or the constraints) of the prefixed search by lists alone, clip by clip"""
    net, orc, frames, regions = tiny_pair()
    extra, entries, sets = None, [()] * len(PREFIXES), [None] * len(PREFIXES)
    if kind == 'excl':
        # entries completed across the boundary: (last prefix word, the word the free search puts behind it)
        free = restated(k, g, min_len, alpha)[0]
        pairs = [[(p[-1], free[b][0][len(p)])] if p and free[b][0][len(p)] >= 4 else [] for b, p in enumerate(PREFIXES)]
        extra = pack_exclusions(net.decoder.vocab, per_clip=pairs)
        entries = [[tuple(e) for e in extra.per_clip[b].tolist()] for b in range(len(PREFIXES))]
    if kind == 'cons':
        # clip 1: a constraint its prefix word meets; clip 2: one the search has to meet itself; clip 3: met by the third prefix word
        extra = [[], [[5, 6]], [[8]], [[5], [6, 4]]]
        sets = [[set(c) for c in clip] for clip in extra]
    toks, lps, gaps = [], [], []
    for b, p in enumerate(PREFIXES):
        t, lp, gp = clip_search(orc, frames[b:b + 1], regions[b:b + 1], k, p, g, min_len, entries[b], sets[b])
        toks.append(t); lps.append(lp); gaps.append(gp)
    ids, sc, ln, rank_gap = reference_rank(toks, lps, END, alpha, k)
    if kind == 'cons':                                                   # the stable sort by constraints met
        for b in range(len(PREFIXES)):
            met = [sum(bool(s & set(words_of(row, END))) for s in sets[b]) for row in ids[b]]
            order = sorted(range(k), key=lambda i: (-met[i], i))
            ids[b], sc[b], ln[b] = [ids[b][i] for i in order], [sc[b][i] for i in order], [ln[b][i] for i in order]
    return ids, sc, ln, [min(a, b) for a, b in zip(gaps, rank_gap)], extra


def emulated(k, g, min_len, alpha, kind='plain'):
    net, _, frames, regions = tiny_pair(PrefixEmul())
    px = pack_prefix([tuple(p) for p in PREFIXES], net.decoder.vocab)
    opts = dict(beam_size=k, length_penalty=alpha, no_repeat_ngram=g, min_len=min_len, prefix=px)
    extra = restated(k, g, min_len, alpha, kind)[4]
    if kind == 'cons':
        return net.constrained_beam_search(frames, regions, extra, return_met=True, **opts)
    return net.beam_search(frames, regions, exclude=extra, **opts)


def check_against_lists(got, want):
    ids, scores, lens = got[:3]
    want_ids, want_sc, want_len, gap = want[:4]
    keep = [b for b in range(len(PREFIXES)) if gap[b] >= GAP]
    assert len(keep) >= len(PREFIXES) - 1, gap
    for b in keep:
        assert ids[b].tolist() == want_ids[b] and lens[b].tolist() == want_len[b], (b, ids[b].tolist(), want_ids[b])
        close(scores[b].numpy(), want_sc[b])
    for b, p in enumerate(PREFIXES):                                     # every row begins with its clip's prefix
        assert all(row[:len(p)] == list(p) for row in ids[b].tolist()), b


SEARCHES = [(1, 0, 0, 0.0), (3, 0, 0, 0.7), (3, 2, 3, 0.7), (1, 2, 4, 0.0)]


@pytest.mark.parametrize('k,g,min_len,alpha', SEARCHES)
def test_prefixed_beam_search_matches_the_search_on_lists(k, g, min_len, alpha):
    got = emulated(k, g, min_len, alpha)
    check_against_lists(got, restated(k, g, min_len, alpha))
    # the clip without a prefix gets what it gets without the keyword
    net, _, frames, regions = tiny_pair(PrefixEmul())
    plain = net.beam_search(frames, regions, beam_size=k, length_penalty=alpha, no_repeat_ngram=g, min_len=min_len)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(got, plain))
    assert not torch.equal(got[0][1:], plain[0][1:])
    # min_len counts the prefix: no <end> before min_len tokens, and a forced word overrides the bans (a prefix may repeat a bigram)
    assert bool((got[2][got[1] > -INF] > min_len).all())


def test_forced_words_override_the_ngram_ban_and_the_ban_sees_them():
    net, _, frames, regions = tiny_pair(PrefixEmul())
    px = torch.tensor([[4, 5, 4, 5], [4, 5, 4, -1], [-1] * 4, [6, 6, 6, -1]])
    ids, scores, lens = net.beam_search(frames, regions, beam_size=3, no_repeat_ngram=2, prefix=px)
    assert ids[0, :, :4].tolist() == [[4, 5, 4, 5]] * 3 and ids[3, :, :3].tolist() == [[6, 6, 6]] * 3
    assert bool((ids[1, :, 3] != 5).all()) and bool((ids[3, :, 3] != 6).all())        # (4, 5) and (6, 6) stand in the prefix
    assert bool((ids[0, :, 4] != 4).all())                                             # (5, 4) stands there too
    assert bool(torch.isfinite(scores[:, 0]).all())


@pytest.mark.parametrize('k', [1, 3])
def test_an_exclusion_is_completed_across_the_boundary_and_banned_there(k):
    want = restated(k, 0, 0, 0.7, 'excl')
    got = emulated(k, 0, 0, 0.7, 'excl')
    check_against_lists(got, want)
    free = restated(k, 0, 0, 0.7)[0]
    ex = want[4]
    assert int((ex.per_clip[:, 0, 0] >= 0).sum()) >= 2                                  # the entries exist ...
    assert any(free[b][0] != want[0][b][0] for b in range(len(PREFIXES)))             # ... and bite
    hit = exclusions_hit(got[0], got[2], ex)
    assert not bool(hit[got[1] > -INF].any())
    # the caller's own words are not checked: a prefix that holds an entry is decoded, and counted by exclusions_hit
    net, _, frames, regions = tiny_pair(PrefixEmul())
    own = pack_exclusions(net.decoder.vocab, phrases=[(7, 4)])
    ids, scores, lens = net.beam_search(frames, regions, beam_size=k, exclude=own, prefix=pack_prefix(PREFIXES, net.decoder.vocab))
    assert ids[2, 0, :2].tolist() == [7, 4] and int(exclusions_hit(ids, lens, own)[2, 0]) == 1 and bool(torch.isfinite(scores[2, 0]))


@pytest.mark.parametrize('k', [1, 3])
def test_a_prefix_word_meets_a_constraint(k):
    want = restated(k, 0, 0, 0.7, 'cons')
    got = emulated(k, 0, 0, 0.7, 'cons')
    check_against_lists(got, want)
    met = got[3]
    assert met[1, 0] == 1 and met[3, 0] == 2 and met[2, 0] == 1                         # the prefix's words count
    # phrases: the prefix advances a phrase and the search completes it
    net, _, frames, regions = tiny_pair(PrefixEmul())
    px = pack_prefix(PREFIXES, net.decoder.vocab)
    ids, _, _, pmet = net.constrained_beam_search(frames, regions, [[], ['w1 w4'], ['w3 w0 w2'], []], beam_size=k, prefix=px,
                                                  return_met=True)
    assert ids[1, 0, :2].tolist() == [5, 8] and ids[2, 0, :3].tolist() == [7, 4, 6] and pmet[:, 0].tolist() == [0, 1, 1, 0]


def test_an_ensemble_of_the_model_twice_is_the_model():
    net, _, frames, regions = tiny_pair(PrefixEmul())
    px = pack_prefix(PREFIXES, net.decoder.vocab)
    opts = dict(beam_size=3, length_penalty=0.7, no_repeat_ngram=2, prefix=px)
    want = net.beam_search(frames, regions, **opts)
    for mode in ('prob', 'logprob'):
        got = dlsg_amd.Ensemble([net, net], weights=[0.6, 0.4], mode=mode).beam_search(frames, regions, **opts)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
        close(got[1].numpy(), want[1].numpy())


def test_forcing_what_the_search_chose_changes_nothing_and_score_returns_the_scores():
    net, _, frames, regions = tiny_pair(PrefixEmul())
    opts = dict(beam_size=1, length_penalty=0.7, min_len=5)
    ids, scores, lens = net.beam_search(frames, regions, **opts)
    for p in (1, 3, L - 1):
        px = ids[:, 0, :p].contiguous()
        got = net.beam_search(frames, regions, prefix=px, **opts)
        assert torch.equal(got[0], ids) and torch.equal(got[2], lens)
        close(got[1].numpy(), scores.numpy())
    px = pack_prefix(PREFIXES, net.decoder.vocab)
    ids, scores, lens = net.beam_search(frames, regions, beam_size=3, length_penalty=0.7, prefix=px)
    sc, ln = net.score(frames, regions, ids, length_penalty=0.7)
    assert torch.equal(ln, lens)
    close(sc.numpy(), scores.numpy(), tol=1e-4)


# ---------------------------------------------------------------------------------------------- the samplers
def test_the_samplers_continue_the_prefix():
    net, _, frames, regions = tiny_pair(PrefixEmul())
    px = pack_prefix(PREFIXES, net.decoder.vocab)
    n = 2
    for kw in (dict(), dict(top_k=3, no_repeat_ngram=2, return_kept=True),
               dict(exclude=pack_exclusions(net.decoder.vocab, words=['w4']), return_kept=True), dict(share_encoder=True)):
        out = net.sample(frames, regions, n=n, temperature=0.8, seed=5, prefix=px, **kw)
        ids, logp, lens = out[:3]
        for b, p in enumerate(PREFIXES):
            rows = ids[b * n:(b + 1) * n].tolist()
            assert all(row[:len(p)] == list(p) for row in rows), (kw, b)
            assert bool((lens[b * n:(b + 1) * n] > len(p)).all())
            if kw.get('return_kept'):
                assert bool((out[3][b * n:(b + 1) * n, :len(p)] == 1).all())
        plain = net.sample(frames, regions, n=n, temperature=0.8, seed=5, **kw)
        assert all(torch.equal(a[:n], b[:n]) for a, b in zip(out, plain))              # the clip without a prefix
    # forcing what the plain sampler drew: the same ids, lens and log-probs
    ids, logp, lens = net.sample(frames, regions, n=n, temperature=0.8, seed=5)
    first = ids.view(len(PREFIXES), n, L)[:, 0]                                         # (the clip's first row: both rows are forced to it)
    own = torch.where(torch.arange(L - 1).view(1, -1) < (lens.view(-1, n)[:, :1] - 1).clamp(max=3), first[:, :L - 1], torch.tensor(-1))
    got = net.sample(frames, regions, n=n, temperature=0.8, seed=5, prefix=own)
    rows = torch.arange(0, len(PREFIXES) * n, n)
    assert torch.equal(got[0][rows], ids[rows]) and torch.equal(got[2][rows], lens[rows])
    assert float((got[1][rows] - logp[rows]).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------- refusals
def test_what_is_not_covered_raises_before_the_encoder_runs():
    class NoEncoder(PrefixEmul):
        def gemm(self, *a, **kw):
            raise AssertionError('the encoder ran')
    net, _, frames, regions = tiny_pair(NoEncoder())
    px = pack_prefix(PREFIXES, net.decoder.vocab)
    with pytest.raises(ValueError, match='prefix and num_groups = 2'):
        net.beam_search(frames, regions, beam_size=4, num_groups=2, prefix=px)
    with pytest.raises(ValueError, match='prefix and num_groups = 2'):
        dlsg_amd.Ensemble([net]).beam_search(frames, regions, beam_size=4, num_groups=2, prefix=px)
    with pytest.raises(ValueError, match='prefix and sample_without_replacement'):
        net.sample_without_replacement(frames, regions, n=2, prefix=px)
    with pytest.raises(ValueError, match='prefix and sample_without_replacement'):
        dlsg_amd.sample_without_replacement(net, frames, regions, n=2, prefix=px)
    with pytest.raises(ValueError, match='prefix and StochasticBeamGraph'):
        dlsg_amd.StochasticBeamGraph(net, frames, regions, n=2, prefix=px)
    from dlsg_amd.consensus import consensus_search
    with pytest.raises(ValueError, match=r'prefix and consensus_search\(stochastic'):
        consensus_search(net, frames, regions, None, stochastic=dict(n=2, prefix=px))
    with pytest.raises(ValueError, match=r'prefix and consensus_search\(stochastic'):
        consensus_search(net, frames, regions, None, stochastic=dict(n=2), prefix=px)
    with pytest.raises(ValueError, match='prefix is not covered in SCSTTrainer'):
        dlsg_amd.SCSTTrainer(net, None, sample_options=dict(prefix=px))
    for call in (lambda: net.beam_search(frames, regions, prefix=px[:3]), lambda: net.sample(frames, regions, n=2, prefix=px[:3]),
                 lambda: net.constrained_beam_search(frames, regions, [[]] * 4, prefix=px[:3])):
        with pytest.raises(ValueError, match='holds 3 clips, the batch 4'):
            call()
    with pytest.raises(ValueError, match='do not fit into max_words 6'):
        net.beam_search(frames, regions, prefix=torch.full((4, L), 4))
    with pytest.raises(ValueError, match='cannot stand in a prefix'):
        net.beam_search(frames, regions, prefix=['w0 <end>', None, None, None])
    # an ops object without the two launches
    old, _, frames, regions = tiny_pair(type('Old', (BeamEmul,), {'gemm': NoEncoder.gemm})())
    with pytest.raises(PrefixNotCovered, match='Old has no beam_force_prefix'):
        old.beam_search(frames, regions, prefix=px)
    with pytest.raises(PrefixNotCovered, match='Old has no sample_force_prefix'):
        old.sample(frames, regions, prefix=px)
    with pytest.raises(ValueError, match='Old has no beam_force_prefix'):
        old.constrained_beam_search(frames, regions, [[]] * 4, prefix=px)
    loader = [(frames, regions, None, ['a', 'b', 'c', 'd'])]
    with pytest.raises(ValueError, match='decode: prefix is an int64 tensor'):
        S.gather_results(net, loader, decode=dict(beam_size=3, prefix=['w0'] * 4))


def test_every_entry_point_takes_the_keyword():
    for cls in (dlsg_amd.CapGnnModel, dlsg_amd.CapBaseline1, dlsg_amd.CapBaselineModel):
        for name in ('beam_search', 'constrained_beam_search', 'sample', 'sample_without_replacement'):
            assert inspect.signature(getattr(cls, name)).parameters['prefix'].default is None
    assert inspect.signature(dlsg_amd.Ensemble.beam_search).parameters['prefix'].default is None
    for fn in (dlsg_amd.beam_nbest, dlsg_amd.beam.ensemble_nbest, dlsg_amd.constrained_nbest, dlsg_amd.beam.stochastic_nbest):
        assert inspect.signature(fn).parameters['prefix'].default is None
    assert inspect.signature(dlsg_amd.SampleGraph.__init__).parameters['prefix'].default is None
    from dlsg_amd import abi
    assert len(abi.functions['dlsg_beam_force_prefix'][1]) == 14 and len(abi.functions['dlsg_sample_force_prefix'][1]) == 24
    assert abi.defines['DLSG_ABI_VERSION'] == 8 and len(abi.functions) == 130
    for name in ('pack_prefix', 'check_prefix', 'PrefixNotCovered'):
        assert hasattr(dlsg_amd, name)
    from dlsg_amd.hip import HipOps
    assert list(inspect.signature(HipOps.beam_force_prefix).parameters)[1:4] == ['logits_list', 'weights', 'mode']
    assert list(inspect.signature(HipOps.beam_force_prefix).parameters)[-1] == 'prefix' and hasattr(HipOps, 'sample_force_prefix')


# ---------------------------------------------------------------------------------------------- the launch sequences
class PrefixTrace(PrefixEmul):
    """PrefixEmul that records its calls as tests/launch_trace.py's TraceEmul does (its bases are among PrefixEmul's)"""
    trace = None
    __getattribute__ = TraceEmul.__getattribute__


def names(trace):
    return [call[0] for call in trace]


def without(seq, name):
    return [x for x in seq if x != name]


def record(call):
    """the trace of call(net, vocab, frames, regions) on a fresh, seeded model (so that two records draw the same seeds), and its ops"""
    net, args, vocab, frames, regions, caps, lens = fresh('capgnn')
    net.set_ops(PrefixTrace())
    return traced(net, lambda: call(net, vocab, frames, regions)), net.ops


@pytest.mark.parametrize('search', ['hist', 'excl', 'cons', 'ens'])
def test_the_prefixed_search_launches_the_plain_one_with_a_force_launch_behind_the_first_selects(search):
    select = dict(hist='beam_select_hist', excl='beam_select_excl', cons='beam_select_cons', ens='beam_select_ens')[search]

    def run(**kw):
        return dict(hist=lambda net, vocab, frames, regions: net.beam_search(frames, regions, beam_size=3, min_len=2, **kw),
                    excl=lambda net, vocab, frames, regions: net.beam_search(frames, regions, beam_size=3,
                                                                             exclude=pack_exclusions(vocab, words=[10]), **kw),
                    cons=lambda net, vocab, frames, regions: net.constrained_beam_search(frames, regions, [[5], [], [6]], beam_size=3, **kw),
                    ens=lambda net, vocab, frames, regions: dlsg_amd.Ensemble([net, net]).beam_search(frames, regions, beam_size=3, **kw))[search]
    plain, _ = record(run())
    for px in (None, torch.full((3, 0), -1, dtype=torch.int64), [None, '', ()]):       # P == 0: what was launched before
        assert record(run(prefix=px))[0] == plain
    forced, ops = record(run(prefix=torch.tensor([[4, 5, 6], [-1, -1, -1], [7, -1, -1]])))
    assert without(names(forced), 'beam_force_prefix') == names(plain)
    assert [c for c in forced if c[0] != 'beam_force_prefix'] == plain                  # the other launches: the same arguments
    seq = names(forced)
    at = [i for i, x in enumerate(seq) if x == 'beam_force_prefix']
    selects = [i for i, x in enumerate(seq) if x == select]
    assert len(selects) == 26 and at == [i + 1 for i in selects[:3]]                    # behind each of the first P selects
    assert ops.force_calls == [('beam', 0), ('beam', 1), ('beam', 2)]


@pytest.mark.parametrize('step,kw', [('sample_embed', {}), ('sample_filter_embed', dict(top_k=5)), ('sample_excl_embed', dict(exclude=[10]))])
def test_the_prefixed_sampler_launches_the_plain_one_with_a_force_launch_behind_the_first_steps(step, kw):
    def run(**more):
        def call(net, vocab, frames, regions):
            opts = dict(exclude=pack_exclusions(vocab, words=kw['exclude'])) if 'exclude' in kw else kw
            return net.sample(frames, regions, n=2, seed=9, **opts, **more)
        return call
    plain, _ = record(run())
    assert record(run(prefix=None))[0] == plain
    assert record(run(prefix=torch.full((3, 0), -1, dtype=torch.int64)))[0] == plain
    forced, ops = record(run(prefix=torch.tensor([[4, 5], [-1, -1], [7, -1]])))
    assert [c for c in forced if c[0] != 'sample_force_prefix'] == plain               # the other launches: the same arguments
    forced = names(forced)
    steps = [i for i, x in enumerate(forced) if x == step]
    behind = [forced.index('sample_force_prefix', i) for i in steps[:2]]                # (the emulated step embeds inside its call)
    assert forced.count('sample_force_prefix') == 2 and behind == sorted(set(behind)) and all(b < steps[j + 1] for j, b in enumerate(behind))
    assert ops.force_calls == [('sample', 0), ('sample', 1)]


# ---------------------------------------------------------------------------------------------- graphs, gather_results
class ReplayStub(object):
    def replay(self):
        pass


def test_the_graph_classes_keep_their_own_prefix(monkeypatch):
    """without a capture (the body runs once, eagerly): `graph.prefix` is a copy of the table and the decode runs on that tensor"""
    monkeypatch.setattr(graphs, 'capture', lambda dev, body, warmup=None: (ReplayStub(), body()))
    net, _, frames, regions = tiny_pair(PrefixEmul())
    px = pack_prefix(PREFIXES, net.decoder.vocab)
    ens = dlsg_amd.Ensemble([net])
    cons = [[], [[5, 6]], [[8]], []]
    cases = [(lambda **kw: dlsg_amd.NBestBeamGraph(net, frames, regions, beam_size=3, **kw),
              lambda **kw: net.beam_search(frames, regions, beam_size=3, **kw)),
             (lambda **kw: dlsg_amd.EnsembleBeamGraph(ens, frames, regions, beam_size=3, **kw),
              lambda **kw: ens.beam_search(frames, regions, beam_size=3, **kw)),
             (lambda **kw: dlsg_amd.ConstrainedBeamGraph(net, frames, regions, cons, beam_size=3, **kw),
              lambda **kw: net.constrained_beam_search(frames, regions, cons, beam_size=3, **kw)),
             (lambda **kw: dlsg_amd.SampleGraph(net, frames, regions, n=2, temperature=0.8, **kw),
              lambda **kw: net.sample(frames, regions, 2, 0.8, 0, **kw))]
    for make, eager in cases:
        graph = make(prefix=px)
        assert torch.equal(graph.prefix, px) and graph.prefix.data_ptr() != px.data_ptr()
        assert all(torch.equal(a, b) for a, b in zip(graph.out, eager(prefix=px)))
        assert torch.equal(make(prefix=[tuple(p) for p in PREFIXES]).prefix, px)        # per-clip lists are packed
        plain = make()
        assert plain.prefix is None and all(torch.equal(a, b) for a, b in zip(plain.out, eager()))


def test_gather_results_prefix_option():
    net, _, frames, regions = tiny_pair(PrefixEmul())
    vocab = net.decoder.vocab
    vids = ['a', 'b', 'c', 'd']
    loader = [(frames, regions, None, vids)]
    begin = dict(zip(vids, ('', 'w1', 'w3 w0', 'w0 w4 w1')))
    fn = lambda ids: pack_prefix([begin[v] for v in ids], vocab)       # noqa: E731
    plain = S.gather_results(net, loader, decode=dict(beam_size=3))
    got = S.gather_results(net, loader, decode=dict(beam_size=3, prefix=fn))
    assert got['a'] == plain['a'] and all(got[v].startswith(begin[v]) for v in vids) and got != plain
    assert S.gather_results(net, loader, decode=dict(beam_size=3, prefix=fn(vids))) == got
    assert S.gather_results(net, loader, decode=dict(beam_size=3, prefix=lambda ids: [begin[v] for v in ids])) == got
    assert S.gather_results(net, loader, decode=dict(beam_size=3, prefix=None)) == plain
    # consensus and rescore searches hand the keyword to their beam search
    ids = dlsg_amd.rescore_search(net, net, frames, regions, n_best=3, beam_size=3, prefix=fn(vids))[0]
    assert ids[3, :, :3].tolist() == [[4, 8, 5]] * 3

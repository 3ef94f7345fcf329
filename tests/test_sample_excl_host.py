"""CPU: exclusions in sampling -- `sample(exclude=...)`, `sample_without_replacement(exclude=...)`, their graph classes and
`SCSTTrainer(sample_options=dict(exclude=...))` through the emulated ops (tests/emul_sample_excl.py: the steps without tables on
logits with the banned words at -inf): what an exclusion owes its caller, the row-to-clip mapping, which op a word step launches,
and every refusal.  The GPU side is tests/test_gpu_sample_excl.py."""
import collections
import functools
import inspect

import numpy as np
import pytest
import torch

import dlsg_amd
from dlsg_amd import engine as E
from dlsg_amd import graphs
from dlsg_amd import scoring as S
from dlsg_amd.beam import BAD_ENDINGS, ExcludeNotCovered, Exclusions, exclusions_hit, pack_exclusions
from dlsg_amd.consensus import consensus_search
from emul_excl import ExclEmul, excluded_word
from emul_sample_excl import SampleExclEmul, banned_by_tables, masked
from test_beam_nbest_host import synth_pair
from test_cider_device_host import corpus_for
from test_scst_host import LengthReward, _spy

SEED, CLIPS, N = 11, 4, 3
INF = float('inf')


@functools.lru_cache(maxsize=None)
def host_net():
    return synth_pair(SEED, CLIPS, end_bias=1.0, ops=SampleExclEmul())


def caption_words(ids, lens):
    """per row the words of the caption: up to and including the first <end>"""
    return [row[:n] for row, n in zip(ids.tolist(), lens.tolist())]


def exclusions_from_draw(ids, lens, vocab, n):
    """Exclusions that bite a draw ids (B*n, L): per clip the first word of its first row; shared, a bigram of a caption of the
    last clip that stands behind the caption's first word; and the ending (last word, <end>) of the first caption that ends before L"""
    B = ids.shape[0] // n
    L = ids.shape[1]
    caps = caption_words(ids, lens)
    per_clip = [[(caps[b * n][0],)] for b in range(B)]
    row = next(r for r in range((B - 1) * n, B * n) if len(caps[r]) >= 4)
    bigram = tuple(caps[row][1:3])
    ending = next(c for c in caps if 2 <= len(c) < L and c[-2] >= 4)[-2]
    return pack_exclusions(vocab, phrases=[bigram], bad_endings=[vocab.idx2word[ending]], per_clip=per_clip), bigram, ending


@functools.lru_cache(maxsize=None)
def drawn(share):
    net, _, frames, regions = host_net()
    plain = net.sample(frames, regions, n=N, seed=5, share_encoder=share)
    ex, bigram, ending = exclusions_from_draw(plain[0], plain[2], net.decoder.vocab, N)
    got = net.sample(frames, regions, n=N, seed=5, share_encoder=share, exclude=ex, return_kept=True)
    return plain, ex, got, bigram, ending


# ---------------------------------------------------------------------------------------------- sample()
@pytest.mark.parametrize('share', [False, True])
def test_no_sampled_row_holds_what_is_excluded(share):
    net, _, frames, regions = host_net()
    plain, ex, (ids, logp, lens, kept), _, _ = drawn(share)
    L, V = net.decoder.max_words, net.decoder.vocab_size
    assert ids.shape == (CLIPS * N, L) and logp.shape == ids.shape and lens.shape == (CLIPS * N,) and kept.shape == ids.shape
    assert bool((exclusions_hit(plain[0].view(CLIPS, N, L), plain[2].view(CLIPS, N), ex) > 0).any(1).all())      # (it bites every clip)
    assert int(exclusions_hit(ids.view(CLIPS, N, L), lens.view(CLIPS, N), ex).sum()) == 0
    assert bool(torch.isfinite(logp).all()) and bool((logp <= 0).all())
    # a ban renormalises: every step chose from V words less what the tables ban for the row (no other control is on)
    entries = [ex.shared.tolist() + ex.per_clip[b].tolist() for b in range(CLIPS)]
    for r in (0, N, CLIPS * N - 1):
        row = ids[r].tolist()
        for t in range(L):
            banned = {excluded_word(row[:t], e, V) for e in entries[r // N]} - {None}
            assert int(kept[r, t]) == V - len(banned), (r, t)
    # the per-clip ban sits at step 0 of every row of its own clip and of no other clip's
    assert bool((kept[:, 0] == V - 1).all())


@pytest.mark.parametrize('share', [False, True])
def test_a_row_that_meets_no_entry_keeps_its_words(share):
    plain, ex, (ids, logp, lens, kept), _, _ = drawn(share)
    L = ids.shape[1]
    hit = exclusions_hit(plain[0].view(CLIPS, N, L), plain[2].view(CLIPS, N), ex).view(-1)
    free = [r for r in range(CLIPS * N) if int(hit[r]) == 0]
    assert free and len(free) < CLIPS * N
    for r in free:                                     # the noise does not depend on the bans: the same words up to <end>
        n = int(plain[2][r])
        assert ids[r, :n].tolist() == plain[0][r, :n].tolist() and int(lens[r]) == n, r


def test_row_to_clip_mapping_with_per_clip_tables():
    """n = 3, every clip bans another word at step 0 -- the word its neighbour's first row drew: rows b*n .. b*n+n-1 read clip b's
    table under share_encoder False and True alike"""
    net, _, frames, regions = host_net()
    V = net.decoder.vocab_size
    for share in (False, True):
        plain = net.sample(frames, regions, n=N, seed=9, share_encoder=share)[0]
        first = plain[:, 0].view(CLIPS, N)
        words = [int(first[b, 0]) for b in range(CLIPS)]
        assert len(set(words)) > 1
        ex = pack_exclusions(net.decoder.vocab, per_clip=[[w] for w in words])
        del net.ops.excl_calls[:]
        ids = net.sample(frames, regions, n=N, seed=9, share_encoder=share, exclude=ex)[0]
        assert len(net.ops.excl_calls) == net.decoder.max_words
        assert all(sh is None and pc.shape == ex.per_clip.shape and rpc == N for sh, pc, rpc in net.ops.excl_calls)
        got = ids[:, 0].view(CLIPS, N)
        for b in range(CLIPS):
            assert words[b] not in got[b].tolist(), (share, b)
            for i in range(N):                                         # another clip's word is not banned here
                if int(first[b, i]) != words[b]:
                    assert int(got[b, i]) == int(first[b, i]), (share, b, i)


def test_temperature_zero_is_greedy_over_what_is_left():
    net, _, frames, regions = host_net()
    greedy = net.sample(frames, regions, n=1, temperature=0.0, seed=1)
    caps = caption_words(greedy[0], greedy[2])
    ex = pack_exclusions(net.decoder.vocab, words=[caps[0][0]], per_clip=[[]] + [[tuple(c[:2])] for c in caps[1:]])
    ids, logp, lens, kept = net.sample(frames, regions, n=1, temperature=0.0, seed=1, exclude=ex, return_kept=True)
    assert int(exclusions_hit(ids, lens, ex).sum()) == 0 and not torch.equal(ids, greedy[0])
    again = net.sample(frames, regions, n=1, temperature=0.0, seed=77, exclude=ex)
    assert torch.equal(again[0], ids) and torch.equal(again[2], lens)
    assert int(kept[0, 0]) == net.decoder.vocab_size - 1


def test_exclusions_join_the_other_controls():
    net, _, frames, regions = host_net()
    vocab = net.decoder.vocab
    opts = dict(n=N, seed=13, top_k=6, top_p=0.9, min_len=3, no_repeat_ngram=2)
    plain = net.sample(frames, regions, **opts)
    common = collections.Counter(w for c in caption_words(plain[0], plain[2]) for w in set(c) if w >= 4).most_common(1)[0][0]
    ex = pack_exclusions(vocab, words=[common])
    ids, logp, lens, kept = net.sample(frames, regions, exclude=ex, return_kept=True, **opts)
    assert not bool((ids == common).any()) and bool((kept >= 1).all()) and bool((kept <= 6).all()) and bool((lens > 3).all())
    assert bool(torch.isfinite(logp).all())


def test_a_row_with_no_word_left_takes_word_zero():
    """the emulated step, directly: entries that ban the whole vocabulary of the rows of clip 1"""
    V, rows = 37, 6
    ops = SampleExclEmul()
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(3))
    emb = torch.randn(V, 8, generator=torch.Generator().manual_seed(4))
    per_clip = torch.full((3, 32, 2), -1, dtype=torch.int64)
    per_clip[1, :, 0] = torch.arange(5, 37)
    shared = torch.tensor([[w, -1] for w in range(5)])
    out = dict(ids=torch.zeros(rows, dtype=torch.int64), we=torch.zeros(rows, 8), logp=torch.zeros(rows), lens=torch.full((rows,), 9),
               kept=torch.zeros(rows, dtype=torch.int32))
    ops.sample_excl_embed(x, emb, out['ids'], out['we'], out['logp'], out['lens'], 0, 2, seed=5, site_sample=3, kept=out['kept'],
                          excl_shared=shared, excl_clip=per_clip, rows_per_clip=2)
    assert out['kept'].tolist() == [32, 32, 0, 0, 32, 32] and out['ids'][2:4].tolist() == [0, 0]
    assert bool((out['ids'][[0, 1, 4, 5]] >= 5).all())


# ---------------------------------------------------------------------------------------------- which op a word step launches
def recorded(net, call):
    net.ops.recording = []
    try:
        call()
        return net.ops.recording
    finally:
        net.ops.recording = None


def test_exclude_none_and_empty_tables_launch_what_is_launched_today():
    net, _, frames, regions = host_net()
    vocab, L = net.decoder.vocab, net.decoder.max_words
    empties = (None, Exclusions(None, None), pack_exclusions(vocab, per_clip=[[]] * CLIPS),
               Exclusions(torch.zeros(0, 2, dtype=torch.int64), torch.zeros(CLIPS, 0, 2, dtype=torch.int64)))
    for opts in (dict(), dict(min_len=2), dict(top_k=3, share_encoder=True)):
        today = recorded(net, lambda: net.sample(frames, regions, n=N, seed=1, **opts))
        assert 'sample_excl_embed' not in today
        for ex in empties:
            assert recorded(net, lambda: net.sample(frames, regions, n=N, seed=1, exclude=ex, **opts)) == today, opts
        ex = pack_exclusions(vocab, words=[10])
        got = recorded(net, lambda: net.sample(frames, regions, n=N, seed=1, exclude=ex, **opts))
        assert got.count('sample_excl_embed') == L and 'sample_embed' not in got and 'sample_filter_embed' not in got
        step = 'sample_filter_embed' if opts.get('min_len') or opts.get('top_k') else 'sample_embed'
        assert [c for c in got if c != 'sample_excl_embed'] == [c for c in today if c != step]
    today = recorded(net, lambda: net.sample_without_replacement(frames, regions, n=3, seed=1))
    assert today.count('beam_select_gumbel') == L
    for ex in empties:
        assert recorded(net, lambda: net.sample_without_replacement(frames, regions, n=3, seed=1, exclude=ex)) == today
    got = recorded(net, lambda: net.sample_without_replacement(frames, regions, n=3, seed=1, exclude=pack_exclusions(vocab, words=[10])))
    assert got.count('beam_select_gumbel_excl') == L and 'beam_select_gumbel' not in got
    assert [c for c in got if c != 'beam_select_gumbel_excl'] == [c for c in today if c != 'beam_select_gumbel']


def test_scst_without_exclude_is_the_step_of_today():
    net, _, frames, regions = host_net()
    vids = [str(b) for b in range(CLIPS)]
    logs = []
    for so in (None, dict(exclude=None), dict(exclude=Exclusions(None, None))):
        tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=N, baseline='greedy', sample_options=so, lr=0.0)
        net.seed_counter = 7
        logs.append(recorded(net, lambda: tr.step(frames, regions, vids)))
    assert logs[0] == logs[1] and 'sample_excl_embed' not in logs[0]
    assert logs[2] == logs[0]


# ---------------------------------------------------------------------------------------------- without replacement
def test_sample_without_replacement_under_exclusions():
    net, _, frames, regions = host_net()
    vocab, L = net.decoder.vocab, net.decoder.max_words
    end = vocab('<end>')
    plain = net.sample_without_replacement(frames, regions, n=N, seed=5)
    flat = plain[0].view(-1, L)
    ex, _, _ = exclusions_from_draw(flat, plain[2].view(-1), vocab, N)
    assert bool((exclusions_hit(plain[0], plain[2], ex) > 0).any(1).all())
    ids, logp, lens = net.sample_without_replacement(frames, regions, n=N, seed=5, exclude=ex)
    finite = logp > -INF
    assert bool(finite[:, 0].all()) and int(exclusions_hit(ids, lens, ex)[finite].sum()) == 0
    for clip in ids.tolist():
        assert len({tuple(r) for r in clip}) == N                      # still distinct
    fn = dlsg_amd.sample_without_replacement(net, frames, regions, n=N, seed=5, exclude=ex)
    assert all(torch.equal(a, b) for a, b in zip(fn, (ids, logp, lens)))
    # one beam draws what sample draws, under the exclusions too
    one = net.sample_without_replacement(frames, regions, n=1, seed=5, exclude=ex)
    want = net.sample(frames, regions, n=1, seed=5, exclude=ex)
    for b in range(CLIPS):
        n = int(want[2][b])
        assert int(one[2][b, 0]) == n and one[0][b, 0, :n].tolist() == want[0][b, :n].tolist()
        assert abs(float(one[1][b, 0]) - float(want[1][b, :n].double().sum())) <= 1e-5
        assert bool((one[0][b, 0, n:] == end).all())


def test_consensus_search_passes_the_exclusions_on():
    net, _, frames, regions = host_net()
    reward = S.CiderD(corpus_for(net.decoder.vocab, CLIPS)).to_device(net.decoder.vocab, device='cpu')
    reward.ops = net.ops
    ex = pack_exclusions(net.decoder.vocab, words=[10, 11, 12])
    opts = dict(n=4, temperature=0.9, seed=21, exclude=ex)
    want = dlsg_amd.consensus_rerank(reward, *net.sample_without_replacement(frames, regions, **opts), n_best=2)
    got = consensus_search(net, frames, regions, reward, n_best=2, stochastic=opts)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not bool(((got[0] == 10) | (got[0] == 11) | (got[0] == 12)).any())


# ---------------------------------------------------------------------------------------------- SCST
def renamed_vocab(net, words):
    """the vocabulary with the ids `words` renamed to the first of BAD_ENDINGS"""
    vocab = net.decoder.vocab
    for i, name in zip(words, BAD_ENDINGS):
        old = vocab.idx2word[i]
        vocab.idx2word[i] = name
        vocab.word2idx[name] = vocab.word2idx.pop(old)
    return vocab


@pytest.mark.parametrize('share', [False, True])
def test_scst_step_samples_and_baselines_under_the_exclusions(share):
    net, _, frames, regions = synth_pair(SEED, CLIPS, end_bias=1.0, ops=SampleExclEmul())
    L = net.decoder.max_words
    vids = [str(b) for b in range(CLIPS)]
    plain = net.sample(frames, regions, n=N, seed=3)
    stops = collections.Counter(c[-2] for c in caption_words(plain[0], plain[2]) if 2 <= len(c) < L and c[-2] >= 4)
    vocab = renamed_vocab(net, [w for w, _ in stops.most_common(3)])
    ex = pack_exclusions(vocab, suppress_unk=True, bad_endings=True)
    assert ex.per_clip is None and ex.shared.shape[0] >= 3
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=N, baseline='greedy', share_encoder=share,
                              sample_options=dict(exclude=ex, min_len=2), lr=0.0)
    seen = _spy(tr)
    net.train()
    log = recorded(net, lambda: tr.step(frames, regions, vids))
    assert net.training                                                # (the baseline ran in eval mode and put the mode back)
    assert log.count('sample_excl_embed') == 2 * L and 'sample_embed' not in log and 'argmax' not in log
    (fx, rx, ids, lens, tf), kw = seen[0]
    want = net.sample(frames, regions, n=N, seed=kw['seed'], share_encoder=share, exclude=ex, min_len=2)
    assert torch.equal(ids, want[0]) and torch.equal(lens, want[2])
    net.eval()
    greedy = net.sample(frames, regions, n=1, temperature=0.0, seed=0, exclude=ex)
    bad = {vocab(w) for w in BAD_ENDINGS if w in vocab.word2idx}
    unk = vocab('<unk>')
    for got_ids, got_lens in ((ids, lens), (greedy[0], greedy[2])):
        assert int(exclusions_hit(got_ids, got_lens, ex).sum()) == 0
        for c in caption_words(got_ids, got_lens):
            assert unk not in c and not (len(c) >= 2 and c[-1] == vocab('<end>') and c[-2] in bad)
    r = LengthReward().scores([v for v in vids for _ in range(N)], [net.decoder.decode_tokens(x) for x in ids])
    b = np.repeat(LengthReward().scores(vids, [net.decoder.decode_tokens(x) for x in greedy[0]]), N)
    assert np.array_equal(kw['seq_weights'].numpy(), (r - b).astype(np.float32))
    # the greedy caption is what beam_search(beam_size=1, exclude=...) decodes: evaluation's caption
    beam = net.beam_search(frames, regions, beam_size=1, exclude=ex)
    for b_ in range(CLIPS):
        n = int(beam[2][b_, 0])
        assert greedy[0][b_, :n].tolist() == beam[0][b_, 0, :n].tolist() and int(greedy[2][b_]) == n


# ---------------------------------------------------------------------------------------------- the graph classes
class ReplayStub(object):
    def replay(self):
        pass


def test_the_sampling_graphs_keep_their_own_exclusions(monkeypatch):
    monkeypatch.setattr(graphs, 'capture', lambda dev, body, warmup=None: (ReplayStub(), body()))
    net, _, frames, regions = host_net()
    ex = pack_exclusions(net.decoder.vocab, words=[10, 11], per_clip=[[(12, 13)], [14], [], []])
    del net.ops.excl_calls[:]
    g = dlsg_amd.SampleGraph(net, frames, regions, N, 1.0, min_len=2, exclude=ex)
    assert g.options == dict(top_k=0, top_p=1.0, min_len=2, no_repeat_ngram=0, return_kept=False) and isinstance(g.exclude, Exclusions)
    for mine, theirs in zip(g.exclude, ex):
        assert torch.equal(mine, theirs) and mine.data_ptr() != theirs.data_ptr()
    assert all(sh is g.exclude.shared and pc is g.exclude.per_clip for sh, pc, _ in net.ops.excl_calls) and net.ops.excl_calls
    plain = dlsg_amd.SampleGraph(net, frames, regions, N, 1.0, min_len=2)
    assert plain.exclude is None and plain.options == g.options
    del net.ops.excl_calls[:]
    s = dlsg_amd.StochasticBeamGraph(net, frames, regions, n=3, min_len=2, exclude=ex)
    assert s.options == dict(min_len=2) and all(sh is s.exclude.shared and pc is s.exclude.per_clip for sh, pc, _ in net.ops.excl_calls)
    assert len(net.ops.excl_calls) == net.decoder.max_words
    assert dlsg_amd.StochasticBeamGraph(net, frames, regions, n=3).exclude is None


# ---------------------------------------------------------------------------------------------- refusals
@torch.no_grad()
def test_what_is_refused_names_the_combination():
    net, _, frames, regions = host_net()
    vocab = net.decoder.vocab
    ex = pack_exclusions(vocab, words=[10])
    clipped = pack_exclusions(vocab, per_clip=[[10]] * CLIPS)
    with pytest.raises(ValueError, match='not covered in constrained beam search'):
        net.constrained_beam_search(frames, regions, [[10]] * CLIPS, exclude=ex)
    with pytest.raises(ValueError, match='not covered in constrained beam search'):
        dlsg_amd.constrained_beam_search(net, frames, regions, [[10]] * CLIPS, exclude=ex)
    with pytest.raises(ValueError, match='not covered in diverse beam search'):
        net.beam_search(frames, regions, beam_size=4, num_groups=2, exclude=ex)
    loader = [(frames, regions, None, ['v%d' % b for b in range(CLIPS)])]
    with pytest.raises(ValueError, match='exclude and constraints cannot be combined'):
        S.gather_results(net, loader, decode=dict(beam_size=3, exclude=ex, constraints=lambda vids: [[10]] * CLIPS))
    with pytest.raises(ValueError, match='per-clip part is not covered in SCSTTrainer'):
        dlsg_amd.SCSTTrainer(net, LengthReward(), sample_options=dict(exclude=clipped))
    with pytest.raises(ValueError, match='exclude: an Exclusions'):
        dlsg_amd.SCSTTrainer(net, LengthReward(), sample_options=dict(exclude=[10]))
    with pytest.raises(ValueError, match='unknown keys'):
        dlsg_amd.SCSTTrainer(net, LengthReward(), sample_options=dict(excluded=ex))
    # the tables: B clips, not B*n rows
    rows = pack_exclusions(vocab, per_clip=[[10]] * (CLIPS * N))
    for call in (lambda e: net.sample(frames, regions, n=N, exclude=e), lambda e: net.sample(frames, regions, n=N, share_encoder=True, exclude=e),
                 lambda e: net.sample_without_replacement(frames, regions, n=N, exclude=e)):
        with pytest.raises(ValueError, match='holds %d clips, the batch %d' % (CLIPS * N, CLIPS)):
            call(rows)
        with pytest.raises(ValueError, match='exclude: an Exclusions'):
            call([10])
        with pytest.raises(ValueError, match='int64 tensor'):
            call(Exclusions(torch.zeros(2, 2), None))
        with pytest.raises(ValueError, match='at most 64 entries'):
            call(Exclusions(torch.zeros(65, 2, dtype=torch.int64), None))
        with pytest.raises(ValueError, match='words per entry'):
            call(Exclusions(torch.zeros(2, 2, dtype=torch.int64), torch.zeros(CLIPS, 1, 3, dtype=torch.int64)))
    with pytest.raises(ValueError, match='return_kept needs one of'):
        net.sample(frames, regions, return_kept=True, exclude=Exclusions(None, None))
    assert len(net.sample(frames, regions, return_kept=True, exclude=ex)) == 4            # allowed with exclude alone
    # the step's own arguments
    with pytest.raises(ValueError, match='rows_per_clip'):
        E.dec_sample(net.ops, net.decoder, *decoder_inputs(net, frames, regions), exclude=ex, rows_per_clip=3)
    with pytest.raises(ValueError, match='rows_per_clip'):
        E.dec_sample(net.ops, net.decoder, *decoder_inputs(net, frames, regions), exclude=ex, rows_per_clip=0)
    with pytest.raises(ValueError, match='vocabulary 40000 > 32768'):
        E.sample_exclusions(ex, CLIPS, frames.device, 26, 40000)
    with pytest.raises(ValueError, match='at most 64 words of history'):
        E.sample_exclusions(ex, CLIPS, frames.device, 65, 50)
    assert E.sample_exclusions(Exclusions(None, None), CLIPS, frames.device, 65, 40000) is None
    for cls in (dlsg_amd.CapBaseline1, dlsg_amd.CapBaselineModel):
        with pytest.raises(NotImplementedError):
            cls.sample(None, frames, regions, exclude=ex)
    # an ops object without the steps under exclusions (the beam step's emulator): refused before the encoder runs, by an error that
    # is a ValueError and, as while these calls took no such keyword, a TypeError
    assert issubclass(ExcludeNotCovered, ValueError) and issubclass(ExcludeNotCovered, TypeError)
    old, _, f2, r2 = synth_pair(SEED, 2, ops=ExclEmul())
    with pytest.raises(ExcludeNotCovered, match='exclude: ExclEmul has no sample_excl_embed'):
        old.sample(f2, r2, exclude=ex)
    with pytest.raises(ExcludeNotCovered, match='exclude: ExclEmul has no beam_select_gumbel_excl'):
        old.sample_without_replacement(f2, r2, n=2, exclude=ex)
    with pytest.raises(ValueError, match="unknown keys \\['exclude'\\] \\(top_k, top_p, min_len, no_repeat_ngram\\)"):
        dlsg_amd.SCSTTrainer(old, LengthReward(), sample_options=dict(exclude=ex))
    assert old.beam_search(f2, r2, beam_size=2, exclude=ex)[0].shape[0] == 2          # (the step it has)


@torch.no_grad()
def decoder_inputs(net, frames, regions):
    """(mems, sv, L, training, seed, temperature) of a `dec_sample` call on the CLIPS clips"""
    sv = {}
    _, mems = net._encoder_pass(frames, regions, False, 1, sv, 1)
    return list(mems), sv, net.decoder.max_words, False, 1, 1.0


@torch.no_grad()
def test_dec_sample_runs_the_new_step():
    net, _, frames, regions = host_net()
    ex = pack_exclusions(net.decoder.vocab, words=[10, 11, 12, 13])
    s = E.dec_sample(net.ops, net.decoder, *decoder_inputs(net, frames, regions), exclude=ex)
    ids = s['IDS'][1:].t()
    assert 'KEPT' in s and bool((s['KEPT'] == net.decoder.vocab_size - 4).all())
    assert not bool(((ids >= 10) & (ids <= 13)).any())
    assert 'KEPT' not in E.dec_sample(net.ops, net.decoder, *decoder_inputs(net, frames, regions), exclude=None)


def test_every_entry_point_takes_the_keyword():
    for fn in (dlsg_amd.CapGnnModel.sample, dlsg_amd.CapGnnModel.sample_without_replacement, dlsg_amd.stochastic_nbest, E.dec_sample,
               dlsg_amd.SampleGraph.__init__):
        assert inspect.signature(fn).parameters['exclude'].default is None
    from dlsg_amd import abi
    base = len(abi.functions['dlsg_sample_filter_embed'][1])
    assert len(abi.functions['dlsg_sample_excl_embed'][1]) == base + 6
    assert len(abi.functions['dlsg_beam_select_gumbel_excl'][1]) == len(abi.functions['dlsg_beam_select_gumbel'][1]) + 5
    assert abi.defines['DLSG_ABI_VERSION'] == 8
    from dlsg_amd.hip import HipOps
    assert callable(HipOps.sample_excl_embed) and callable(HipOps.beam_select_gumbel_excl)


def test_the_emulation_masks_what_the_rule_bans():
    """`banned_by_tables` on a hand-made case: a one-word entry, a bigram behind its first word, an entry longer than the history, a
    cut entry, and clips that differ"""
    shared = torch.tensor([[7, -1, -1], [3, 4, -1], [1, 2, 3], [5, 99, 6]])
    per_clip = torch.tensor([[[8, -1, -1]], [[4, 9, -1]]])
    hist = [[3], [3, 4], [1, 2], [4]]
    got = banned_by_tables(hist, [0, 0, 1, 1], shared, per_clip, 2, 50)
    assert got == [{7, 4, 5, 8}, {7, 5, 8}, {7, 3, 5}, {7, 5, 9}]
    x = masked(torch.zeros(4, 50), got)
    assert [int((x[r] == -INF).sum()) for r in range(4)] == [4, 3, 3, 3] and float(x[0, 7]) == -INF and float(x[1, 4]) == 0.0

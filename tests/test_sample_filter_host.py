"""CPU: the sampling controls (top_k, top_p, min_len, no_repeat_ngram) through `CapGnnModel.sample` and `SCSTTrainer` -- what
they promise about the captions, which op a word step launches, the argument checks.  `dlsg_sample_filter_embed` is emulated in
float64 numpy (`SampleFilterEmul`, on tests/emul_sample.py); the GPU side is tests/test_gpu_sample_filter.py."""
import numpy as np
import pytest
import torch

import dlsg_amd
from emul_sample import apply_bans, kept_sets, tempered
from test_scst_host import LengthReward, ScstEmul, _spy, gumbel_keys, small_net


class SampleFilterEmul(ScstEmul):
    """ScstEmul + sample_filter_embed: the rules of include/dlsg.h restated in float64"""

    def sample_filter_embed(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature=1.0, p=0.0, seed=0, site=0,
                            site_sample=0, row0=0, top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, hist=None, kept=None):
        if torch.is_tensor(seed):
            seed = int(seed.item())
        z = apply_bans(tempered(logits, temperature), None if hist is None else hist.numpy(), t, no_repeat_ngram, min_len, end_id)
        if temperature > 0:
            keep = kept_sets(z, top_k, top_p)[0]
            keys = gumbel_keys(logits, temperature, seed, site_sample, row0)
        else:
            keep = z > -np.inf
            keys = z
        ids = np.where(keep, keys, -np.inf).argmax(1)                    # nothing kept: word 0
        zk = np.where(keep, z, -np.inf)
        m = zk.max(1)
        with np.errstate(invalid='ignore', divide='ignore'):
            lse = m + np.log(np.exp(zk - m[:, None]).sum(1))
            lp = z[np.arange(len(ids)), ids] - lse
        ids = torch.from_numpy(ids)
        ids_out.copy_(ids)
        logp.copy_(torch.from_numpy(lp).float())
        if kept is not None:
            kept.copy_(torch.from_numpy(keep.sum(1).astype(np.int32)))
        hit = (ids == end_id) & (lens > t)
        lens.copy_(torch.where(hit, torch.full_like(lens, t + 1), lens))
        self.embed_fwd(E, ids, out, p=p, seed=seed, site=site, row0=row0)


def filter_net(end_bias=1.2, **kw):
    net, sd, args, vocab, frames, regions, _, _ = small_net(**kw)
    net.set_ops(SampleFilterEmul())
    net.decoder.word_restore.bias.data[vocab('<end>')] += end_bias        # some captions end early
    return net, vocab, frames, regions


def repeated_bigrams(ids, lens):
    """rows whose words before <end> hold the same bigram twice"""
    bad = []
    for r in range(ids.shape[0]):
        w = ids[r, :int(lens[r])].tolist()
        grams = list(zip(w[:-1], w[1:]))
        if len(grams) != len(set(grams)):
            bad.append(r)
    return bad


def test_top_k_one_is_greedy():
    net, vocab, frames, regions = filter_net()
    want = net.sample(frames, regions, n=3, temperature=0.0, seed=5)
    got = net.sample(frames, regions, n=3, temperature=1.0, seed=5, top_k=1, return_kept=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert (got[1] == 0).all() and (got[3] == 1).all()
    assert got[3].shape == got[0].shape and got[3].dtype == torch.int32


def test_min_len_keeps_end_away():
    net, vocab, frames, regions = filter_net(end_bias=6.0)
    L = net.decoder.max_words
    plain = net.sample(frames, regions, n=4, seed=11)
    assert (plain[2] <= 5).any()                                      # without the control captions do end this early
    for m in (1, 5, L):
        ids, logp, lens = net.sample(frames, regions, n=4, seed=11, min_len=m)
        assert (lens > m).all() if m < L else (lens == L).all()
        assert (ids[:, :m] != vocab('<end>')).all() and torch.isfinite(logp).all()


def test_no_repeat_ngram_blocks_bigrams():
    net, vocab, frames, regions = filter_net(end_bias=-4.0)
    plain = net.sample(frames, regions, n=4, temperature=0.25, seed=3)
    assert repeated_bigrams(plain[0], plain[2])                       # sharp sampling loops without the control
    ids, logp, lens, kept = net.sample(frames, regions, n=4, temperature=0.25, seed=3, no_repeat_ngram=2, return_kept=True)
    assert repeated_bigrams(ids, lens) == []
    assert torch.isfinite(logp).all() and (kept < len(vocab)).any() and (kept <= len(vocab)).all()


def test_filters_compose_and_logp_is_the_truncated_log_probability():
    net, vocab, frames, regions = filter_net()
    ids, logp, lens, kept = net.sample(frames, regions, n=4, seed=9, top_k=5, top_p=0.9, min_len=3, no_repeat_ngram=2,
                                       return_kept=True)
    assert (kept >= 1).all() and (kept <= 5).all() and (lens > 3).all() and repeated_bigrams(ids, lens) == []
    assert (logp <= 0).all() and (logp[kept == 1] == 0).all()
    full = net.sample(frames, regions, n=4, seed=9)
    assert not torch.equal(full[0], ids)
    again = net.sample(frames, regions, n=4, seed=9, top_k=5, top_p=0.9, min_len=3, no_repeat_ngram=2)
    assert len(again) == 3 and torch.equal(again[0], ids) and torch.equal(again[1], logp) and torch.equal(again[2], lens)


def test_which_op_a_word_step_launches():
    net, vocab, frames, regions = filter_net()
    L = net.decoder.max_words
    net.ops.recording = []
    net.sample(frames, regions, n=2, seed=1)
    log = net.ops.recording
    assert log.count('sample_embed') == L and 'sample_filter_embed' not in log
    for opts in (dict(top_k=3), dict(top_p=0.5), dict(min_len=2), dict(no_repeat_ngram=3), dict(top_k=3, top_p=0.5)):
        net.ops.recording = []
        net.sample(frames, regions, n=2, seed=1, **opts)
        got = net.ops.recording
        assert got.count('sample_filter_embed') == L and 'sample_embed' not in got, opts
        assert [c for c in got if c != 'sample_filter_embed'] == [c for c in log if c != 'sample_embed'], opts
    net.ops.recording = None


def test_bad_options_raise():
    net, vocab, frames, regions = filter_net()
    L = net.decoder.max_words
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(min_len=-1), dict(min_len=L + 1),
                dict(no_repeat_ngram=-1), dict(return_kept=True)):
        with pytest.raises(ValueError):
            net.sample(frames, regions, **bad)
    with pytest.raises(ValueError):
        dlsg_amd.SCSTTrainer(net, LengthReward(), sample_options=dict(top_p=2.0))
    with pytest.raises(ValueError):
        dlsg_amd.SCSTTrainer(net, LengthReward(), sample_options=dict(temperature=2.0))
    from dlsg_amd.hip import SAMPLE_FILTER_MAXV
    from dlsg_amd import engine as E
    with pytest.raises(ValueError):
        E.check_sample_options(L, top_k=5, vocab_size=SAMPLE_FILTER_MAXV + 1)
    assert E.check_sample_options(L, vocab_size=SAMPLE_FILTER_MAXV + 1) is False      # the plain kernel has no such bound
    assert E.check_sample_options(L, top_k=5, vocab_size=SAMPLE_FILTER_MAXV) is True


def test_scst_with_top_k_one_and_the_greedy_baseline_has_zero_advantages():
    net, vocab, frames, regions = filter_net()
    tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=3, baseline='greedy', sample_options=dict(top_k=1), lr=0.0)
    seen = _spy(tr)
    out = tr.step(frames, regions, ['0', '1', '2'])
    (fx, rx, ids, lens, tf), kw = seen[0]
    with torch.no_grad():
        greedy = net(frames, regions, None)[0]
    assert torch.equal(ids, greedy.repeat_interleave(3, 0))
    assert (kw['seq_weights'] == 0).all() and out['reward_mean'] == out['baseline_mean']


def test_scst_without_sample_options_is_the_plain_step():
    stats = []
    for kw in ({}, {'sample_options': None}, {'sample_options': {}}):
        net, vocab, frames, regions = filter_net()
        tr = dlsg_amd.SCSTTrainer(net, LengthReward(), n_samples=3, lr=0.0, **kw)
        net.ops.recording = []
        out = tr.step(frames, regions, ['0', '1', '2'])
        assert 'sample_filter_embed' not in net.ops.recording
        net.ops.recording = None
        stats.append((float(out['loss']), out['reward_mean'], net._gflat.clone()))
    assert all(s[0] == stats[0][0] and s[1] == stats[0][1] and torch.equal(s[2], stats[0][2]) for s in stats[1:])

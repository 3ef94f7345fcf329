"""Test-only restatement of the two force launches of a decode under a forced prefix (dlsg_beam_force_prefix,
dlsg_sample_force_prefix) in torch, with float64 values, on top of the emulated ops of every decode that takes the keyword: the
history steps (hist, ens, excl, cons, phrases), the three sampled steps and `seq_logprob`.  `prefix_lens` states once what a
clip's prefix is; `force_calls` notes the step of every force launch."""
import torch

from emul_ensemble import INF, combined_logp
from emul_phrases import PhraseEmul
from emul_sample_excl import SampleExclEmul
from emul_seqscore import SeqScoreEmul


def prefix_lens(prefix, V):
    """per clip the length of the leading run of ids in [0, V) of its row: a list of ints"""
    out = []
    for row in prefix.tolist():
        n = 0
        while n < len(row) and 0 <= row[n] < V:
            n += 1
        out.append(n)
    return out


def forced_value(logits_list, weights, mode, row, word):
    """the combined log-prob of `word` on beam row `row`, float64: log-softmax per member, then the members' combination"""
    return float(combined_logp([x[row:row + 1] for x in logits_list], weights, mode)[0, word])


class PrefixEmul(SampleExclEmul, PhraseEmul, SeqScoreEmul):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.force_calls = []

    def beam_force_prefix(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                          prefix):
        assert len(logits_list) == len(weights) and mode in (0, 1)
        R, V = logits_list[0].shape
        B, L = R // k, hist_out.shape[1]
        assert prefix.dtype == torch.int64 and prefix.shape[0] == B and prefix.shape[1] <= L - 1 and 0 <= t < L
        object.__getattribute__(self, 'force_calls').append(('beam', t))
        for b, p in enumerate(prefix_lens(prefix, V)):
            if t >= p:
                continue                                               # nothing of this clip is written
            word, row = int(prefix[b, t]), b * k
            value = forced_value(logits_list, weights, mode, row, word) + (0.0 if t == 0 else float(last_lp[row]))
            h = (hist_in[row, :t].tolist() if t else []) + [word] + [end] * (L - t - 1)
            for c in range(k):
                o = row + c
                pred[o], back[o], rows[o] = word, 0, row
                new_lp[o] = value if c == 0 else -INF
                hist_out[o] = torch.tensor(h, dtype=torch.int64)

    def sample_force_prefix(self, logits, E, ids_out, out, logp, lens, t, prefix, L, temperature=1.0, p=0.0, seed=0, site=0, row0=0,
                            rows_per_clip=1, kept=None):
        rows, V = logits.shape
        assert rows % rows_per_clip == 0 and prefix.shape[0] == rows // rows_per_clip and prefix.shape[1] <= L - 1 and 0 <= t < L
        object.__getattribute__(self, 'force_calls').append(('sample', t))
        if torch.is_tensor(seed):
            seed = int(seed.item())
        plen = prefix_lens(prefix, V)
        forced = [r for r in range(rows) if t < plen[r // rows_per_clip]]
        if not forced:
            return
        lp = torch.log_softmax(logits.double() / temperature if temperature > 0 else logits.double(), 1)
        ids = ids_out.clone()
        for r in forced:
            ids[r] = int(prefix[r // rows_per_clip, t])
        rows_out = torch.empty_like(out)
        PrefixEmul.embed_fwd(self, E, ids, rows_out, p=p, seed=seed, site=site, row0=row0)    # the stream of the rows row0 + r
        for r in forced:
            ids_out[r] = ids[r]
            logp[r] = float(lp[r, ids[r]])
            lens[r] = L
            out[r] = rows_out[r]
            if kept is not None:
                kept[r] = 1

"""Test-only emulation of the two sampling steps under exclusions (dlsg_sample_excl_embed, dlsg_beam_select_gumbel_excl), by
composition: a banned word is one whose logit is -inf, so each new op masks the words the rule bans for a row -- `banned_by_tables`,
on `emul_excl.table_entries` and `emul_excl.excluded_word` -- and runs the emulation of the step without tables on the masked
logits (`SampleFilterEmul.sample_filter_embed`, whose other bans are `emul_sample.apply_bans`, and `SbsEmul.beam_select_gumbel`).
That is also what the GPU tests compare the kernels with: the existing kernel on the masked logits."""
import torch

from emul_excl import ExclEmul, excluded_word, table_entries
from emul_sbs import SbsEmul
from test_sample_filter_host import SampleFilterEmul
from test_seq_per_clip_host import SeqEmul


def banned_by_tables(histories, clip_of_row, shared, per_clip, clips, V):
    """per row the set of words the two tables ban: histories[r] the row's words so far (a list), clip_of_row[r] its clip"""
    entries = table_entries(shared, per_clip, clips, V)
    return [{excluded_word(h, list(e), V) for e in entries[c]} - {None} for h, c in zip(histories, clip_of_row)]


def masked(logits, banned):
    """a copy of the (rows, V) logits with each row's banned words at -inf"""
    x = logits.clone()
    for r, words in enumerate(banned):
        if words:
            x[r, sorted(words)] = -float('inf')
    return x


class SampleExclEmul(SampleFilterEmul, SeqEmul, SbsEmul, ExclEmul):
    """the emulated ops of a model that samples, trains (SCST, shared encoder) and searches, stochastically and under exclusions,
    plus the two new ops; `excl_calls` notes the tables each of them was handed"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.excl_calls = []

    def sample_excl_embed(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature=1.0, p=0.0, seed=0, site=0, site_sample=0,
                          row0=0, top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, hist=None, kept=None, excl_shared=None,
                          excl_clip=None, rows_per_clip=1):
        rows, V = logits.shape
        if rows_per_clip < 1 or rows % rows_per_clip:
            raise ValueError('sample_excl_embed: %d rows are not clips of rows_per_clip = %r rows' % (rows, rows_per_clip))
        clips = rows // rows_per_clip
        assert excl_clip is None or excl_clip.shape[0] == clips, (excl_clip.shape, clips)
        assert t == 0 or hist is not None or (excl_shared is None and excl_clip is None)
        object.__getattribute__(self, 'excl_calls').append((excl_shared, excl_clip, rows_per_clip))
        histories = [[int(hist[i][r]) for i in range(t)] for r in range(rows)]
        banned = banned_by_tables(histories, [r // rows_per_clip for r in range(rows)], excl_shared, excl_clip, clips, V)
        SampleFilterEmul.sample_filter_embed(self, masked(logits, banned), E, ids_out, out, logp, lens, t, end_id, temperature, p, seed,
                                             site, site_sample, row0, top_k, top_p, min_len, no_repeat_ngram, hist, kept)

    def beam_select_gumbel_excl(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, G_in, G_out,
                                excl_shared=None, excl_clip=None, temperature=1.0, seed=0, site_sample=0, no_repeat_ngram=0, min_len=0,
                                ended_count=None):
        R, V = logits.shape
        assert excl_clip is None or excl_clip.shape[0] == R // k, (excl_clip.shape, R, k)
        object.__getattribute__(self, 'excl_calls').append((excl_shared, excl_clip, k))
        histories = [hist_in[r, :t].tolist() for r in range(R)]
        banned = banned_by_tables(histories, [r // k for r in range(R)], excl_shared, excl_clip, R // k, V)
        SbsEmul.beam_select_gumbel(self, masked(logits, banned), last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                                   G_in, G_out, temperature, seed, site_sample, no_repeat_ngram, min_len, ended_count)

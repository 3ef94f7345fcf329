"""Test-only emulation of the ensemble's sampled word step (dlsg_sample_ens), by composition: the combined values are
`emul_ensemble.combined_logp` (float64 from torch.log_softmax, stored as the float32 workspace the kernel fills), and the draw is the
emulation of the sampled step under exclusions on those values as its logits (`emul_sample_excl.SampleExclEmul.sample_excl_embed`, whose
bans, thresholds and noise are the existing sample emulators').  That is also what the GPU tests compare the kernel with: its `comb`
with `combined_logp`, its draw with the existing kernels on `comb`."""
import torch

from emul_ensemble import combined_logp
from emul_sample_excl import SampleExclEmul
from emul_seqscore import SeqScoreEmul


class EnsSampleEmul(SampleExclEmul, SeqScoreEmul):
    """the emulated ops of members that search, score and sample, singly and as an ensemble, plus `sample_ens`"""

    def sample_ens(self, logits_list, weights, mode, comb, ids_out, logp, lens, t, end_id, temperature=1.0, seed=0, site_sample=0, row0=0,
                   top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, hist=None, kept=None, excl_shared=None, excl_clip=None,
                   rows_per_clip=1):
        assert len(logits_list) == len(weights) and mode in (0, 1)
        rows, V = logits_list[0].shape
        assert comb.shape == (rows, V) and comb.dtype == torch.float32
        comb.copy_(combined_logp(logits_list, weights, mode).float())
        # the step writes no embedding: the composed emulator's goes nowhere and is kept out of a recording of the ops launched
        E, out = torch.zeros(V, 1), torch.zeros(rows, 1)
        state = object.__getattribute__(self, '__dict__')
        rec = state.pop('recording', None)
        try:
            SampleExclEmul.sample_excl_embed(self, comb, E, ids_out, out, logp, lens, t, end_id, temperature, 0.0, seed, 0, site_sample,
                                             row0, top_k, top_p, min_len, no_repeat_ngram, hist, kept, excl_shared, excl_clip,
                                             rows_per_clip)
        finally:
            if rec is not None:
                state['recording'] = rec

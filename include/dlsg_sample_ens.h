/* dlsg_sample_ens.h -- an entry point of libdlsg_hip.so beside the versioned C ABI of dlsg.h: the sampled word step of an ensemble.
 *
 * dlsg.h is the ABI DLSG_ABI_VERSION counts and its list of entry points is closed at that version; what is added beside it
 * stands in a header of its own, in the same subset of C, and dlsg_amd/abi.py reads it into `abi.extensions` the way it reads dlsg.h
 * into `abi.functions` -- the binding is derived from this text, not mirrored.  The conventions are dlsg.h's: device pointers owned by
 * the caller, nothing allocated, asynchronous on `stream`, 0 or a negative DLSG_E* code.  DLSG_ENS_MAX, DLSG_SAMPLE_FILTER_MAXV,
 * DLSG_EXCL_SHARED, DLSG_EXCL_CLIP and DLSG_PHRASE_MAX are that header's.  See INTEGRATION.md.
 */
#ifndef DLSG_SAMPLE_ENS_H
#define DLSG_SAMPLE_ENS_H
#include "dlsg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A sampled word step of an ENSEMBLE: one word per row drawn from the members' combined distribution.  logits, ld, w (normalised
 * to sum 1), logw = log(w), M, mode: HOST arrays of M entries and the rule, exactly as dlsg_beam_select_ens takes them (read during
 * the call, passed to the kernel by value: a captured launch keeps them); row r of member m is logits[m] + r * ld[m], V floats.  One
 * launch, one workgroup of 256 per row, two phases:
 *   A. comb[r, j] = c_j, the combined value of class j, for all V classes of the row, in the float32 operations and order of
 *      dlsg_beam_select_ens as dlsg_seq_logprob states them: per member lse_m (one wave: strided maximum, wave maximum, strided
 *      exponential sum, wave sum, logf(sum) + max), then mode 0 or mode 1 over the members in member order; M == 1: x - lse.  A
 *      member row that is all -inf or holds a NaN has lse_m = NaN and gives what dlsg_seq_logprob documents for tok_lp: NaN with
 *      M == 1 and in mode 1; in mode 0 NaN where another member gives the class a value above -inf, -inf where none does.
 *      comb (rows, V) float32, dense, is the caller's workspace AND AN OUTPUT: on return comb[r] holds row r's combined values.
 *   B. dlsg_sample_excl_embed's draw on comb[r] as its logits, without the embedding (the members embed the word themselves):
 *      z = c * (1 / temperature); the bans of min_len, no_repeat_ngram and the two exclusion tables; top_k, then top_p; the Gumbel-max
 *      draw with the noise keyed (seed (+ *seed_ptr), site_sample, (row0 + r) * V + j); ids_out, logp, lens and kept as that call
 *      writes them.  The launch returns the bits of dlsg_sample_excl_embed (with the tables empty: dlsg_sample_filter_embed; with
 *      every control off: dlsg_sample_embed) on comb with the same arguments.  One kind of row apart: with every control off a row
 *      that holds no value above -inf but some -inf gives word 0 and kept 0 here, as in the filtered steps, where
 *      dlsg_sample_embed's tie rule names the row's first -inf word.
 * So the temperature tempers the ENSEMBLE's distribution: a word is drawn with probability proportional to exp(c / temperature)
 * over the kept words (M == 1: softmax(x / temperature)), logp is its log-probability under that renormalised distribution, and
 * temperature 0 is the first maximum of c over the words that are not banned.  hist, hist_stride, kept, the tables and
 * rows_per_clip: as in dlsg_sample_excl_embed.  No atomics, fixed-order reductions: two launches, or a launch and a graph replay,
 * give equal bits.  EINVAL and no launch for M outside 1..DLSG_ENS_MAX, mode outside {0, 1}, a NULL member, V < 1, temperature < 0,
 * t outside 0..63 (a caption of more than 64 words), V > DLSG_SAMPLE_FILTER_MAXV with a control on (top_k > 0, top_p < 1, min_len > 0,
 * no_repeat_ngram > 0 or an entry in a table: the threshold searches hold the row in LDS), and for what dlsg_sample_excl_embed
 * refuses of its controls, tables and rows.  rows == 0 launches nothing. */
int dlsg_sample_ens(const float* const* logits, const int64_t* ld, const float* w, const float* logw, int M, int mode, int V,
                    float temperature, float* comb, int64_t* ids_out, float* logp, int64_t* lens, int t, int64_t end_id, int rows,
                    uint64_t seed, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p, int min_len,
                    int no_repeat_ngram, const int64_t* hist, int64_t hist_stride, int32_t* kept, const int64_t* excl_shared, int NS,
                    const int64_t* excl_clip, int NC, int P, int rows_per_clip, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* addons/dlsg_risk.h -- entry points of libdlsg_hip.so beside the versioned C ABI of dlsg.h: the minimum-risk loss over a candidate list.
 *
 * dlsg.h is the ABI DLSG_ABI_VERSION counts, and its list of entry points is closed at that version.  Every later entry point stands in a
 * header under include/addons/, in the same subset of C and holding prototypes only; dlsg_amd/abi.py reads the headers of that directory in
 * sorted order into `abi.addons`, and hip.load_library binds them like dlsg.h's.  The conventions are dlsg.h's: device pointers owned by the
 * caller, nothing allocated, asynchronous on `stream`, 0 or a negative DLSG_E* code.  See INTEGRATION.md.
 *
 * Minimum-risk training (Shen et al. 2016; the sequence-level risk of Edunov et al. 2018).  Clip b has n candidate captions, caption rows
 * b*n .. b*n+n-1 of `rows` = B*n; candidate i has words targets[bi, t], a length len = min(lens[bi], L) counting its <end>, a reward
 * rewards[bi] and a flag valid[bi].  With the logits of one teacher-forced pass over all rows,
 *     s_bi = sum_{t < len} log softmax(logits[t, bi])[targets[bi, t]]       token terms float32, summed over t ascending in float64
 *     a_bi = alpha / len^length_penalty
 *     Q_bi = v_bi exp(a_bi s_bi) / sum_j v_bj exp(a_bj s_bj)                float64, the clip's maximum exponent subtracted
 *     R_b  = sum_i Q_bi rewards[bi],     loss = -(1/B) sum_b R_b
 *     dlogits[t, bi, j] = c_bi (softmax_j - [j == target]) for t < len, else 0,     c_bi = a_bi Q_bi (rewards[bi] - R_b) / B
 * the model renormalised over the list and the gradient of the negative expected reward: dlsg_ce_ragged_weighted's arithmetic with the
 * weight c_bi and no 1 / ntot.  A candidate is COUNTED (v = 1) when its flag is set (valid NULL: every flag set), len >= 1 and s > -inf
 * or NaN; one that is not has Q = 0 and a zero gradient whatever its words, and its reward is not read into any sum.  A clip without a
 * counted candidate has R_b = 0 and a zero gradient.  A target outside [0, V) at a position t < len of a counted candidate indexes nothing:
 * lse and tok_lp of that row are NaN, hence s, every Q and R of the clip, the loss, and the gradient rows of the clip's counted candidates
 * (dlsg_ce_ragged's rule); other clips are untouched.  n = 1 or alpha = 0 gives c = 0.  A row whose c is exactly 0 is filled with zeros.
 * Layout: logits, dlogits (rows, L, V) or, time_major, (L, rows, V), dense float32; targets (rows, L) int64; lens (rows,) int64;
 * lse, tok_lp: rows * L floats in the row order of logits.
 * Limits: 1 <= n <= 32 (one lane per candidate), L <= 64, rows % n == 0, V >= 1, rows * L < 2^31: outside them DLSG_EINVAL and no launch.
 * rows * L == 0 launches nothing.  No atomics, fixed-order reductions: two calls, or a call and a graph replay, give equal bits.
 */
#ifndef DLSG_ADDONS_RISK_H
#define DLSG_ADDONS_RISK_H
#include "../dlsg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One workgroup of 256 per (t, row): lse[row] = log sum_j exp(logits[row, j]) and tok_lp[row] = logits[row, target] - lse[row]; both 0
 * where t >= len, both NaN for a target outside [0, V). */
int dlsg_risk_rows(const float* logits, const int64_t* targets, const int64_t* lens, float* lse, float* tok_lp, int rows, int n, int L,
                   int V, int time_major, void* stream);

/* One workgroup of 256 per (t, row) on what dlsg_risk_rows left in lse and tok_lp for the same logits: its first wave rebuilds the clip's
 * s, Q, R_b and c from the clip's n * L token terms, the workgroup then reads the logits row once and writes the gradient row once.  The
 * workgroups of a clip's first row at t = 0 write Q (rows,) and s (rows,) float64 and R (B,) float64.  A second launch of one workgroup
 * then writes stats, 4 float64: {loss, mean reward over the counted candidates, their mean length, mean_b R_b} (the two means 0 without
 * a counted candidate), and loss, 1 float32: (float)stats[0].  rewards (rows,) float64; valid (rows,) bytes (0 / nonzero) or NULL.
 * alpha >= 0 and length_penalty finite, else DLSG_EINVAL. */
int dlsg_risk_grad(const float* logits, const int64_t* targets, const int64_t* lens, const float* lse, const float* tok_lp,
                   const double* rewards, const void* valid, float* dlogits, double* Q, double* s, double* R, float* loss, double* stats,
                   int rows, int n, int L, int V, int time_major, double alpha, double length_penalty, void* stream);

#ifdef __cplusplus
}
#endif
#endif

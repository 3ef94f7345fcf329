// Scoring GIVEN captions (gfx950): dlsg_seq_logprob, the log-probability of every word of a caption under one model or an
// ensemble, the caption's sum and length-normalised score, and optionally each word's rank in its row.  One workgroup per
// caption, one wave per position (SEQ_WAVES = 8 positions at a time): only the logit rows of a caption's live positions are
// read.  A row's log-sum-exp and the members' combination take the float32 operations of the beam steps in their order, so a
// word's value has the bits the searches add to a beam's log-prob; the length and the score are dlsg_beam_finalize's.  No
// atomics, every reduction in a fixed order.  (16 waves per caption measured slower: DESIGN.md section 27.)
#include <math.h>

#include "beam.hpp"

using namespace dlsg;

namespace {

constexpr int SEQ_WAVES = 8;

// the M members' bases, time and row strides and weights: by value in the argument block (a captured launch keeps them)
struct SeqPack {
    const float* x[DLSG_ENS_MAX];
    int64_t ld_t[DLSG_ENS_MAX], ld_r[DLSG_ENS_MAX];
    float w[DLSG_ENS_MAX], logw[DLSG_ENS_MAX];
    int M, mode;
};

// A member row's log-sum-exp and a class's combined value: beam_row_lse and beam_ens_combine (beam.hpp).

// RANK: tok_rank is wanted.  With one member the count rides on the maximum pass over the raw logits (the row is read twice, as
// without it); with several it is a third pass per member over the combined values.
template <bool RANK>
__global__ __launch_bounds__(64 * SEQ_WAVES) void seq_logprob_kernel(const SeqPack e, const int64_t* __restrict__ ids, int64_t ids_ld,
                                                                      const int64_t* __restrict__ lens_in, int L, int V, int64_t end,
                                                                      double alpha, float* __restrict__ tok_lp,
                                                                      int32_t* __restrict__ tok_rank, float* __restrict__ lp,
                                                                      float* __restrict__ scores, int64_t* __restrict__ lens_out) {
    __shared__ float tl_s[BEAM_MAXL];
    __shared__ float lse_s[SEQ_WAVES][DLSG_ENS_MAX];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r = blockIdx.x;
    // every wave holds the caption: lane t word t (no barrier before the rows are read)
    const int64_t myid = lane < L ? ids[r * ids_ld + lane] : end;
    int len;
    if (lens_in) {
        const int64_t l = lens_in[r];
        len = l < 0 ? 0 : l > L ? L : (int)l;
    } else {
        const unsigned long long m = __ballot(lane < L && myid == end);
        len = m ? __ffsll((long long)m) : L;
    }
    for (int t = w; t < len; t += SEQ_WAVES) {
        const int64_t tgt64 = (int64_t)lane_u64((uint64_t)myid, t);
        float val = NAN;
        int cnt = -1;
        if (tgt64 >= 0 && tgt64 < V) {                        // a target outside [0, V) reads nothing: NaN, rank -1
            const int tgt = (int)tgt64;
            if (e.M == 1) {
                const float* x = e.x[0] + t * e.ld_t[0] + r * e.ld_r[0];
                const float xt = x[tgt];
                float lse;
                if constexpr (RANK) {                         // beam_row_lse with the count in its first pass
                    float mx = -INFINITY;
                    cnt = 0;
                    for (int j = lane; j < V; j += 64) {
                        const float v = x[j];
                        mx = fmaxf(mx, v);
                        cnt += beam_better(v, j, xt, tgt);
                    }
                    mx = dlsg::wave_max(mx);
                    float sum = 0.f;
                    for (int j = lane; j < V; j += 64) sum += expf(x[j] - mx);
                    sum = dlsg::wave_sum(sum);
                    lse = logf(sum) + mx;
                } else {
                    lse = beam_row_lse(x, V, lane);
                }
                val = xt - lse;
            } else {
                for (int m = 0; m < e.M; ++m)                 // (not unrolled; every lane reads back its own store)
                    lse_s[w][m] = beam_row_lse(e.x[m] + t * e.ld_t[m] + r * e.ld_r[m], V, lane);
                const float* x[DLSG_ENS_MAX];
                float lse[DLSG_ENS_MAX];
#pragma unroll
                for (int m = 0; m < DLSG_ENS_MAX; ++m) {
                    x[m] = m < e.M ? e.x[m] + t * e.ld_t[m] + r * e.ld_r[m] : nullptr;
                    lse[m] = m < e.M ? lse_s[w][m] : 0.f;
                }
                val = beam_ens_combine(x, lse, e.w, e.logw, e.M, e.mode, tgt);
                if constexpr (RANK) {
                    cnt = 0;
                    for (int j = lane; j < V; j += 64)
                        cnt += j != tgt && beam_better(beam_ens_combine(x, lse, e.w, e.logw, e.M, e.mode, j), j, val, tgt);
                }
            }
            if constexpr (RANK) cnt = wave_sum_xor(cnt);
        }
        if (lane == 0) {
            tl_s[t] = val;
            if (tok_lp) tok_lp[r * L + t] = val;
            if constexpr (RANK) tok_rank[r * L + t] = cnt;
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= len && t < L) {                                  // padding
        if (tok_lp) tok_lp[r * L + t] = 0.f;
        if constexpr (RANK) tok_rank[r * L + t] = -1;
    }
    if (t == 0) {
        float acc = 0.f;                                      // the searches' order: new_lp = word + last_lp
        for (int i = 0; i < len; ++i) acc = tl_s[i] + acc;
        if (lp) lp[r] = acc;
        if (scores) scores[r] = len ? (float)((double)acc / pow((double)len, alpha)) : 0.f;
        if (lens_out) lens_out[r] = len;
    }
}

// A forced prefix behind a history step (dlsg_beam_force_prefix): one workgroup of ONE wave per clip, launched behind the step's
// select launch on its argument block and history buffers.  Lane j holds word j of the clip's prefix row; the clip is forced at
// step t iff words 0 .. t all lie in [0, V) -- otherwise the workgroup returns and the select launch's outputs stand.  A forced
// clip's K output slots are rewritten: the word, parent row b*K, the parent's history with the word at t (beam_write_hist); slot 0
// carries the parent's log-prob plus the word's value -- seq_logprob_kernel's, by the two functions above -- the other slots -inf,
// so that the first free step expands beam 0 alone, as step 0 does.  e.ld_t is not looked at.
__global__ __launch_bounds__(64) void beam_force_prefix_kernel(const dlsg_beam_select_args a, const SeqPack e,
                                                               const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out,
                                                               int L, int t, const int64_t* __restrict__ prefix, int P) {
    __shared__ float lse_s[DLSG_ENS_MAX];
    const int lane = threadIdx.x, K = a.k;
    const int64_t b = blockIdx.x, row = b * K;
    const int64_t id = lane < P ? prefix[b * P + lane] : -1;
    if (__ballot(lane <= t && !(id >= 0 && id < a.V))) return;       // t >= p_b: nothing of this clip is written
    const int wd = (int)lane_u64((uint64_t)id, t);
    float val;
    if (e.M == 1) {
        const float* x = e.x[0] + row * e.ld_r[0];
        val = x[wd] - beam_row_lse(x, a.V, lane);
    } else {
        for (int m = 0; m < e.M; ++m)                         // (not unrolled; every lane reads back its own store)
            lse_s[m] = beam_row_lse(e.x[m] + row * e.ld_r[m], a.V, lane);
        const float* x[DLSG_ENS_MAX];
        float lse[DLSG_ENS_MAX];
#pragma unroll
        for (int m = 0; m < DLSG_ENS_MAX; ++m) {
            x[m] = m < e.M ? e.x[m] + row * e.ld_r[m] : nullptr;
            lse[m] = m < e.M ? lse_s[m] : 0.f;
        }
        val = beam_ens_combine(x, lse, e.w, e.logw, e.M, e.mode, wd);
    }
    val = val + (t == 0 ? 0.f : a.last_lp[row]);              // the searches' order: new_lp = word + last_lp
    for (int c = 0; c < K; ++c) {
        const int64_t o = row + c;
        if (lane == 0) {
            a.pred[o] = wd;
            a.new_lp[o] = c == 0 ? val : -INFINITY;
            a.back[o] = 0;
            a.rows[o] = row;
        }
        beam_write_hist(hist_in, hist_out, o, row, L, t, lane, wd, a.end);
    }
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dlsg_seq_logprob(const float* const* logits, const int64_t* ld_t, const int64_t* ld_r, const float* w, const float* logw,
                                int M, int mode, const int64_t* ids, int64_t ids_ld, const int64_t* lens_in, int R, int L, int V,
                                int64_t end, double alpha, float* tok_lp, int32_t* tok_rank, float* lp, float* scores, int64_t* lens_out,
                                void* stream) {
    if (!logits || !ld_t || !ld_r || !w || !logw || M < 1 || M > DLSG_ENS_MAX || (mode != 0 && mode != 1)) return DLSG_EINVAL;
    if (L < 1 || L > BEAM_MAXL || V < 1 || R < 0 || !(alpha >= 0.0)) return DLSG_EINVAL;     // (NaN fails the comparison)
    SeqPack e = {};
    for (int m = 0; m < M; ++m) {
        if (!logits[m]) return DLSG_EINVAL;
        e.x[m] = logits[m]; e.ld_t[m] = ld_t[m]; e.ld_r[m] = ld_r[m]; e.w[m] = w[m]; e.logw[m] = logw[m];
    }
    e.M = M; e.mode = mode;
    if (R == 0) return DLSG_OK;
    if (!ids || ids_ld < L) return DLSG_EINVAL;
    if (tok_rank)
        hipLaunchKernelGGL(seq_logprob_kernel<true>, dim3(R), dim3(64 * SEQ_WAVES), 0, ST(stream), e, ids, ids_ld, lens_in, L, V, end,
                           alpha, tok_lp, tok_rank, lp, scores, lens_out);
    else
        hipLaunchKernelGGL(seq_logprob_kernel<false>, dim3(R), dim3(64 * SEQ_WAVES), 0, ST(stream), e, ids, ids_ld, lens_in, L, V, end,
                           alpha, tok_lp, tok_rank, lp, scores, lens_out);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_beam_force_prefix(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                                      const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                      const int64_t* prefix, int P, void* stream) {
    if (!a || a->k < 1 || a->k > BEAM_MAXK || a->V < 1 || a->B < 0 || L < 1 || L > BEAM_MAXL || t < 0 || t >= L) return DLSG_EINVAL;
    if (P < 0 || P > L - 1 || (P > 0 && !prefix)) return DLSG_EINVAL;
    if (!logits || !ld || !w || !logw || M < 1 || M > DLSG_ENS_MAX || (mode != 0 && mode != 1)) return DLSG_EINVAL;
    if (!hist_out || (t > 0 && (!hist_in || hist_in == hist_out))) return DLSG_EINVAL;
    SeqPack e = {};
    for (int m = 0; m < M; ++m) {
        if (!logits[m]) return DLSG_EINVAL;
        e.x[m] = logits[m]; e.ld_r[m] = ld[m]; e.w[m] = w[m]; e.logw[m] = logw[m];
    }
    e.M = M; e.mode = mode;
    if (P == 0 || a->B == 0 || t >= P) return DLSG_OK;         // (no clip is forced at a step behind the table's width)
    hipLaunchKernelGGL(beam_force_prefix_kernel, dim3(a->B), dim3(64), 0, ST(stream), *a, e, hist_in, hist_out, L, t, prefix, P);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

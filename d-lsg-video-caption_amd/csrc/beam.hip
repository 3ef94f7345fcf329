// The beam-search step (gfx950): dlsg_beam_select and its variants with a token history, lexical constraints (dynamic beam
// allocation), Gumbel-perturbed selection (stochastic beam search, also under exclusions), an ensemble of members, beam groups and exclusions, and dlsg_beam_finalize.  One workgroup per batch item, one wave per live
// beam (BeamSearch.search, allennlp_beamsearch.py:140-260 with per_node_beam_size == beam_size): log-softmax of the beam's logits
// row, its top-k classes (a finished beam offers <end> at log-prob 0 and nothing else), then the top-k of the k*k summed
// candidates, back-pointers and the row indices that reorder the recurrent state.  Ties resolve to the lower index.  The step kernels are compositions of the
// phases in beam.hpp: a tie rule, the ban rule or the -inf slot rule is written once, there.  Each kernel declares only the LDS
// its phases use.
#include <type_traits>

#include "beam.hpp"

using namespace dlsg;

namespace {

template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_kernel(const dlsg_beam_select_args a) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;                      // step 0: the k rows of a group are identical, use row 0
    if (w < nbeam) {
        const int64_t row = (int64_t)blockIdx.x * K + w;
        const float base = a.first ? 0.f : a.last_lp[row];
        if (!a.first && a.last[row] == a.end) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
        } else {
            float lse, bv[K];
            int bi[K];
            beam_row_topk<K>(a.logits + row * a.ld, a.V, lane, lse, bv, bi);
#pragma unroll
            for (int c = 0; c < K; ++c) bv[c] -= lse;
            beam_offer_live<K>(lane, bv, bi, base, cand_lp + w * K, cand_cls + w * K);
        }
    }
    __syncthreads();
    if (w == 0) beam_flat_merge<K, false>(a, nbeam, lane, cand_lp, cand_cls, nullptr, nullptr, 0, 0);
}

// The step with a token history that travels with the beams, a repeated-n-gram ban and a minimum length.  hist_in / hist_out
// (B*k, L) int64, ping-pong (beam_write_hist).  Each live beam's wave lists the classes it may not choose in LDS (beam_ban_list).
// g = 0 and min_len = 0 give the bits of beam_select_kernel.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_hist_kernel(const dlsg_beam_select_args a, const int64_t* __restrict__ hist_in,
                                                                    int64_t* __restrict__ hist_out, int L, int t, int g, int min_len) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_MAXL + 1];
    __shared__ int nban[K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    beam_row_bans(hist_in, row, L, t, g, min_len, a.end, w < nbeam && !ended, hist, ban, nban);
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
        } else {
            float lse, bv[K];
            int bi[K];
            beam_row_topk<K, true>(a.logits + row * a.ld, a.V, lane, lse, bv, bi, ban[w], nban[w]);
#pragma unroll
            for (int c = 0; c < K; ++c) bv[c] -= lse;
            beam_offer_live<K>(lane, bv, bi, base, cand_lp + w * K, cand_cls + w * K);
        }
    }
    __syncthreads();
    if (w == 0) beam_flat_merge<K, true>(a, nbeam, lane, cand_lp, cand_cls, hist_in, hist_out, L, t);
}

// The step of stochastic beam search (dlsg_beam_select_gumbel): beam_select_hist_kernel's launch, bans and history, but a live
// row offers the K classes with the largest Gumbel keys at their conditioned perturbed values (beam_offer_gumbel) and the clip
// keeps the K largest of those, float64, in that order.  last_lp / new_lp carry the log-prob under the tempered, renormalised
// model, G_in / G_out the perturbed value.  The noise of class j of row r is keyed ((t + 1) * B*K + r) * V + j: with K = 1 the key
// sample_embed_kernel ranks by at row0 = (t + 1) * B.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_gumbel_kernel(const dlsg_beam_select_args a, const int64_t* __restrict__ hist_in,
                                                                      int64_t* __restrict__ hist_out, int L, int t, int g, int min_len,
                                                                      float tau, uint64_t seed, const uint64_t* __restrict__ seed_ptr,
                                                                      uint32_t site_sample, const double* __restrict__ G_in,
                                                                      double* __restrict__ G_out) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ double cand_g[K * K];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_MAXL + 1];
    __shared__ int nban[K];
    if (seed_ptr) seed += *seed_ptr;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    beam_row_bans(hist_in, row, L, t, g, min_len, a.end, w < nbeam && !ended, hist, ban, nban);
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        // the root's perturbed value: Gumbel(0) noise of its own, keyed as class 0 of this row one step before step 0.  (A root
        // pinned to 0 conditions the largest perturbed value of all captions on being 0: the same sample, but a threshold that
        // no longer gives unbiased importance weights.)
        const double T = a.first ? gumbel_noise64(seed, site_sample, (uint64_t)row * (uint64_t)a.V) : G_in[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
            if (lane < K) cand_g[w * K + lane] = lane == 0 ? T : -INFINITY;
        } else {
            const uint64_t key0 = ((uint64_t)(t + 1) * ((uint64_t)a.B * K) + (uint64_t)row) * (uint64_t)a.V;
            beam_offer_gumbel<K>(a.logits + row * a.ld, a.V, lane, 1.f / tau, seed, site_sample, key0, ban[w], nban[w], base, T,
                                 cand_lp + w * K, cand_cls + w * K, cand_g + w * K);
        }
    }
    __syncthreads();
    if (w == 0) beam_flat_merge<K, true, double>(a, nbeam, lane, cand_g, cand_cls, hist_in, hist_out, L, t, cand_lp, G_out);
}

// Lexically constrained beam search (dlsg_beam_select_cons): beam_select_hist_kernel's step with dynamic beam allocation.  Phase 0
// stages the clip's C * W set entries in LDS (an id outside [0, V) as -1).  Phase 1, wave w for row w: the constraints the row has
// met, from its history (beam_row_met); the ban list with `end` added while a constraint is unmet (beam_ban_list bans `end` below a
// minimum length: an unmet row's is t + 1); list A as beam_select_hist_kernel offers it, and list B, the best word of every unmet
// constraint (beam_offer_constraints).  Phase 2, wave 0: beam_bank_merge.  C = 0 gives the bits of beam_select_hist_kernel.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_cons_kernel(const dlsg_beam_select_args a, const int64_t* __restrict__ hist_in,
                                                                    int64_t* __restrict__ hist_out, int L, int t, int g, int min_len,
                                                                    const int64_t* __restrict__ cons, int C, int W,
                                                                    int32_t* __restrict__ met_out) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ float cons_lp[K * DLSG_CONS_MAX];
    __shared__ int cons_cls[K * DLSG_CONS_MAX];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_MAXL + 1];
    __shared__ int nban[K];
    __shared__ int cons_s[CONS_SLOTS];
    __shared__ unsigned met_s[K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)threadIdx.x < C * W) {
        const int64_t id = cons[(int64_t)blockIdx.x * (C * W) + threadIdx.x];
        cons_s[threadIdx.x] = id >= 0 && id < a.V ? (int)id : -1;
    }
    __syncthreads();
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    const unsigned met = beam_row_met(hist_in, row, L, t, cons_s, C, W);
    const unsigned unmet = beam_cons_present(cons_s, C, W) & ~met;
    if (lane == 0) met_s[w] = met;
    beam_row_bans(hist_in, row, L, t, g, unmet ? t + 1 : min_len, a.end, w < nbeam && !ended, hist, ban, nban);
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
            if (lane < C) { cons_lp[w * C + lane] = -INFINITY; cons_cls[w * C + lane] = 0; }
        } else {
            float lse, bv[K];
            int bi[K];
            beam_row_topk<K, true>(a.logits + row * a.ld, a.V, lane, lse, bv, bi, ban[w], nban[w]);
            beam_offer_constraints<K>(a.logits + row * a.ld, lane, cons_s, C, W, unmet, ban[w], nban[w], bi, lse, base, cons_lp + w * C,
                                      cons_cls + w * C);
#pragma unroll
            for (int c = 0; c < K; ++c) bv[c] -= lse;
            beam_offer_live<K>(lane, bv, bi, base, cand_lp + w * K, cand_cls + w * K);
        }
    }
    __syncthreads();
    if (w == 0)
        beam_bank_merge<K>(a, nbeam, lane, cand_lp, cand_cls, cons_lp, cons_cls, met_s, cons_s, C, W, hist_in, hist_out, L, t, met_out);
}

// Constrained beam search with multi-word phrases (dlsg_beam_select_phrases): beam_select_cons_kernel's step, a constraint being a
// set of alternative phrases.  Phase 0 stages the clip's C * W alternatives in LDS, cut to their valid leading run
// (beam_stage_phrases).  Phase 1, wave w for row w: the row's history into LDS, whatever g is; from it the constraints met, the
// border masks of all alternatives -- kept in LDS for the merge -- and the row's progress (beam_row_phrases); the ban list with
// `end` added while a constraint is unmet; list A, and list B, the next word of the most advanced phrase of every unmet constraint
// (beam_offer_phrases).  Phase 2, wave 0: beam_phrase_merge over the banks (constraints met, progress), which it works out per
// candidate from the parent's masks and the class.  P = 1 gives the bits of beam_select_cons_kernel, C = 0 those of
// beam_select_hist_kernel.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_phrases_kernel(const dlsg_beam_select_args a, const int64_t* __restrict__ hist_in,
                                                                       int64_t* __restrict__ hist_out, int L, int t, int g, int min_len,
                                                                       const int64_t* __restrict__ phr, int C, int W, int P,
                                                                       int32_t* __restrict__ met_out, int32_t* __restrict__ bank_out) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ float cons_lp[K * DLSG_CONS_MAX];
    __shared__ int cons_cls[K * DLSG_CONS_MAX];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_MAXL + 1];
    __shared__ int nban[K];
    __shared__ int phr_s[PHRASE_SLOTS];
    __shared__ int n_s[CONS_SLOTS];
    __shared__ unsigned char border_s[K][CONS_SLOTS];
    __shared__ unsigned met_s[K];
    __shared__ int q_s[K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    beam_stage_phrases(phr + (int64_t)blockIdx.x * (C * W * P), C * W, P, a.V, phr_s, n_s);
    hist[w][lane] = lane < t ? (int)hist_in[row * L + lane] : -1;
    __syncthreads();
    unsigned present, border;
    int q;
    const unsigned met = beam_row_phrases(hist[w], t, phr_s, n_s, C, W, P, border_s[w], present, q, border);
    const unsigned unmet = present & ~met;
    if (lane == 0) { met_s[w] = met; q_s[w] = q; }
    if (w < nbeam && !ended) beam_ban_list(hist[w], t, g, unmet ? t + 1 : min_len, a.end, ban[w], &nban[w]);
    __syncthreads();
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
            if (lane < C) { cons_lp[w * C + lane] = -INFINITY; cons_cls[w * C + lane] = 0; }
        } else {
            float lse, bv[K];
            int bi[K];
            beam_row_topk<K, true>(a.logits + row * a.ld, a.V, lane, lse, bv, bi, ban[w], nban[w]);
            beam_offer_phrases<K>(a.logits + row * a.ld, lane, phr_s, n_s, C, W, P, unmet, border, ban[w], nban[w], bi, lse, base,
                                  cons_lp + w * C, cons_cls + w * C);
#pragma unroll
            for (int c = 0; c < K; ++c) bv[c] -= lse;
            beam_offer_live<K>(lane, bv, bi, base, cand_lp + w * K, cand_cls + w * K);
        }
    }
    __syncthreads();
    if (w == 0)
        beam_phrase_merge<K>(a, nbeam, lane, cand_lp, cand_cls, cons_lp, cons_cls, met_s, q_s, border_s, phr_s, n_s, C, W, P, hist_in,
                             hist_out, L, t, met_out, bank_out);
}

// Phase 1 of the ensemble step and of the group step, wave w for row w: beam_select_hist_kernel's, but a live beam's candidates
// are the K best combined values of the members' rows (beam_ens_row_topk).  Every row's K (c + last_lp, class) end up in LDS.
template <int K>
__device__ __forceinline__ void beam_ens_candidates(const dlsg_beam_select_args& a, const EnsPack& e, const int64_t* __restrict__ hist_in,
                                                    int L, int t, int g, int min_len, int (&hist)[K][BEAM_MAXL], int (&ban)[K][BEAM_MAXL + 1],
                                                    int (&nban)[K], float (*lse_s)[DLSG_ENS_MAX], float* cand_lp, int* cand_cls) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    beam_row_bans(hist_in, row, L, t, g, min_len, a.end, w < nbeam && !ended, hist, ban, nban);
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
        } else {
            float bv[K];
            int bi[K];
            beam_ens_row_topk<K>(e, row, a.V, lane, lse_s[w], ban[w], nban[w], bv, bi);
            beam_offer_live<K>(lane, bv, bi, base, cand_lp + w * K, cand_cls + w * K);
        }
    }
    __syncthreads();
}

// The step of an ensemble (dlsg_beam_select_ens).  With one member of weight 1 the launch returns what beam_select_hist_kernel
// returns.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_ens_kernel(const dlsg_beam_select_args a, const EnsPack e,
                                                                   const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out,
                                                                   int L, int t, int g, int min_len) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_MAXL + 1];
    __shared__ int nban[K];
    __shared__ float lse_s[K][DLSG_ENS_MAX];
    beam_ens_candidates<K>(a, e, hist_in, L, t, g, min_len, hist, ban, nban, lse_s, cand_lp, cand_cls);
    if (threadIdx.x < 64) beam_flat_merge<K, true>(a, a.first ? 1 : K, threadIdx.x, cand_lp, cand_cls, hist_in, hist_out, L, t);
}

// Diverse (group) beam search (dlsg_beam_select_groups): the K beams of a clip are G groups of KG = K / G consecutive rows.
// Phase 1 is beam_select_ens_kernel's, wave w for row w: every row's K best (c + last_lp, class) in LDS.  Phase 2, wave 0: the
// groups in order; lane i < KG * K holds candidate i of the group (row within the group, then rank; step 0: the K entries of the
// clip's one list, parent = the group's first row), key = lp, minus diversity * cnt[class] where the parent is live and cnt, the
// number of picks of that class by earlier groups at this step from live parents, is not 0 (diversity = +inf: the key is -inf).
// KG rounds of wave_argmax over (key, lane); a -inf key is no candidate, a slot left over takes candidate slot q of the group at
// log-prob -inf and is not counted.  new_lp is lp, not the key.  The picks so far (at most K) are wave-uniform registers.
// G = 1: no class is ever counted, so every key is its lp and the launch chooses what beam_select_ens_kernel chooses.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_groups_kernel(const dlsg_beam_select_args a, const EnsPack e,
                                                                      const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out,
                                                                      int L, int t, int g, int min_len, int G, float diversity) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_MAXL + 1];
    __shared__ int nban[K];
    __shared__ float lse_s[K][DLSG_ENS_MAX];
    beam_ens_candidates<K>(a, e, hist_in, L, t, g, min_len, hist, ban, nban, lse_s, cand_lp, cand_cls);
    const int b = blockIdx.x, k = K, lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const int kg = k / G;
        const int n = a.first ? k : kg * k;                   // candidates of one group (<= 64: one per lane)
        int mypick = -1;                                      // lane s: the s-th class counted at this step
        int npicked = 0, n_end = 0;                           // (wave-uniform; at most k)
        for (int gr = 0; gr < G; ++gr) {
            const int first_row = gr * kg;                    // the group's first row within the clip
            const bool have = lane < n;
            const int ci = !have ? 0 : a.first ? lane : first_row * k + lane;      // this lane's slot in cand_lp / cand_cls
            const int par = !have || a.first ? first_row : first_row + lane / k;   // and its parent within the clip
            const int mycls = cand_cls[ci];
            int cnt = 0;
            for (int q = 0; q < npicked; ++q) cnt += __builtin_amdgcn_readlane(mypick, q) == mycls;
            float key = have ? cand_lp[ci] : -INFINITY;
            if (cnt > 0 && (a.first || a.last[(int64_t)b * k + par] != a.end))
                key = diversity == INFINITY ? -INFINITY : key - __fmul_rn(diversity, (float)cnt);
            int idx = key == -INFINITY ? 0x7fffffff : lane;   // a -inf key is no candidate
            for (int q = 0; q < kg; ++q) {                    // (keys are taken once per group: a pick counts from the next group on)
                float bv = key;
                int bi = idx;
                wave_argmax(bv, bi);
                if (lane == bi) key = -INFINITY, idx = 0x7fffffff;
                const bool fill = bi == 0x7fffffff;            // fewer than kg candidates: slot q of the group, log-prob -inf
                if (fill) bi = q;
                const int sl = a.first ? bi : first_row * k + bi;
                const int pb = a.first ? first_row : first_row + bi / k;
                const int cls = cand_cls[sl];
                const int64_t o = (int64_t)b * k + first_row + q;
                if (lane == 0) {
                    a.pred[o] = cls;
                    a.new_lp[o] = fill ? -INFINITY : cand_lp[sl];
                    a.back[o] = pb;
                    a.rows[o] = (int64_t)b * k + pb;
                }
                beam_write_hist(hist_in, hist_out, o, (int64_t)b * k + pb, L, t, lane, cls, a.end);
                n_end += cls == a.end;
                if (!fill && (a.first || a.last[(int64_t)b * k + pb] != a.end)) {
                    if (lane == npicked) mypick = cls;
                    ++npicked;
                }
            }
        }
        if (lane == 0 && a.ended_count) atomicAdd(a.ended_count, n_end);
    }
}

// The step with exclusions (dlsg_beam_select_excl): beam_select_ens_kernel's step whose live rows may not choose the last word of
// an excluded entry behind the entry's other words.  Phase 0 stages the NS shared entries and the clip's NC own in LDS
// (beam_stage_exclusions); phase 1, wave w for row w: the ban list of beam_select_ens_kernel with the matching entries' last words
// behind it, a longer list sorted by residue so that a lane scans only the classes it can meet (beam_row_bans_excl), then that kernel's
// candidates; phase 2, wave 0: beam_flat_merge.  NS = NC = 0 gives the bits of beam_select_ens_kernel.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_excl_kernel(const dlsg_beam_select_args a, const EnsPack e,
                                                                    const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out,
                                                                    int L, int t, int g, int min_len,
                                                                    const int64_t* __restrict__ excl_shared, int NS,
                                                                    const int64_t* __restrict__ excl_clip, int NC, int P) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_BAN_EXCL];
    __shared__ int sorted[K][BEAM_BAN_EXCL];
    __shared__ int nban[K];
    __shared__ float lse_s[K][DLSG_ENS_MAX];
    __shared__ int ex_s[EXCL_SLOTS * DLSG_PHRASE_MAX];
    __shared__ int exn_s[EXCL_SLOTS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    const int tok = lane < t ? (int)hist_in[row * L + lane] : -1;     // (asked for before the tables: one wait for both)
    beam_stage_exclusions(excl_shared, NS, excl_clip + (int64_t)blockIdx.x * (NC * P), NC, P, a.V, ex_s, exn_s);
    int cnt;                                                  // what this lane scans: list[0 .. cnt)
    const int* list = beam_row_bans_excl(tok, t, g, min_len, a.end, w < nbeam && !ended, ex_s, exn_s, NS + NC, P, hist, ban, nban, sorted,
                                         cnt);
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
        } else {
            float bv[K];
            int bi[K];
            beam_ens_row_topk<K>(e, row, a.V, lane, lse_s[w], list, cnt, bv, bi);
            beam_offer_live<K>(lane, bv, bi, base, cand_lp + w * K, cand_cls + w * K);
        }
    }
    __syncthreads();
    if (w == 0) beam_flat_merge<K, true>(a, nbeam, lane, cand_lp, cand_cls, hist_in, hist_out, L, t);
}

// The stochastic step under exclusions (dlsg_beam_select_gumbel_excl): beam_select_gumbel_kernel with phase 0 and the ban list of
// beam_select_excl_kernel.  beam_offer_gumbel looks every class up in the list, since its log-sum-exp leaves the banned classes out,
// so the list by residue (beam_row_bans_excl) saves it more than it saves the beam step.  The keys, the conditioning in float64, the
// merge and G_in / G_out are beam_select_gumbel_kernel's; NS = NC = 0 gives its bits.
template <int K>
__global__ __launch_bounds__(64 * K) void beam_select_gumbel_excl_kernel(const dlsg_beam_select_args a, const int64_t* __restrict__ hist_in,
                                                                           int64_t* __restrict__ hist_out, int L, int t, int g, int min_len,
                                                                           float tau, uint64_t seed, const uint64_t* __restrict__ seed_ptr,
                                                                           uint32_t site_sample, const double* __restrict__ G_in,
                                                                           double* __restrict__ G_out, const int64_t* __restrict__ excl_shared,
                                                                           int NS, const int64_t* __restrict__ excl_clip, int NC, int P) {
    __shared__ float cand_lp[K * K];
    __shared__ int cand_cls[K * K];
    __shared__ double cand_g[K * K];
    __shared__ int hist[K][BEAM_MAXL];
    __shared__ int ban[K][BEAM_BAN_EXCL];
    __shared__ int sorted[K][BEAM_BAN_EXCL];
    __shared__ int nban[K];
    __shared__ int ex_s[EXCL_SLOTS * DLSG_PHRASE_MAX];
    __shared__ int exn_s[EXCL_SLOTS];
    if (seed_ptr) seed += *seed_ptr;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nbeam = a.first ? 1 : K;
    const int64_t row = (int64_t)blockIdx.x * K + w;
    const bool ended = !a.first && a.last[row] == a.end;
    const int tok = lane < t ? (int)hist_in[row * L + lane] : -1;     // (asked for before the tables: one wait for both)
    beam_stage_exclusions(excl_shared, NS, excl_clip + (int64_t)blockIdx.x * (NC * P), NC, P, a.V, ex_s, exn_s);
    int cnt;                                                  // what this lane scans: list[0 .. cnt)
    const int* list = beam_row_bans_excl(tok, t, g, min_len, a.end, w < nbeam && !ended, ex_s, exn_s, NS + NC, P, hist, ban, nban, sorted,
                                         cnt);
    if (w < nbeam) {
        const float base = a.first ? 0.f : a.last_lp[row];
        const double T = a.first ? gumbel_noise64(seed, site_sample, (uint64_t)row * (uint64_t)a.V) : G_in[row];
        if (ended) {
            beam_offer_ended<K>(a, lane, base, cand_lp + w * K, cand_cls + w * K);
            if (lane < K) cand_g[w * K + lane] = lane == 0 ? T : -INFINITY;
        } else {
            const uint64_t key0 = ((uint64_t)(t + 1) * ((uint64_t)a.B * K) + (uint64_t)row) * (uint64_t)a.V;
            beam_offer_gumbel<K>(a.logits + row * a.ld, a.V, lane, 1.f / tau, seed, site_sample, key0, list, cnt, base, T,
                                 cand_lp + w * K, cand_cls + w * K, cand_g + w * K);
        }
    }
    __syncthreads();
    if (w == 0) beam_flat_merge<K, true, double>(a, nbeam, lane, cand_g, cand_cls, hist_in, hist_out, L, t, cand_lp, G_out);
}

// The n best of each clip's k finished beams, by score = lp / len^alpha (double, stored as float), descending, ties to the lower
// beam: one wave per clip.  len = tokens up to and including the first `end` of the beam's history row, L without one.
__global__ __launch_bounds__(64) void beam_finalize_kernel(const int64_t* __restrict__ hist, const float* __restrict__ lp, int k, int L,
                                                           int64_t end, double alpha, int n, int64_t* __restrict__ ids,
                                                           float* __restrict__ scores, int64_t* __restrict__ lens) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float sc[BEAM_MAXK];
    int len[BEAM_MAXK];
    for (int c = 0; c < k; ++c) {
        const int64_t row = (int64_t)b * k + c;
        const unsigned long long m = __ballot(lane < L && hist[row * L + lane] == end);
        len[c] = m ? __ffsll((long long)m) : L;
        sc[c] = (float)((double)lp[row] / pow((double)len[c], alpha));
    }
    for (int c = 0; c < k; ++c) {
        int rank = 0;
        for (int d = 0; d < k; ++d) rank += d != c && beam_better(sc[d], d, sc[c], c);
        if (rank >= n) continue;
        const int64_t o = (int64_t)b * n + rank;
        if (lane < L) ids[o * L + lane] = hist[((int64_t)b * k + c) * L + lane];
        if (lane == 0) { scores[o] = sc[c]; lens[o] = len[c]; }
    }
}

// ---- what the launchers share: the three argument checks and the dispatch over K
bool beam_args_ok(const dlsg_beam_select_args* a) { return a && a->k >= 1 && a->k <= BEAM_MAXK && a->V >= a->k; }
// what every history launcher checks first: the argument block and the history step
bool beam_hist_ok(const dlsg_beam_select_args* a, const int64_t* hist_in, const int64_t* hist_out, int L, int t, int g, int min_len) {
    if (!beam_args_ok(a) || !hist_out || L < 1 || L > BEAM_MAXL || t < 0 || t >= L || g < 0 || min_len < 0) return false;
    return (a->first != 0) == (t == 0) && (t == 0 || (hist_in && hist_in != hist_out));
}
// what the two stochastic steps ask beyond the history step
bool beam_gumbel_ok(float temperature, const double* G_in, const double* G_out, int t) {
    return temperature > 0.f && G_out && (t == 0 || (G_in && G_in != G_out));     // (NaN fails the comparison)
}
// launch(integral_constant<int, k>) for k = 1 .. BEAM_MAXK (checked by beam_args_ok)
template <typename F>
void beam_for_k(int k, F&& launch) {
    switch (k) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 5: launch(std::integral_constant<int, 5>{}); break;
        case 6: launch(std::integral_constant<int, 6>{}); break;
        case 7: launch(std::integral_constant<int, 7>{}); break;
        default: launch(std::integral_constant<int, 8>{}); break;
    }
}
// KERNEL<k> on B workgroups of k waves
#define BEAM_LAUNCH(KERNEL, ...)                                                                                        \
    beam_for_k(a->k, [&](auto kk) {                                                                                     \
        hipLaunchKernelGGL(KERNEL<decltype(kk)::value>, dim3(a->B), dim3(64 * decltype(kk)::value), 0, ST(stream), *a, ##__VA_ARGS__); \
    })
#define ST(s) reinterpret_cast<hipStream_t>(s)

}  // namespace

extern "C" int dlsg_beam_select(const dlsg_beam_select_args* a, void* stream) {
    if (!beam_args_ok(a)) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    BEAM_LAUNCH(beam_select_kernel);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_hist(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                     int no_repeat_ngram, int min_len, void* stream) {
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len)) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    BEAM_LAUNCH(beam_select_hist_kernel, hist_in, hist_out, L, t, no_repeat_ngram, min_len);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_cons(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                     int no_repeat_ngram, int min_len, const int64_t* cons, int C, int W, int32_t* met_out, void* stream) {
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len)) return DLSG_EINVAL;
    if (C < 0 || C > DLSG_CONS_MAX || (C > 0 && (W < 1 || W > DLSG_CONS_ALT || !cons))) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    if (!cons) C = 0;
    if (C == 0) W = 1;
    BEAM_LAUNCH(beam_select_cons_kernel, hist_in, hist_out, L, t, no_repeat_ngram, min_len, cons, C, W, met_out);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_phrases(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                        int no_repeat_ngram, int min_len, const int64_t* phr, int C, int W, int P, int32_t* met_out,
                                        int32_t* bank_out, void* stream) {
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len)) return DLSG_EINVAL;
    if (C < 0 || C > DLSG_CONS_MAX || (C > 0 && (W < 1 || W > DLSG_CONS_ALT || P < 1 || P > DLSG_PHRASE_MAX || !phr))) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    if (!phr) C = 0;
    if (C == 0) W = P = 1;
    BEAM_LAUNCH(beam_select_phrases_kernel, hist_in, hist_out, L, t, no_repeat_ngram, min_len, phr, C, W, P, met_out, bank_out);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_gumbel(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                       int no_repeat_ngram, int min_len, float temperature, uint64_t seed, const uint64_t* seed_ptr,
                                       uint32_t site_sample, const double* G_in, double* G_out, void* stream) {
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len)) return DLSG_EINVAL;
    if (!beam_gumbel_ok(temperature, G_in, G_out, t)) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    BEAM_LAUNCH(beam_select_gumbel_kernel, hist_in, hist_out, L, t, no_repeat_ngram, min_len, temperature, seed, seed_ptr, site_sample,
                G_in, G_out);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_ens(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                                    const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                    int no_repeat_ngram, int min_len, void* stream) {
    EnsPack e;
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len) ||
        !beam_ens_pack(logits, ld, w, logw, M, mode, e))
        return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    BEAM_LAUNCH(beam_select_ens_kernel, e, hist_in, hist_out, L, t, no_repeat_ngram, min_len);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_groups(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                                       const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                       int no_repeat_ngram, int min_len, int groups, float diversity, void* stream) {
    EnsPack e;
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len) ||
        !beam_ens_pack(logits, ld, w, logw, M, mode, e))
        return DLSG_EINVAL;
    if (groups < 1 || a->k % groups != 0 || !(diversity >= 0.f)) return DLSG_EINVAL;     // (NaN fails the comparison)
    if (a->B == 0) return DLSG_OK;
    BEAM_LAUNCH(beam_select_groups_kernel, e, hist_in, hist_out, L, t, no_repeat_ngram, min_len, groups, diversity);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_excl(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                                     const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                     int no_repeat_ngram, int min_len, const int64_t* excl_shared, int NS, const int64_t* excl_clip,
                                     int NC, int P, void* stream) {
    EnsPack e;
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len) ||
        !beam_ens_pack(logits, ld, w, logw, M, mode, e))
        return DLSG_EINVAL;
    if (!beam_excl_ok(excl_shared, NS, excl_clip, NC, P)) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    if (NS + NC == 0) P = 1;
    BEAM_LAUNCH(beam_select_excl_kernel, e, hist_in, hist_out, L, t, no_repeat_ngram, min_len, excl_shared, NS, excl_clip, NC, P);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_select_gumbel_excl(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                            int no_repeat_ngram, int min_len, float temperature, uint64_t seed, const uint64_t* seed_ptr,
                                            uint32_t site_sample, const double* G_in, double* G_out, const int64_t* excl_shared, int NS,
                                            const int64_t* excl_clip, int NC, int P, void* stream) {
    if (!beam_hist_ok(a, hist_in, hist_out, L, t, no_repeat_ngram, min_len)) return DLSG_EINVAL;
    if (!beam_gumbel_ok(temperature, G_in, G_out, t)) return DLSG_EINVAL;
    if (!beam_excl_ok(excl_shared, NS, excl_clip, NC, P)) return DLSG_EINVAL;
    if (a->B == 0) return DLSG_OK;
    if (NS + NC == 0) P = 1;
    BEAM_LAUNCH(beam_select_gumbel_excl_kernel, hist_in, hist_out, L, t, no_repeat_ngram, min_len, temperature, seed, seed_ptr,
                site_sample, G_in, G_out, excl_shared, NS, excl_clip, NC, P);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_beam_finalize(const int64_t* hist, const float* lp, int B, int k, int L, int64_t end, double alpha, int n,
                                  int64_t* ids, float* scores, int64_t* lens, void* stream) {
    if (!hist || !lp || !ids || !scores || !lens || B < 0 || k < 1 || k > BEAM_MAXK || L < 1 || L > BEAM_MAXL || n < 1 || n > k)
        return DLSG_EINVAL;
    if (B == 0) return DLSG_OK;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(B), dim3(64), 0, ST(stream), hist, lp, k, L, end, alpha, n, ids, scores, lens);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

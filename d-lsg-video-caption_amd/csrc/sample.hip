// The kernels that choose the next word from a row of logits and write its embedding (gfx950), one workgroup of 256 per row, each
// a composition of the phases of wordpick.hpp: dlsg_argmax (greedy), dlsg_select_embed (scheduled sampling: the caption's word or
// the greedy one), dlsg_sample_embed (Gumbel-max draw with its log-prob) and dlsg_sample_filter_embed, the draw behind a
// repeated-n-gram ban, a minimum length, top-k and nucleus (top-p) truncation, and dlsg_sample_excl_embed, that step's body once more
// with the bans of the exclusion tables (beam.hpp) in the row's list, and dlsg_sample_ens, which combines an ensemble's M logit rows
// into one row of values and runs that body on it without the embedding.  The filtered step holds the row's tempered logits in
// LDS and finds the two thresholds without sorting: a descent over an order-preserving uint32 image of the float, two bits per
// round, each round one pass over the candidates still undecided and one fixed-order block reduction (an integer count for top-k,
// a float mass for top-p).  No atomics anywhere: two launches, or an eager launch and a graph replay, give the same bits.
#include <math.h>
#include <mutex>

#include "beam.hpp"
#include "common.hpp"
#include "dlsg.h"
#include "dlsg_sample_ens.h"
#include "wordpick.hpp"

using namespace dlsg;

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_MAXL = BEAM_MAXL;      // history positions: lane i of wave 0 holds word i

// u < v as floats  <=>  ord_key(u) < ord_key(v) as unsigned, for everything but NaN (staging turns NaN into -inf, -0 into +0)
__device__ __forceinline__ uint32_t ord_key(float z) {
    const uint32_t u = __float_as_uint(z);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

// Block sums of NF floats and NI ints at once with ONE barrier: the waves' partial sums go to red[par], the next call uses the
// other half, so a wave may start writing the round after next only after a barrier every reader of this round has passed.
// The four wave sums are added in a fixed order; every thread gets the same bits.
struct Red {
    float f[2][3][4];
    int i[2][4][4];
};
template <int NF, int NI>
__device__ __forceinline__ void block_sum(float (&f)[3], int (&n)[4], Red& red, int& par) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NF; ++q) f[q] = wave_sum_dpp(f[q]);
#pragma unroll
    for (int q = 0; q < NI; ++q) n[q] = wave_sum_i32(n[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NF; ++q) red.f[par][q][w] = f[q];
#pragma unroll
        for (int q = 0; q < NI; ++q) red.i[par][q][w] = n[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NF; ++q) f[q] = (red.f[par][q][0] + red.f[par][q][1]) + (red.f[par][q][2] + red.f[par][q][3]);
#pragma unroll
    for (int q = 0; q < NI; ++q) n[q] = (red.i[par][q][0] + red.i[par][q][1]) + (red.i[par][q][2] + red.i[par][q][3]);
    par ^= 1;
}

// The threshold search.  A thread owns the candidates zs[tid + 256 i], i < cnt (its private list: nobody else touches those
// slots, so it compacts them in place without a barrier).  The answer lies in [T, upper); a round splits that interval in four
// (two bits of the image), every thread counts (MASS: sums exp(z - m) of) its candidates at or above the three inner bounds on
// top of `acc`, what it has already seen above `upper`, one block reduction decides the quarter, and the next round drops the
// candidates that fell out of the interval on either side.  The lists shrink about fourfold per round, so all rounds together
// read little more than the row once.  Ends early when the interval holds no candidate (nothing left to decide), or, counting,
// when a bound has exactly k candidates at or above it (the set is then the top k with every tie at the k-th).
//   counting: the largest T with count{key >= T} >= k, or a smaller bound with the same set {key >= T};
//   MASS:     the same for mass{key >= T} >= target.  The order of the additions is fixed by (V, the row's values): the same
//             bits on every launch.
template <bool MASS>
__device__ __forceinline__ uint32_t descend(float* zs, int& cnt, float m, int k, float target, Red& red, int& par) {
    const int tid = threadIdx.x;
    uint32_t T = 0;
    uint64_t upper = 1ull << 32;
    float accf = 0.f;
    int acci = 0;
    for (int b = 30; b >= 0; b -= 2) {
        const uint32_t c1 = T | (1u << b), c2 = T | (2u << b), c3 = T | (3u << b);
        float f[3] = {0.f, 0.f, 0.f};
        int n[4] = {0, 0, 0, 0};
        int w = 0;
        for (int i = 0; i < cnt; ++i) {
            const float z = zs[tid + SF_THREADS * i];
            const uint32_t key = ord_key(z);
            if (key < T) continue;
            if ((uint64_t)key >= upper) {
                if constexpr (MASS) accf += __expf(z - m);
                else ++acci;
                continue;
            }
            zs[tid + SF_THREADS * w++] = z;                  // (w <= i: a slot already read)
            if constexpr (MASS) {
                const float e = __expf(z - m);
                f[0] += key >= c1 ? e : 0.f; f[1] += key >= c2 ? e : 0.f; f[2] += key >= c3 ? e : 0.f;
            } else {
                n[1] += key >= c1; n[2] += key >= c2; n[3] += key >= c3;
            }
        }
        cnt = w;
        n[0] = w;                                            // candidates inside the interval this round split
        int pick;
        if constexpr (MASS) {
            f[0] += accf; f[1] += accf; f[2] += accf;
            block_sum<3, 1>(f, n, red, par);
            pick = f[2] >= target ? 3 : f[1] >= target ? 2 : f[0] >= target ? 1 : 0;
        } else {
            n[1] += acci; n[2] += acci; n[3] += acci;
            block_sum<0, 4>(f, n, red, par);
            pick = n[3] >= k ? 3 : n[2] >= k ? 2 : n[1] >= k ? 1 : 0;
        }
        T |= (uint32_t)pick << b;
        upper = (uint64_t)T + (1ull << b);
        if (n[0] == 0) break;
        if (!MASS && pick > 0 && n[pick] == k) break;
    }
    return T;
}

// ids[r] = the row's first maximum
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int64_t ld, int64_t* __restrict__ ids,
                                                     int V) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int r = blockIdx.x;
    const int id = first_max_row(logits + (int64_t)r * ld, V, bv, bi);
    if (threadIdx.x == 0) ids[r] = id;
}

// scheduled sampling select + embedding gather: one block per batch row
__global__ __launch_bounds__(256) void select_embed_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                           const int64_t* __restrict__ captions, int L, int t,
                                                           const int32_t* __restrict__ coins, const float* __restrict__ E,
                                                           int64_t* __restrict__ ids_out, float* __restrict__ out,
                                                           int64_t ldo, int W, float p, uint64_t seed, uint32_t site,
                                                           int64_t row0, const uint64_t* seed_ptr, int prefilled) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ int64_t chosen;
    if (prefilled && coins[t] != 0) return;      // teacher-forced step whose word the caller embedded up front: nothing to do
    if (seed_ptr) seed += *seed_ptr;
    const int r = blockIdx.x;
    if (coins[t] != 0) {
        if (threadIdx.x == 0) chosen = captions[(int64_t)r * L + t];
    } else {
        const int id = first_max_row(logits + (int64_t)r * ld, V, bv, bi);
        if (threadIdx.x == 0) chosen = id;
    }
    __syncthreads();
    const int64_t id = chosen;
    if (threadIdx.x == 0) ids_out[r] = id;
    embed_row(E, id, out, ldo, W, r, p, seed, site, row0, blockDim.x);
}

// sampled word step (self-critical training): WordDraw (wordpick.hpp) over the whole row, then the gather of E[id] under the
// word-dropout stream of embed_fwd / select_embed (row row0 + r).  One block of 256 per row.
__global__ __launch_bounds__(256) void sample_embed_kernel(const float* __restrict__ logits, int64_t ld, int V, float tau,
                                                           const float* __restrict__ E, int64_t* __restrict__ ids_out,
                                                           float* __restrict__ out, int64_t ldo, int W, float* __restrict__ logp,
                                                           int64_t* __restrict__ lens, int t, int64_t end_id, float p,
                                                           uint64_t seed, uint32_t site_word, uint32_t site_sample, int64_t row0,
                                                           const uint64_t* seed_ptr) {
    __shared__ float bv[4], bm[4], bs[4];
    __shared__ int bi[4];
    __shared__ int64_t chosen;
    if (seed_ptr) seed += *seed_ptr;
    const int r = blockIdx.x;
    const float* x = logits + (int64_t)r * ld;
    WordDraw d(tau, seed, site_sample, row0 + r, V);
    for (int j = threadIdx.x; j < V; j += blockDim.x) d.step<false>(j, x[j]);
    d.wave();
    const int64_t id = d.block(bv, bi, bm, bs);
    if (threadIdx.x == 0) {
        chosen = id;
        d.commit(id, x, false, r, ids_out, logp, lens, t, end_id);
    }
    __syncthreads();
    embed_row(E, chosen, out, ldo, W, r, p, seed, site_word, row0, blockDim.x);
}

// The exclusion tables of the step under exclusions (dlsg_sample_excl_embed): beam.hpp's two tables; row r reads the own entries of
// clip r / rows_per_clip
struct SampleExcl {
    const int64_t* shared;
    const int64_t* clip;
    int NS, NC, P, rows_per_clip;
};

// The filtered step.  hist: the row's earlier words, time-major: word i of row r at hist[i * hist_stride + r], i < t.
// EXCL: the step under exclusions -- phase 0 stages the two tables in LDS (beam_stage_exclusions), the history row is loaded whenever
// an entry can look at it, and wave 0 puts the last words of the matching entries behind the list of beam_ban_list
// (beam_ban_exclusions); everything behind the list is the one body.  Without EXCL `e` is not looked at.  EMBED: the chosen word's
// embedding row is written behind the draw; without it (dlsg_sample_ens: every member embeds the word itself) E, out, ldo, W, p and
// site_word are not looked at and the step ends with thread 0's commit.
template <bool EXCL, bool EMBED = true>
__device__ __forceinline__ void sample_filter_embed_body(
    const float* __restrict__ logits, int64_t ld, int V, float tau, const float* __restrict__ E, int64_t* __restrict__ ids_out,
    float* __restrict__ out, int64_t ldo, int W, float* __restrict__ logp, int64_t* __restrict__ lens, int t, int64_t end_id, float p,
    uint64_t seed, uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p,
    int min_len, int g, const int64_t* hist, int64_t hist_stride, int32_t* __restrict__ kept, const SampleExcl& e) {
    extern __shared__ float zs[];                            // V floats: the threads' candidate lists (descend)
    __shared__ Red red;
    __shared__ int hs[SF_MAXL], ban[EXCL ? BEAM_BAN_EXCL : SF_MAXL + 1], nban_s;
    __shared__ int ex_s[EXCL ? EXCL_SLOTS * DLSG_PHRASE_MAX : 1], exn_s[EXCL ? EXCL_SLOTS : 1];
    __shared__ float bv[4], bm[4], bs[4];
    __shared__ int bi[4], bn[4];
    __shared__ int64_t chosen;
    if (seed_ptr) seed += *seed_ptr;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* x = logits + (int64_t)r * ld;
    WordDraw d(tau, seed, site_sample, row0 + r, V);
    int par = 0;

    // ---- the classes this row may not choose: the beam search's rule (beam_ban_list, beam.hpp) on the row's own words
    if constexpr (EXCL) {
        const int NE = e.NS + e.NC;
        const bool need = ((g > 0 && t >= g) || (NE > 0 && t >= 1)) && tid < SF_MAXL;
        const int tok = need && tid < t ? (int)hist[(int64_t)tid * hist_stride + r] : -1;   // (asked for before the tables: one wait)
        beam_stage_exclusions(e.shared, e.NS, e.clip + (int64_t)(r / e.rows_per_clip) * (e.NC * e.P), e.NC, e.P, V, ex_s, exn_s);
        if (need) hs[tid] = tok;
        __syncthreads();
        if (w == 0) {
            beam_ban_list(hs, t, g, min_len, (int)end_id, ban, &nban_s);
            beam_ban_exclusions(hs, t, ex_s, exn_s, NE, e.P, ban, &nban_s);
        }
    } else {
        if (g > 0 && t >= g && tid < SF_MAXL) hs[tid] = tid < t ? (int)hist[(int64_t)tid * hist_stride + r] : -1;
        __syncthreads();
        if (w == 0) beam_ban_list(hs, t, g, min_len, (int)end_id, ban, &nban_s);
    }
    __syncthreads();
    const int nban = nban_s;

    // ---- thresholds.  A word is kept iff it is alive (finite, not banned) and ord_key(z) >= T.
    // alive(j, z): z_j = x_j / tau (+ 0: -0 becomes +0, so equal values have equal images), false for NaN, -inf and banned words
    auto alive = [&](int j, float& z) {
        z = x[j] * d.sc + 0.f;
        bool dead = !(z > -INFINITY);
        for (int b = 0; b < nban; ++b) dead |= ban[b] == j;
        return !dead;
    };
    uint32_t T = 0;
    if (d.gumbel && (top_k > 0 || top_p < 1.f)) {
        // stage the alive words as this thread's candidate list; the row's maximum and the number of alive words
        float m = -INFINITY;
        int cnt = 0;
        for (int j = tid; j < V; j += SF_THREADS) {
            float z;
            if (!alive(j, z)) continue;
            zs[tid + SF_THREADS * cnt++] = z;
            m = fmaxf(m, z);
        }
        float f[3] = {0.f, 0.f, 0.f};
        int n[4] = {cnt, 0, 0, 0};
        m = wave_max(m);
        if (lane == 0) red.f[par][1][w] = m;
        block_sum<0, 1>(f, n, red, par);                     // (its barrier publishes the maxima too)
        m = fmaxf(fmaxf(red.f[par ^ 1][1][0], red.f[par ^ 1][1][1]), fmaxf(red.f[par ^ 1][1][2], red.f[par ^ 1][1][3]));
        const int nfin = n[0];
        bool restage = false;
        if (top_k > 0 && top_k < nfin) {
            T = descend<false>(zs, cnt, m, top_k, 0.f, red, par);
            restage = true;                                  // the search consumed the lists
        }
        if (top_p < 1.f && nfin > 0) {
            const uint32_t Tk = T;
            if (restage) {                                   // what top-k kept, from the row again (it is in L2)
                cnt = 0;
                for (int j = tid; j < V; j += SF_THREADS) {
                    float z;
                    if (alive(j, z) && ord_key(z) >= Tk) zs[tid + SF_THREADS * cnt++] = z;
                }
            }
            f[0] = 0.f;
            for (int i = 0; i < cnt; ++i) f[0] += __expf(zs[tid + SF_THREADS * i] - m);
            block_sum<1, 0>(f, n, red, par);
            T = descend<true>(zs, cnt, m, 0, top_p * f[0], red, par);
            T = T > Tk ? T : Tk;
        }
    }

    // ---- the draw over the kept words, counted
    int nk = 0;
    for (int j = tid; j < V; j += SF_THREADS) {
        float z;
        if (!alive(j, z) || ord_key(z) < T) continue;
        ++nk;
        d.step<true>(j, x[j]);                               // (alive: finite)
    }
    d.wave();
    nk = wave_sum_i32(nk);
    if (lane == 0) bn[w] = nk;
    const int64_t id = d.block(bv, bi, bm, bs);              // (nothing kept: word 0)
    if (tid == 0) {
        const int nkept = (bn[0] + bn[1]) + (bn[2] + bn[3]);
        if constexpr (EMBED) chosen = id;
        if (kept) kept[r] = nkept;
        d.commit(id, x, nkept == 1, r, ids_out, logp, lens, t, end_id);
    }
    if constexpr (EMBED) {
        __syncthreads();
        embed_row(E, chosen, out, ldo, W, r, p, seed, site_word, row0, SF_THREADS);
    }
}

__global__ __launch_bounds__(SF_THREADS) void sample_filter_embed_kernel(
    const float* __restrict__ logits, int64_t ld, int V, float tau, const float* __restrict__ E, int64_t* __restrict__ ids_out,
    float* __restrict__ out, int64_t ldo, int W, float* __restrict__ logp, int64_t* __restrict__ lens, int t, int64_t end_id, float p,
    uint64_t seed, uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p,
    int min_len, int g, const int64_t* hist, int64_t hist_stride, int32_t* __restrict__ kept) {
    sample_filter_embed_body<false>(logits, ld, V, tau, E, ids_out, out, ldo, W, logp, lens, t, end_id, p, seed, site_word, site_sample,
                                    row0, seed_ptr, top_k, top_p, min_len, g, hist, hist_stride, kept, SampleExcl{});
}

// The filtered step under exclusions (dlsg_sample_excl_embed): the same body with the tables' bans in the row's list.
__global__ __launch_bounds__(SF_THREADS) void sample_excl_embed_kernel(
    const float* __restrict__ logits, int64_t ld, int V, float tau, const float* __restrict__ E, int64_t* __restrict__ ids_out,
    float* __restrict__ out, int64_t ldo, int W, float* __restrict__ logp, int64_t* __restrict__ lens, int t, int64_t end_id, float p,
    uint64_t seed, uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p,
    int min_len, int g, const int64_t* hist, int64_t hist_stride, int32_t* __restrict__ kept, const SampleExcl e) {
    sample_filter_embed_body<true>(logits, ld, V, tau, E, ids_out, out, ldo, W, logp, lens, t, end_id, p, seed, site_word, site_sample,
                                   row0, seed_ptr, top_k, top_p, min_len, g, hist, hist_stride, kept, e);
}

// An ensemble's sampled step (dlsg_sample_ens).  Phase A: the row's V combined values into comb[r], in the operations of the
// ensemble beam step -- wave w takes the log-sum-exp of the members w, w + 4 (beam_row_lse: one wave per row, so the sum keeps that
// step's order), then every thread combines the classes tid, tid + 256, ... (beam_ens_combine; one member: x - lse, as
// dlsg_seq_logprob takes it).  Phase B: the filtered body under exclusions on comb[r] as its logits, without the embedding.  The
// barrier between the two is all the hand-over needs: comb[r] is written and read by this workgroup alone, a workgroup's waves share
// their CU's vector L1, which is write-through, and __syncthreads() waits for the stores (vmcnt(0)) in front of s_barrier.  comb is
// not __restrict__ and the body's loads of it all lie behind the barrier.
__global__ __launch_bounds__(SF_THREADS) void sample_ens_kernel(
    const EnsPack e, int V, float tau, float* comb, int64_t* __restrict__ ids_out, float* __restrict__ logp, int64_t* __restrict__ lens,
    int t, int64_t end_id, uint64_t seed, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p,
    int min_len, int g, const int64_t* hist, int64_t hist_stride, int32_t* __restrict__ kept, const SampleExcl excl) {
    __shared__ float lse_s[DLSG_ENS_MAX];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int m = w; m < e.M; m += SF_THREADS / 64) {         // (not unrolled: the member's pointer is read from the argument block)
        const float l = beam_row_lse(e.x[m] + (int64_t)r * e.ld[m], V, lane);
        if (lane == 0) lse_s[m] = l;
    }
    __syncthreads();
    const float* x[DLSG_ENS_MAX];
    float lse[DLSG_ENS_MAX];
#pragma unroll
    for (int m = 0; m < DLSG_ENS_MAX; ++m) {
        x[m] = m < e.M ? e.x[m] + (int64_t)r * e.ld[m] : nullptr;
        lse[m] = m < e.M ? lse_s[m] : 0.f;
    }
    float* c = comb + (int64_t)r * V;
    if (e.M == 1) {
        for (int j = tid; j < V; j += SF_THREADS) c[j] = x[0][j] - lse[0];
    } else {
        for (int j = tid; j < V; j += SF_THREADS) c[j] = beam_ens_combine(x, lse, e.w, e.logw, e.M, e.mode, j);
    }
    __syncthreads();
    sample_filter_embed_body<true, false>(comb, V, V, tau, nullptr, ids_out, nullptr, 0, 0, logp, lens, t, end_id, 0.f, seed, 0u,
                                          site_sample, row0, seed_ptr, top_k, top_p, min_len, g, hist, hist_stride, kept, excl);
}

// A forced prefix behind a sampled step (dlsg_sample_force_prefix): launched behind whichever of the three steps ran, on its
// arguments.  Row r reads the prefix of clip r / rows_per_clip and is forced at step t iff words 0 .. t of that row of the table
// all lie in [0, V); every other row returns at once.  A forced row's outputs are rewritten as sample_embed_kernel writes them for
// a word it draws: the word, its log-prob under softmax(x / tau) with the row's (max, sum-exp) in WordDraw's reduction order (each
// thread's strided online pair, wave(), block()'s merge) and commit()'s expression, the embedding under the same dropout stream;
// lens[r] goes back to L (a prefix holds no end_id and every earlier step of the row was forced) and kept[r] is 1.
__global__ __launch_bounds__(256) void sample_force_prefix_kernel(const float* __restrict__ logits, int64_t ld, int V, float tau,
                                                                  const float* __restrict__ E, int64_t* __restrict__ ids_out,
                                                                  float* __restrict__ out, int64_t ldo, int W, float* __restrict__ logp,
                                                                  int64_t* __restrict__ lens, int t, float p, uint64_t seed,
                                                                  uint32_t site_word, int64_t row0, const uint64_t* seed_ptr,
                                                                  const int64_t* __restrict__ prefix, int P, int rows_per_clip, int L,
                                                                  int32_t* __restrict__ kept) {
    __shared__ float bv[4], bm[4], bs[4];
    __shared__ int bi[4];
    const int r = blockIdx.x;
    const int64_t* px = prefix + (int64_t)(r / rows_per_clip) * P;
    int64_t id = -1;
    for (int j = 0; j <= t; ++j) {                           // (t < P: the launcher checks; every thread reads the same words)
        id = px[j];
        if (!(id >= 0 && id < V)) return;
    }
    if (seed_ptr) seed += *seed_ptr;
    const float* x = logits + (int64_t)r * ld;
    WordDraw d(tau, seed, 0u, row0 + r, V);
    d.gumbel = false;                                        // (no noise is drawn: the step keeps up the pair (m, s) of x * sc)
    for (int j = threadIdx.x; j < V; j += blockDim.x) d.step<false>(j, x[j]);
    d.wave();
    d.block(bv, bi, bm, bs);
    if (threadIdx.x == 0) {
        d.commit(id, x, false, r, ids_out, logp, lens, t, -1);
        lens[r] = L;
        if (kept) kept[r] = 1;
    }
    embed_row(E, id, out, ldo, W, r, p, seed, site_word, row0, blockDim.x);
}

// what the two sampled steps ask of their common arguments
bool sample_args_ok(int V, int W, float temperature) { return V >= 1 && W >= 0 && temperature >= 0.f; }
// and the filtered steps of theirs; reads_hist: something looks at the row's earlier words from step 1 on; maxv: the widest row the
// step holds in LDS
bool sample_filter_args_ok(int V, int W, float temperature, int top_k, float top_p, int min_len, int no_repeat_ngram, int t, int rows,
                           bool reads_hist, const int64_t* hist, int64_t hist_stride, int maxv = DLSG_SAMPLE_FILTER_MAXV) {
    return sample_args_ok(V, W, temperature) && V <= maxv && top_k >= 0 && top_p > 0.f && top_p <= 1.f &&
           min_len >= 0 && no_repeat_ngram >= 0 && t >= 0 && t < SF_MAXL && !(reads_hist && t > 0 && (!hist || hist_stride < rows));
}
#define ST(s) reinterpret_cast<hipStream_t>(s)

}  // namespace

extern "C" int dlsg_select_embed(const float* logits, int64_t ld, int V, const int64_t* captions, int L, int t,
                                 const int32_t* coins, const float* E, int64_t* ids_out, float* out, int64_t ldo, int rows, int W,
                                 float p, uint64_t seed, uint32_t site, int64_t row0, const uint64_t* seed_ptr, int prefilled,
                                 void* stream) {
    if (rows == 0) return DLSG_OK;
    hipLaunchKernelGGL(select_embed_kernel, dim3(rows), dim3(256), 0, ST(stream), logits, ld, V, captions, L, t, coins, E, ids_out,
                       out, ldo, W, p, seed, site, row0, seed_ptr, prefilled);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_sample_embed(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out, float* out,
                                 int64_t ldo, int W, float* logp, int64_t* lens, int t, int64_t end_id, int rows, float p, uint64_t seed,
                                 uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, void* stream) {
    if (rows == 0) return DLSG_OK;
    if (!sample_args_ok(V, W, temperature)) return DLSG_EINVAL;
    hipLaunchKernelGGL(sample_embed_kernel, dim3(rows), dim3(256), 0, ST(stream), logits, ld, V, temperature, E, ids_out, out, ldo, W,
                       logp, lens, t, end_id, p, seed, site_word, site_sample, row0, seed_ptr);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_sample_force_prefix(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out,
                                        float* out, int64_t ldo, int W, float* logp, int64_t* lens, int t, int rows, float p,
                                        uint64_t seed, uint32_t site_word, int64_t row0, const uint64_t* seed_ptr,
                                        const int64_t* prefix, int P, int rows_per_clip, int L, int32_t* kept, void* stream) {
    if (!sample_args_ok(V, W, temperature) || rows < 0 || L < 1 || t < 0 || t >= L || P < 0 || P > L - 1 || (P > 0 && !prefix))
        return DLSG_EINVAL;
    if (rows_per_clip < 1 || rows % rows_per_clip != 0) return DLSG_EINVAL;
    if (rows == 0 || t >= P) return DLSG_OK;                 // (no row is forced at a step behind the table's width)
    if (!logits || !E || !ids_out || !out || !logp || !lens) return DLSG_EINVAL;
    hipLaunchKernelGGL(sample_force_prefix_kernel, dim3(rows), dim3(256), 0, ST(stream), logits, ld, V, temperature, E, ids_out, out,
                       ldo, W, logp, lens, t, p, seed, site_word, row0, seed_ptr, prefix, P, rows_per_clip, L, kept);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}
extern "C" int dlsg_argmax(const float* logits, int64_t ld, int64_t* ids, int rows, int V, void* stream) {
    if (rows == 0) return DLSG_OK;
    hipLaunchKernelGGL(argmax_kernel, dim3(rows), dim3(256), 0, ST(stream), logits, ld, ids, V);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_sample_filter_embed(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out,
                                        float* out, int64_t ldo, int W, float* logp, int64_t* lens, int t, int64_t end_id, int rows,
                                        float p, uint64_t seed, uint32_t site_word, uint32_t site_sample, int64_t row0,
                                        const uint64_t* seed_ptr, int top_k, float top_p, int min_len, int no_repeat_ngram,
                                        const int64_t* hist, int64_t hist_stride, int32_t* kept, void* stream) {
    if (rows == 0) return DLSG_OK;
    if (!sample_filter_args_ok(V, W, temperature, top_k, top_p, min_len, no_repeat_ngram, t, rows, no_repeat_ngram > 0, hist, hist_stride))
        return DLSG_EINVAL;
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] {
        attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_filter_embed_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, DLSG_SAMPLE_FILTER_MAXV * 4);
    });
    if (attr_rc != hipSuccess) return DLSG_ELAUNCH;
    hipLaunchKernelGGL(sample_filter_embed_kernel, dim3(rows), dim3(SF_THREADS), (size_t)V * 4, ST(stream),
                       logits, ld, V, temperature, E, ids_out, out, ldo, W, logp, lens, t, end_id, p, seed, site_word, site_sample,
                       row0, seed_ptr, top_k, top_p, min_len, no_repeat_ngram, hist, hist_stride, kept);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_sample_excl_embed(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out,
                                      float* out, int64_t ldo, int W, float* logp, int64_t* lens, int t, int64_t end_id, int rows,
                                      float p, uint64_t seed, uint32_t site_word, uint32_t site_sample, int64_t row0,
                                      const uint64_t* seed_ptr, int top_k, float top_p, int min_len, int no_repeat_ngram,
                                      const int64_t* hist, int64_t hist_stride, int32_t* kept, const int64_t* excl_shared, int NS,
                                      const int64_t* excl_clip, int NC, int P, int rows_per_clip, void* stream) {
    if (rows == 0) return DLSG_OK;
    if (!beam_excl_ok(excl_shared, NS, excl_clip, NC, P)) return DLSG_EINVAL;
    if (rows_per_clip < 1 || rows % rows_per_clip != 0) return DLSG_EINVAL;
    if (!sample_filter_args_ok(V, W, temperature, top_k, top_p, min_len, no_repeat_ngram, t, rows, no_repeat_ngram > 0 || NS + NC > 0, hist,
                               hist_stride))
        return DLSG_EINVAL;
    if (NS + NC == 0) P = 1;
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] {
        attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_excl_embed_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, DLSG_SAMPLE_FILTER_MAXV * 4);
    });
    if (attr_rc != hipSuccess) return DLSG_ELAUNCH;
    const SampleExcl e{NS > 0 ? excl_shared : nullptr, NC > 0 ? excl_clip : nullptr, NS, NC, P, rows_per_clip};
    hipLaunchKernelGGL(sample_excl_embed_kernel, dim3(rows), dim3(SF_THREADS), (size_t)V * 4, ST(stream),
                       logits, ld, V, temperature, E, ids_out, out, ldo, W, logp, lens, t, end_id, p, seed, site_word, site_sample,
                       row0, seed_ptr, top_k, top_p, min_len, no_repeat_ngram, hist, hist_stride, kept, e);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_sample_ens(const float* const* logits, const int64_t* ld, const float* w, const float* logw, int M, int mode, int V,
                               float temperature, float* comb, int64_t* ids_out, float* logp, int64_t* lens, int t, int64_t end_id,
                               int rows, uint64_t seed, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k,
                               float top_p, int min_len, int no_repeat_ngram, const int64_t* hist, int64_t hist_stride, int32_t* kept,
                               const int64_t* excl_shared, int NS, const int64_t* excl_clip, int NC, int P, int rows_per_clip,
                               void* stream) {
    EnsPack e;
    if (!beam_ens_pack(logits, ld, w, logw, M, mode, e) || !beam_excl_ok(excl_shared, NS, excl_clip, NC, P)) return DLSG_EINVAL;
    if (rows < 0 || rows_per_clip < 1 || rows % rows_per_clip != 0) return DLSG_EINVAL;
    // a control: what makes the one-model sampler leave dlsg_sample_embed for a step that holds the row in LDS
    const bool control = top_k > 0 || top_p < 1.f || min_len > 0 || no_repeat_ngram > 0 || NS + NC > 0;
    if (!sample_filter_args_ok(V, 0, temperature, top_k, top_p, min_len, no_repeat_ngram, t, rows, no_repeat_ngram > 0 || NS + NC > 0, hist,
                               hist_stride, control ? DLSG_SAMPLE_FILTER_MAXV : 0x7fffffff))
        return DLSG_EINVAL;
    if (rows == 0) return DLSG_OK;
    if (!comb || !ids_out || !logp || !lens) return DLSG_EINVAL;
    if (NS + NC == 0) P = 1;
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] {
        attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_ens_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      DLSG_SAMPLE_FILTER_MAXV * 4);
    });
    if (attr_rc != hipSuccess) return DLSG_ELAUNCH;
    const SampleExcl x{NS > 0 ? excl_shared : nullptr, NC > 0 ? excl_clip : nullptr, NS, NC, P, rows_per_clip};
    // the candidate lists of the two threshold searches are the only use of the dynamic LDS
    const size_t lds = temperature > 0.f && (top_k > 0 || top_p < 1.f) ? (size_t)V * 4 : 0;
    hipLaunchKernelGGL(sample_ens_kernel, dim3(rows), dim3(SF_THREADS), lds, ST(stream), e, V, temperature, comb, ids_out, logp, lens, t,
                       end_id, seed, site_sample, row0, seed_ptr, top_k, top_p, min_len, no_repeat_ngram, hist, hist_stride, kept, x);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

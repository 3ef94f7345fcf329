// The phases of a beam-search step (gfx950), one definition each: the step kernels of beam.hip are compositions of them, and
// the filtered sampler (sample.hip) bans words by the same rule.  A step is one workgroup per clip and one wave per beam row:
// every row offers its K best (log-prob, class) candidates in LDS, then wave 0 takes the K best of the clip's candidates.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "dlsg.h"
#include "wordpick.hpp"

namespace dlsg {

constexpr int BEAM_MAXK = 8;
constexpr int BEAM_MAXL = 64;           // history positions: lane i of a row's wave holds token i

// (value, index) order of the search: larger value first, ties to the smaller index (torch.topk on equal log-probs is not
// specified; the oracle and the reference fixtures agree with this rule on every golden case)
__device__ __forceinline__ bool beam_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ bool beam_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, dpp_i32<0xB1>(v));
    v = min(v, dpp_i32<0x4E>(v));
    v = min(v, dpp_i32<0x141>(v));
    v = min(v, dpp_i32<0x140>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// the best (value, index) pair of the wave, to every lane: two DPP reductions instead of twelve ds_bpermute round trips
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
    const float m = dlsg::wave_max(v);
    i = wave_min_i32(v == m ? i : 0x7fffffff);
    v = m;
}
// the same pair of float64 values (the stochastic step selects by them): a butterfly under beam_better, which is commutative, so
// every lane ends with the same pair
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (beam_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// ------------------------------------------------------------------------------------------------ ban list
// The classes a row may not choose, by ONE wave from the row's history in LDS (hist[i] = token i for i < t, -1 behind): with
// g = no_repeat_ngram, every h[i + g - 1] whose g - 1 predecessors equal the last g - 1 tokens of the history (lane i: the g-gram
// that starts at i), and `end` while t < min_len.  ban holds up to BEAM_MAXL + 1 classes; lane 0 stores their number.
__device__ __forceinline__ void beam_ban_list(const int* hist, int t, int g, int min_len, int end, int* ban, int* nban) {
    const int lane = threadIdx.x & 63;
    int n = 0;
    if (g > 0 && t >= g) {                                   // (never at step 0)
        bool hit = lane <= t - g;
        for (int j = 0; hit && j < g - 1; ++j) hit = hist[lane + j] == hist[t - g + 1 + j];
        const unsigned long long m = __ballot(hit);
        if (hit) ban[__popcll(m & ((1ull << lane) - 1ull))] = hist[lane + g - 1];
        n = __popcll(m);
    }
    if (lane == 0) {
        if (t < min_len) ban[n++] = end;
        *nban = n;
    }
}

// The ban lists of a workgroup's rows, wave w for `row` (every wave calls it: two barriers): the row's history from hist_in
// (B*k, L) into LDS, then the list of a row that is `live` (searched at this step and not ended).  The LDS arrays come whole and
// are indexed by w here: handed in as the wave's row pointers they cost two VGPRs, and beam_select_groups_kernel<8> a wave of
// occupancy (profiles/beam_step_resources_parent_vs_tree.md).
template <int K>
__device__ __forceinline__ void beam_row_bans(const int64_t* __restrict__ hist_in, int64_t row, int L, int t, int g, int min_len,
                                              int end, bool live, int (&hist)[K][BEAM_MAXL], int (&ban)[K][BEAM_MAXL + 1], int (&nban)[K]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (g > 0 && t >= g) hist[w][lane] = lane < t ? (int)hist_in[row * L + lane] : -1;
    __syncthreads();
    if (live) beam_ban_list(hist[w], t, g, min_len, end, ban[w], &nban[w]);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ a row's K candidates
// A beam that has ended offers `end` at its own log-prob and nothing else: the K - 1 other slots are -inf, with classes that are
// distinct and not `end`.  lp / cls: the row's K slots.
template <int K>
__device__ __forceinline__ void beam_offer_ended(const dlsg_beam_select_args& a, int lane, float base, float* lp, int* cls) {
    if (lane < K) {
        lp[lane] = lane == 0 ? base : -INFINITY;
        cls[lane] = lane == 0 ? a.end : (lane - 1 < a.end ? lane - 1 : lane);
    }
}
// a live beam offers the wave's K best (value, class) at value + base
template <int K>
__device__ __forceinline__ void beam_offer_live(int lane, const float (&bv)[K], const int (&bi)[K], float base, float* lp, int* cls) {
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            lp[c] = bv[c] + base;
            cls[c] = bi[c];
        }
    }
}

// A lane's K best of the elements it has seen, sorted: empty, then one push per element, then the wave's K best by merge.
template <int K>
__device__ __forceinline__ void beam_topk_clear(float (&tv)[K], int (&ti)[K]) {
#pragma unroll
    for (int q = 0; q < K; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
}
// BAN: the classes in ban[0..nban) count as -inf.  The list is looked at only for an element that would enter the lane's K best.
template <int K, bool BAN>
__device__ __forceinline__ void beam_topk_push(float (&tv)[K], int (&ti)[K], float cv, int ci, const int* ban, int nban) {
    if (!beam_better(cv, ci, tv[K - 1], ti[K - 1])) return;
    if constexpr (BAN) {
        for (int q = 0; q < nban; ++q) cv = ban[q] == ci ? -INFINITY : cv;
        if (!beam_better(cv, ci, tv[K - 1], ti[K - 1])) return;
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {                           // one bubble pass keeps tv sorted
        const bool up = beam_better(cv, ci, tv[q], ti[q]);
        const float nv = up ? tv[q] : cv;
        const int ni = up ? ti[q] : ci;
        tv[q] = up ? cv : tv[q];
        ti[q] = up ? ci : ti[q];
        cv = nv; ci = ni;
    }
}
// the K best of the wave from the lanes' sorted lists (which it consumes): K rounds over the lanes' heads
template <int K>
__device__ __forceinline__ void beam_topk_merge(float (&tv)[K], int (&ti)[K], float (&outv)[K], int (&outi)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
        float bv = tv[0];
        int bi = ti[0];
        wave_argmax(bv, bi);
        outv[c] = bv; outi[c] = bi;
        if (ti[0] == bi && bi != 0x7fffffff) {               // the winning lane pops its head
#pragma unroll
            for (int q = 0; q + 1 < K; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
            tv[K - 1] = -INFINITY; ti[K - 1] = 0x7fffffff;
        }
    }
}

// One model's row: the K best classes of a V-wide logit row and the row's log-sum-exp, ONE wave.  The row is read twice (maximum +
// each lane's own K best in the first pass, the exponential sum in the second -- same summation order as a plain strided loop, so
// the log-probs are bit-identical to a 2 + K pass form), then the merge.  The selection is on raw logits; the caller subtracts lse.
// With a ban list the row's maximum and exponential sum stay those of the whole row.
template <int K, bool BAN = false>
__device__ __forceinline__ void beam_row_topk(const float* x, int V, int lane, float& lse, float (&outv)[K], int (&outi)[K],
                                              const int* ban = nullptr, int nban = 0) {
    float tv[K];
    int ti[K];
    beam_topk_clear<K>(tv, ti);
    float m = -INFINITY;
    for (int j = lane; j < V; j += 64) {
        const float cv = x[j];
        m = fmaxf(m, cv);
        beam_topk_push<K, BAN>(tv, ti, cv, j, ban, nban);
    }
    m = dlsg::wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < V; j += 64) sum += expf(x[j] - m);
    sum = dlsg::wave_sum(sum);
    lse = logf(sum) + m;
    beam_topk_merge<K>(tv, ti, outv, outi);
}

// An ensemble's row: a live beam's V candidate values are combined from M logit rows, one per member.  Per member the row's
// log-sum-exp in beam_row_topk's order (strided maximum + wave_max, strided exponential sum + wave_sum), then per class, in member
// order and float32,
//   mode 0: c = mx + logf(sum_m expf(v_m - mx)),  v_m = (x_m - lse_m) + logw_m,  mx = max_m v_m   (log of the weighted mean probability)
//   mode 1: c = sum_m w_m (x_m - lse_m)                                                          (weighted mean log-probability)
// and the K best unbanned c of the row.  With one member of weight 1 both modes give c = x - lse exactly, the value the one-model
// step ranks by (on raw logits: it reads the row twice, not three times).  The M pointers, strides and weights travel by value in
// the argument block; lse_s: the row's DLSG_ENS_MAX floats of LDS (the member loop that fills it is not unrolled).
struct EnsPack {
    const float* x[DLSG_ENS_MAX];
    int64_t ld[DLSG_ENS_MAX];
    float w[DLSG_ENS_MAX], logw[DLSG_ENS_MAX];
    int M, mode;
};
// the members' host arrays into the block a launcher passes by value (host); false for what every ensemble entry point refuses
inline bool beam_ens_pack(const float* const* logits, const int64_t* ld, const float* w, const float* logw, int M, int mode, EnsPack& e) {
    if (!logits || !ld || !w || !logw || M < 1 || M > DLSG_ENS_MAX || (mode != 0 && mode != 1)) return false;
    e = {};
    for (int m = 0; m < M; ++m) {
        if (!logits[m]) return false;
        e.x[m] = logits[m]; e.ld[m] = ld[m]; e.w[m] = w[m]; e.logw[m] = logw[m];
    }
    e.M = M; e.mode = mode;
    return true;
}
// The two steps of beam_ens_row_topk for the kernels that want the combined value without the K best (dlsg_seq_logprob,
// dlsg_beam_force_prefix, dlsg_sample_ens), operation for operation: that function keeps its own statement of them, because calling
// these from it changed the code the compiler emits for the ensemble and group step kernels, and those stay as they are.
// tests/test_gpu_rescore.py holds the two statements together: a word's value here equals the new_lp of dlsg_beam_select_hist /
// dlsg_beam_select_ens bit for bit.
// a member's row: its log-sum-exp, ONE wave, to every lane
__device__ __forceinline__ float beam_row_lse(const float* x, int V, int lane) {
    float mx = -INFINITY;
    for (int j = lane; j < V; j += 64) mx = fmaxf(mx, x[j]);
    mx = dlsg::wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < V; j += 64) sum += expf(x[j] - mx);
    sum = dlsg::wave_sum(sum);
    return logf(sum) + mx;
}
// class j's combined value from the members' rows x and their log-sum-exps
__device__ __forceinline__ float beam_ens_combine(const float* const (&x)[DLSG_ENS_MAX], const float (&lse)[DLSG_ENS_MAX],
                                                  const float (&w)[DLSG_ENS_MAX], const float (&logw)[DLSG_ENS_MAX], int M, int mode,
                                                  int j) {
    float c;
    if (mode == 0) {
        float v[DLSG_ENS_MAX], mx = -INFINITY, sum = 0.f;
#pragma unroll
        for (int m = 0; m < DLSG_ENS_MAX; ++m)
            if (m < M) { v[m] = (x[m][j] - lse[m]) + logw[m]; mx = fmaxf(mx, v[m]); }
#pragma unroll
        for (int m = 0; m < DLSG_ENS_MAX; ++m)
            if (m < M) sum += expf(v[m] - mx);
        c = mx == -INFINITY ? -INFINITY : mx + logf(sum);
    } else {
        c = 0.f;
#pragma unroll
        for (int m = 0; m < DLSG_ENS_MAX; ++m)
            if (m < M) c += w[m] * (x[m][j] - lse[m]);
    }
    return c;
}

template <int K>
__device__ __forceinline__ void beam_ens_row_topk(const EnsPack& e, int64_t row, int V, int lane, float* lse_s, const int* ban,
                                                  int nban, float (&bv)[K], int (&bi)[K]) {
    for (int m = 0; m < e.M; ++m) {                          // every lane writes the wave's value and reads back its own store
        const float* x = e.x[m] + row * e.ld[m];
        float mx = -INFINITY;
        for (int j = lane; j < V; j += 64) mx = fmaxf(mx, x[j]);
        mx = dlsg::wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < V; j += 64) sum += expf(x[j] - mx);
        sum = dlsg::wave_sum(sum);
        lse_s[m] = logf(sum) + mx;
    }
    const float* x[DLSG_ENS_MAX];
    float lse[DLSG_ENS_MAX];
#pragma unroll
    for (int m = 0; m < DLSG_ENS_MAX; ++m) {
        x[m] = m < e.M ? e.x[m] + row * e.ld[m] : nullptr;
        lse[m] = m < e.M ? lse_s[m] : 0.f;
    }
    float tv[K];
    int ti[K];
    beam_topk_clear<K>(tv, ti);
    for (int j = lane; j < V; j += 64) {
        float c;
        if (e.mode == 0) {
            float v[DLSG_ENS_MAX], mx = -INFINITY, sum = 0.f;
#pragma unroll
            for (int m = 0; m < DLSG_ENS_MAX; ++m)
                if (m < e.M) { v[m] = (x[m][j] - lse[m]) + e.logw[m]; mx = fmaxf(mx, v[m]); }
#pragma unroll
            for (int m = 0; m < DLSG_ENS_MAX; ++m)
                if (m < e.M) sum += expf(v[m] - mx);
            c = mx == -INFINITY ? -INFINITY : mx + logf(sum);
        } else {
            c = 0.f;
#pragma unroll
            for (int m = 0; m < DLSG_ENS_MAX; ++m)
                if (m < e.M) c += e.w[m] * (x[m][j] - lse[m]);
        }
        beam_topk_push<K, true>(tv, ti, c, j, ban, nban);
    }
    beam_topk_merge<K>(tv, ti, bv, bi);
}

// ------------------------------------------------------------------------------------------------ a stochastic row
// -log(-log u) in float64, u = (hi + 1/2) 2^-24 from the 24 hash bits gumbel_key draws its float32 noise from
__device__ __forceinline__ double gumbel_noise64(uint64_t seed, uint32_t site, uint64_t ctr) {
    const uint32_t hi = counter_hash(seed, site, ctr) >> 8;
    return -log(-log(((double)hi + 0.5) * (1.0 / 16777216.0)));
}
// log(1 - exp(a)) for a <= 0
__device__ __forceinline__ double log1mexp(double a) { return a > -0.6931471805599453 ? log(-expm1(a)) : log1p(-exp(a)); }

// Stochastic beam search (Kool, van Hoof & Welling 2019): a live row's K children, ONE wave.  One pass over the row: z = x * sc as
// WordDraw tempers it, the K largest gumbel_key(z) (wordpick.hpp: the key the sampler ranks by) and the online (max, sum-exp) of z
// over the classes that are neither banned nor -inf / NaN.  Such a dead class has key -inf, so that a row with fewer than K live
// classes still names K distinct ones.  The ban list is scanned for every class, because the log-sum-exp leaves the banned
// classes out (the filtered sampler's convention).  Then lane c < K works out child c in float64: with phi the parent's
// log-prob, T its perturbed value and noise = -log(-log u) of the key's own 24 hash bits,
//   g = phi + (z - lse) + noise,  Z = max of the K values g,  v = T - g + log1mexp(g - Z),  G = T - max(0, v) - log1p(exp(-|v|))
// -- the children's perturbed values conditioned on their maximum being T; the largest child gets T itself.  lp / cls / G: the
// row's K slots: phi + ((z - m) - log s) in float32 (the sampler's log-prob), the class, G; a dead slot is -inf in both.
template <int K>
__device__ __forceinline__ void beam_offer_gumbel(const float* x, int V, int lane, float sc, uint64_t seed, uint32_t site, uint64_t key0,
                                                  const int* ban, int nban, float phi, double T, float* lp, int* cls, double* G) {
    float tv[K], bv[K];
    int ti[K], bi[K];
    beam_topk_clear<K>(tv, ti);
    float m = -INFINITY, s = 0.f;
    for (int j = lane; j < V; j += 64) {
        const float z = x[j] * sc;
        bool dead = !(z > -INFINITY);
        for (int q = 0; q < nban; ++q) dead |= ban[q] == j;
        beam_topk_push<K, false>(tv, ti, dead ? -INFINITY : gumbel_key(z, seed, site, key0 + j), j, nullptr, 0);
        if (!dead) lse_update<true>(m, s, z);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    beam_topk_merge<K>(tv, ti, bv, bi);
    float key = bv[0];
    int c = bi[0];
#pragma unroll
    for (int q = 1; q < K; ++q) {
        key = lane == q ? bv[q] : key;
        c = lane == q ? bi[q] : c;
    }
    float child = -INFINITY;
    double g = -INFINITY;
    if (lane < K && key > -INFINITY) {
        const float z = x[c] * sc;
        child = phi + ((z - m) - logf(s));
        g = (double)phi + (((double)z - (double)m) - log((double)s)) + gumbel_noise64(seed, site, key0 + c);
    }
    double Z = -INFINITY;
#pragma unroll
    for (int q = 0; q < K; ++q) Z = fmax(Z, __shfl(g, q, 64));
    if (lane < K) {
        double gt = -INFINITY;
        if (g > -INFINITY) {
            const double v = T - g + log1mexp(g - Z);
            gt = T - fmax(0.0, v) - log1p(exp(-fabs(v)));
        }
        lp[lane] = child;
        cls[lane] = c;
        G[lane] = gt;
    }
}

// ------------------------------------------------------------------------------------------------ lexical constraints
// A clip's constraints are C sets of W word ids, staged in LDS as cons[c * W + w] with -1 for padding (C * W <= 64: one lane per
// entry).  Bit c of a mask stands for constraint c.
constexpr int CONS_SLOTS = DLSG_CONS_MAX * DLSG_CONS_ALT;

// the constraints that hold `cls` as a valid entry (cls < 0: none).  Every lane reads the same entry: LDS broadcasts.
__device__ __forceinline__ unsigned beam_cons_of(const int* cons, int C, int W, int cls) {
    unsigned m = 0;
    for (int c = 0; c < C; ++c)
        for (int w = 0; w < W; ++w) m |= (cls >= 0 && cons[c * W + w] == cls) ? 1u << c : 0u;
    return m;
}
// the constraints with a valid entry
__device__ __forceinline__ unsigned beam_cons_present(const int* cons, int C, int W) {
    unsigned m = 0;
    for (int c = 0; c < C; ++c)
        for (int w = 0; w < W; ++w) m |= cons[c * W + w] >= 0 ? 1u << c : 0u;
    return m;
}

// The constraints a row has met, ONE wave, to every lane: lane i holds token i of the row's history (i < t), and per constraint a
// ballot over "the token is an entry of the set".  A function of the history row alone, so the search carries no mask along.
__device__ __forceinline__ unsigned beam_row_met(const int64_t* __restrict__ hist_in, int64_t row, int L, int t, const int* cons, int C,
                                                 int W) {
    const int lane = threadIdx.x & 63;
    const unsigned mine = beam_cons_of(cons, C, W, lane < t ? (int)hist_in[row * L + lane] : -1);
    unsigned met = 0;
    for (int c = 0; c < C; ++c) met |= __ballot((mine >> c) & 1u) ? 1u << c : 0u;
    return met;
}

// A live row's list B, ONE wave: per constraint c of `unmet` the best word of its set -- lane c * W + w reads the logit of entry w;
// a padding entry, a banned word, a -inf and a NaN logit are out; larger logit first, ties to the lower class -- offered at
// (x - lse) + base, the float32 operations of list A.  The slot is empty (-inf) for a constraint that is met or absent or has no
// such word, and for a class that is already in the row's list A (bi) or in an earlier slot of the row: the clip would get the
// same beam twice.  lp / cls: the row's C slots.
template <int K>
__device__ __forceinline__ void beam_offer_constraints(const float* x, int lane, const int* cons, int C, int W, unsigned unmet,
                                                       const int* ban, int nban, const int (&bi)[K], float lse, float base, float* lp,
                                                       int* cls) {
    const int id = lane < C * W ? cons[lane] : -1;
    const int mine = lane / W;
    float v = -INFINITY;
    if (id >= 0 && ((unmet >> mine) & 1u)) {
        const float xv = x[id];
        bool ok = xv > -INFINITY;                              // (NaN fails)
        for (int q = 0; q < nban; ++q) ok &= ban[q] != id;
        v = ok ? xv : -INFINITY;
    }
    int mypick = -1;                                           // lane c: the class in slot c
    for (int c = 0; c < C; ++c) {
        float bv = mine == c ? v : -INFINITY;
        int bc = bv > -INFINITY ? id : 0x7fffffff;
        wave_argmax(bv, bc);
        bool have = bc != 0x7fffffff;
#pragma unroll
        for (int q = 0; q < K; ++q) have &= bi[q] != bc;
        have &= __ballot(lane < c && mypick == bc) == 0ull;
        if (lane == c) {
            mypick = have ? bc : -1;
            lp[c] = have ? (bv - lse) + base : -INFINITY;
            cls[c] = have ? bc : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the clip's K best
// Row o of hist_out (B*k, L): the parent's row of hist_in up to t, the chosen class at t, `end` behind it (step 0 writes whole
// rows, so the search fills its own buffers).  One wave.
__device__ __forceinline__ void beam_write_hist(const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out, int64_t o,
                                                int64_t parent, int L, int t, int lane, int cls, int end) {
    if (lane < L) hist_out[o * L + lane] = lane < t ? hist_in[parent * L + lane] : (lane == t ? (int64_t)cls : (int64_t)end);
}

// The K best of the clip's nbeam * K candidates, by wave 0: pred, new_lp, back and rows of the clip's K new beams, and the number
// of `end` among them onto ended_count.  HIST: the new beams' history rows as well.  The candidates are ranked by cand_key: the
// log-probs themselves (float), or the stochastic step's perturbed values (double) -- then new_lp is the winner's cand_lp, -inf
// for a key of -inf, and key_out takes the key.
template <int K, bool HIST, class T = float>
__device__ __forceinline__ void beam_flat_merge(const dlsg_beam_select_args& a, int nbeam, int lane, const T* cand_key,
                                                const int* cand_cls, const int64_t* __restrict__ hist_in,
                                                int64_t* __restrict__ hist_out, int L, int t, const float* cand_lp = nullptr,
                                                T* __restrict__ key_out = nullptr) {
    const int b = blockIdx.x, k = K, n = nbeam * k;
    T v = lane < n ? cand_key[lane] : (T)-INFINITY;
    int idx = lane < n ? lane : 0x7fffffff;
    int n_end = 0;
    for (int c = 0; c < k; ++c) {
        T bv = v;
        int bi = idx;
        wave_argmax(bv, bi);
        if (lane == bi) v = (T)-INFINITY, idx = 0x7fffffff;     // remove the winner (it can win only once)
        if (bi == 0x7fffffff) bi = c < n ? c : 0;               // fewer than k finite candidates: any slot, log-prob -inf
        const int cls = cand_cls[bi];
        const int64_t o = (int64_t)b * k + c;
        if (lane == 0) {
            a.pred[o] = cls;
            if constexpr (std::is_same<T, float>::value) {
                a.new_lp[o] = bv;
            } else {
                a.new_lp[o] = bv == (T)-INFINITY ? -INFINITY : cand_lp[bi];
                key_out[o] = bv;
            }
            a.back[o] = bi / k;
            a.rows[o] = (int64_t)b * k + bi / k;
        }
        if constexpr (HIST) beam_write_hist(hist_in, hist_out, o, (int64_t)b * k + bi / k, L, t, lane, cls, a.end);
        n_end += cls == a.end;
    }
    if (lane == 0 && a.ended_count) atomicAdd(a.ended_count, n_end);
}

// Dynamic beam allocation (Post & Vilar 2018) over the clip's candidates, by wave 0.  Lane i holds two slots: candidate i of list A
// (row, then rank; index i) and candidate i of list B (row, then constraint; index 64 + i).  A candidate is a value above -inf
// (a NaN is none); its mask is its parent's met mask and the constraints of its class, its bank the mask's population count.
// Rounds until K output slots are filled or no candidate is left: bank C down to 0, the best candidate left in the bank -- larger
// value first, ties to the lower index -- takes the next output slot; an empty bank (seen by ballot) is skipped.  A slot q left
// over takes candidate q of list A at log-prob -inf, as beam_flat_merge fills it.  With one bank the picks are beam_flat_merge's.
template <int K>
__device__ __forceinline__ void beam_bank_merge(const dlsg_beam_select_args& a, int nbeam, int lane, const float* a_lp, const int* a_cls,
                                                const float* b_lp, const int* b_cls, const unsigned* met, const int* cons, int C, int W,
                                                const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out, int L, int t,
                                                int32_t* __restrict__ met_out) {
    const int b = blockIdx.x, Cd = C > 0 ? C : 1;
    float v0 = lane < nbeam * K ? a_lp[lane] : -INFINITY;
    float v1 = lane < nbeam * C ? b_lp[lane] : -INFINITY;
    unsigned m0 = 0, m1 = 0;
    int bank0 = -1, bank1 = -1;                               // -1: no candidate (never one, or taken)
    if (v0 > -INFINITY) {
        m0 = met[lane / K] | beam_cons_of(cons, C, W, a_cls[lane]);
        bank0 = __popc(m0);
    }
    if (v1 > -INFINITY) {
        m1 = met[lane / Cd] | beam_cons_of(cons, C, W, b_cls[lane]);
        bank1 = __popc(m1);
    }
    int filled = 0, n_end = 0;
    for (bool any = true; any && filled < K;) {
        any = false;
        for (int bank = C; bank >= 0 && filled < K; --bank) {
            if ((__ballot(bank0 == bank) | __ballot(bank1 == bank)) == 0ull) continue;
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            if (bank0 == bank && (bank1 != bank || v0 >= v1)) { bv = v0; bi = lane; }
            else if (bank1 == bank) { bv = v1; bi = 64 + lane; }
            wave_argmax(bv, bi);
            if (bi == lane) bank0 = -1;
            if (bi == 64 + lane) bank1 = -1;
            const bool listb = bi >= 64;
            const int j = bi & 63;
            const int cls = listb ? b_cls[j] : a_cls[j];
            const int par = listb ? j / Cd : j / K;
            const unsigned mask = __shfl(listb ? m1 : m0, j, 64);
            const int64_t o = (int64_t)b * K + filled;
            if (lane == 0) {
                a.pred[o] = cls;
                a.new_lp[o] = bv;
                a.back[o] = par;
                a.rows[o] = (int64_t)b * K + par;
                if (met_out) met_out[o] = (int32_t)mask;
            }
            beam_write_hist(hist_in, hist_out, o, (int64_t)b * K + par, L, t, lane, cls, a.end);
            n_end += cls == a.end;
            ++filled;
            any = true;
        }
    }
    for (; filled < K; ++filled) {
        const int cls = a_cls[filled];
        const int64_t o = (int64_t)b * K + filled;
        if (lane == 0) {
            a.pred[o] = cls;
            a.new_lp[o] = -INFINITY;
            a.back[o] = 0;
            a.rows[o] = (int64_t)b * K;
            if (met_out) met_out[o] = 0;
        }
        beam_write_hist(hist_in, hist_out, o, (int64_t)b * K, L, t, lane, cls, a.end);
        n_end += cls == a.end;
    }
    if (lane == 0 && a.ended_count) atomicAdd(a.ended_count, n_end);
}

// ------------------------------------------------------------------------------------------------ phrase constraints
// A clip's constraints are C sets of W alternative phrases of up to P <= DLSG_PHRASE_MAX words: alternative a = c * W + w lies in LDS
// as phr[a * P + j], cut behind its leading run of ids in [0, V) (-1 from there on), with its length in n[a] (0: absent).
constexpr int PHRASE_SLOTS = CONS_SLOTS * DLSG_PHRASE_MAX;

// Phase 0, thread a < CW of the workgroup: alternative a of the clip from global memory (phr: the clip's CW * P entries)
__device__ __forceinline__ void beam_stage_phrases(const int64_t* __restrict__ phr, int CW, int P, int V, int* phr_s, int* n_s) {
    const int a = threadIdx.x;
    if (a < CW) {
        int n = 0;
        bool run = true;
        for (int j = 0; j < P; ++j) {
            const int64_t id = phr[(int64_t)a * P + j];
            run = run && id >= 0 && id < V;
            phr_s[a * P + j] = run ? (int)id : -1;
            n += run;
        }
        n_s[a] = n;
    }
}

// What a row's history (hist[i] = token i for i < t, in LDS) says about the clip's phrases, ONE wave.  To every lane: the mask of
// the constraints that are met (lane i tests "alternative a starts at token i", one ballot per constraint), `present`, and q, the
// largest progress among the valid alternatives of the unmet constraints.  Lane a < C * W: the border mask of alternative a -- bit
// j: j <= t, j < n[a] and the last j tokens equal its first j words (bit 0 of a valid alternative is set) -- in border[a] and
// `mine`; its progress is the highest bit.  border[a] is 0 for every other lane below CONS_SLOTS.
__device__ __forceinline__ unsigned beam_row_phrases(const int* hist, int t, const int* phr, const int* n_s, int C, int W, int P,
                                                     unsigned char* border, unsigned& present, int& q, unsigned& mine) {
    const int lane = threadIdx.x & 63;
    unsigned met = 0;
    present = 0;
    for (int c = 0; c < C; ++c) {
        bool hit = false;
        for (int w = 0; w < W; ++w) {
            const int a = c * W + w, n = n_s[a];                 // (every lane reads the same entry: LDS broadcasts)
            present |= n > 0 ? 1u << c : 0u;
            bool m = n > 0 && lane + n <= t;
            for (int j = 0; j < P; ++j) m = m && (j >= n || hist[lane + j] == phr[a * P + j]);
            hit |= m;
        }
        met |= __ballot(hit) ? 1u << c : 0u;
    }
    const int n = lane < C * W ? n_s[lane] : 0;
    mine = n > 0 ? 1u : 0u;
    for (int j = 1; j < P; ++j) {
        bool ok = j < n && j <= t;
        for (int i = 0; ok && i < j; ++i) ok = hist[t - j + i] == phr[lane * P + i];
        mine |= ok ? 1u << j : 0u;
    }
    border[lane] = (unsigned char)mine;
    const bool open = n > 0 && (((present & ~met) >> (lane / W)) & 1u);
    q = 0;
    for (int j = 1; j < P; ++j) q = __ballot(open && (mine >> j)) ? j : q;
    return met;
}

// A live row's list B with phrases, ONE wave: lane a proposes the next word of alternative a, phr[a * P + p] behind a progress of p
// (`border`: the lane's mask from beam_row_phrases), with a gain of DLSG_PHRASE_MAX if the word completes the phrase, else p + 1.  A
// proposal is out as an entry of beam_offer_constraints is; the slot of an unmet constraint takes its proposal of the largest gain,
// then the larger logit, then the lower class, and is offered, or left empty, by that function's rules.  With one-word phrases
// every gain is equal and the slots are beam_offer_constraints' bit for bit.
template <int K>
__device__ __forceinline__ void beam_offer_phrases(const float* x, int lane, const int* phr, const int* n_s, int C, int W, int P,
                                                   unsigned unmet, unsigned border, const int* ban, int nban, const int (&bi)[K], float lse,
                                                   float base, float* lp, int* cls) {
    const int n = lane < C * W ? n_s[lane] : 0;
    const int mine = lane / W;
    float v = -INFINITY, gain = 0.f;
    int id = -1;
    if (n > 0 && ((unmet >> mine) & 1u)) {
        const int p = 31 - __clz((int)border);
        id = phr[lane * P + p];
        const float xv = x[id];
        bool ok = xv > -INFINITY;                              // (NaN fails)
        for (int q = 0; q < nban; ++q) ok &= ban[q] != id;
        v = ok ? xv : -INFINITY;
        gain = p + 1 == n ? (float)DLSG_PHRASE_MAX : (float)(p + 1);
    }
    int mypick = -1;                                           // lane c: the class in slot c
    for (int c = 0; c < C; ++c) {
        const bool in = mine == c && v > -INFINITY;
        const float top = dlsg::wave_max(in ? gain : 0.f);
        float bv = in && gain == top ? v : -INFINITY;
        int bc = bv > -INFINITY ? id : 0x7fffffff;
        wave_argmax(bv, bc);
        bool have = bc != 0x7fffffff;
#pragma unroll
        for (int q = 0; q < K; ++q) have &= bi[q] != bc;
        have &= __ballot(lane < c && mypick == bc) == 0ull;
        if (lane == c) {
            mypick = have ? bc : -1;
            lp[c] = have ? (bv - lse) + base : -INFINITY;
            cls[c] = have ? bc : 0;
        }
    }
}

// The bank of the history "parent + [cls]" from the parent's state alone: its met mask, its progress qpar and its border masks
// (border[a], LDS).  cls completes alternative a iff bit n - 1 of the mask is set and the phrase's last word is cls; behind it the
// progress of a is the largest j < n with bit j - 1 set and word j - 1 equal to cls, and that of the row the largest over the
// alternatives of the constraints still unmet.  `end` changes neither.  -> popcount(mask) * DLSG_PHRASE_MAX + progress
__device__ __forceinline__ int beam_phrase_bank(const int* phr, const int* n_s, int C, int W, int P, const unsigned char* border,
                                                unsigned met, int qpar, int cls, int end, unsigned& mask) {
    mask = met;
    if (cls == end) return __popc(met) * DLSG_PHRASE_MAX + qpar;
    for (int c = 0; c < C; ++c)
        for (int w = 0; w < W; ++w) {
            const int a = c * W + w, n = n_s[a];
            if (n > 0 && ((border[a] >> (n - 1)) & 1) && phr[a * P + n - 1] == cls) mask |= 1u << c;
        }
    int q = 0;
    for (int c = 0; c < C; ++c) {
        if ((mask >> c) & 1u) continue;
        for (int w = 0; w < W; ++w) {
            const int a = c * W + w, n = n_s[a];
            for (int j = 1; j < n; ++j)
                if (((border[a] >> (j - 1)) & 1) && phr[a * P + j - 1] == cls) q = max(q, j);
        }
    }
    return __popc(mask) * DLSG_PHRASE_MAX + q;
}

// beam_bank_merge over the banks (constraints met, progress) of beam_phrase_bank, by wave 0; the candidates, their indices and the
// rules for ties and left-over slots are that function's.  Every pick takes the best candidate left in the highest non-empty bank
// below the one served before it; when none is below, the round starts again from the top.  bank_out (optional): the new beam's
// bank, 0 for a left-over slot.
template <int K>
__device__ __forceinline__ void beam_phrase_merge(const dlsg_beam_select_args& a, int nbeam, int lane, const float* a_lp, const int* a_cls,
                                                  const float* b_lp, const int* b_cls, const unsigned* met, const int* qrow,
                                                  const unsigned char (&border)[K][CONS_SLOTS], const int* phr, const int* n_s, int C,
                                                  int W, int P, const int64_t* __restrict__ hist_in, int64_t* __restrict__ hist_out,
                                                  int L, int t, int32_t* __restrict__ met_out, int32_t* __restrict__ bank_out) {
    const int b = blockIdx.x, Cd = C > 0 ? C : 1;
    float v0 = lane < nbeam * K ? a_lp[lane] : -INFINITY;
    float v1 = lane < nbeam * C ? b_lp[lane] : -INFINITY;
    unsigned m0 = 0, m1 = 0;
    int bank0 = -1, bank1 = -1;                               // -1: no candidate (never one, or taken)
    if (v0 > -INFINITY) {
        const int par = lane / K;
        bank0 = beam_phrase_bank(phr, n_s, C, W, P, border[par], met[par], qrow[par], a_cls[lane], a.end, m0);
    }
    if (v1 > -INFINITY) {
        const int par = lane / Cd;
        bank1 = beam_phrase_bank(phr, n_s, C, W, P, border[par], met[par], qrow[par], b_cls[lane], a.end, m1);
    }
    constexpr int TOP = (DLSG_CONS_MAX + 1) * DLSG_PHRASE_MAX;  // above every bank
    int filled = 0, n_end = 0, cur = TOP;
    while (filled < K) {
        const int below = max(bank0 < cur ? bank0 : -1, bank1 < cur ? bank1 : -1);
        const int bank = -wave_min_i32(-below);                // the highest bank below cur that has a candidate
        if (bank < 0) {
            if (cur == TOP) break;                            // no candidate is left
            cur = TOP;
            continue;
        }
        cur = bank;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (bank0 == bank && (bank1 != bank || v0 >= v1)) { bv = v0; bi = lane; }
        else if (bank1 == bank) { bv = v1; bi = 64 + lane; }
        wave_argmax(bv, bi);
        if (bi == lane) bank0 = -1;
        if (bi == 64 + lane) bank1 = -1;
        const bool listb = bi >= 64;
        const int j = bi & 63;
        const int cls = listb ? b_cls[j] : a_cls[j];
        const int par = listb ? j / Cd : j / K;
        const unsigned mask = __shfl(listb ? m1 : m0, j, 64);
        const int64_t o = (int64_t)b * K + filled;
        if (lane == 0) {
            a.pred[o] = cls;
            a.new_lp[o] = bv;
            a.back[o] = par;
            a.rows[o] = (int64_t)b * K + par;
            if (met_out) met_out[o] = (int32_t)mask;
            if (bank_out) bank_out[o] = bank;
        }
        beam_write_hist(hist_in, hist_out, o, (int64_t)b * K + par, L, t, lane, cls, a.end);
        n_end += cls == a.end;
        ++filled;
    }
    for (; filled < K; ++filled) {
        const int cls = a_cls[filled];
        const int64_t o = (int64_t)b * K + filled;
        if (lane == 0) {
            a.pred[o] = cls;
            a.new_lp[o] = -INFINITY;
            a.back[o] = 0;
            a.rows[o] = (int64_t)b * K;
            if (met_out) met_out[o] = 0;
            if (bank_out) bank_out[o] = 0;
        }
        beam_write_hist(hist_in, hist_out, o, (int64_t)b * K, L, t, lane, cls, a.end);
        n_end += cls == a.end;
    }
    if (lane == 0 && a.ended_count) atomicAdd(a.ended_count, n_end);
}

// ------------------------------------------------------------------------------------------------ exclusions
// A clip's exclusions are NE = NS + NC entries of up to P <= DLSG_PHRASE_MAX words, the NS shared ones first: entry a lies in LDS as
// ex[a * P + j], cut behind its leading run of ids in [0, V) as beam_stage_phrases cuts an alternative, with its length in n[a]
// (0: absent).  The last word of an entry is banned for a row whose history ends with the words before it.
constexpr int EXCL_SLOTS = DLSG_EXCL_SHARED + DLSG_EXCL_CLIP;
constexpr int BEAM_BAN_EXCL = BEAM_MAXL + 1 + EXCL_SLOTS;      // a row's ban list with every entry matching at once
// what a launcher asks of the two tables (host): the steps under exclusions here and the sampler's in sample.hip
inline bool beam_excl_ok(const int64_t* excl_shared, int NS, const int64_t* excl_clip, int NC, int P) {
    if (NS < 0 || NS > DLSG_EXCL_SHARED || NC < 0 || NC > DLSG_EXCL_CLIP || (NS > 0 && !excl_shared) || (NC > 0 && !excl_clip)) return false;
    return NS + NC == 0 || (P >= 1 && P <= DLSG_PHRASE_MAX);
}

// Phase 0, the whole workgroup (one wave has fewer threads than there are entries): entry a from global memory, `shared` (NS, P)
// or `clip`, the clip's own (NC, P)
__device__ __forceinline__ void beam_stage_exclusions(const int64_t* __restrict__ shared, int NS, const int64_t* __restrict__ clip,
                                                      int NC, int P, int V, int* ex_s, int* n_s) {
    for (int a = threadIdx.x; a < NS + NC; a += blockDim.x) {
        const int64_t* e = a < NS ? shared + (int64_t)a * P : clip + (int64_t)(a - NS) * P;
        int n = 0;
        bool run = true;
        for (int j = 0; j < P; ++j) {
            const int64_t id = e[j];
            run = run && id >= 0 && id < V;
            ex_s[a * P + j] = run ? (int)id : -1;
            n += run;
        }
        n_s[a] = n;
    }
}

// The bans of the exclusions, ONE wave, appended to the list beam_ban_list has made (ban[0 .. *nban)): lane i of a round tests entry
// a = 64 * round + i -- n - 1 <= t and hist[t - n + 1 .. t - 1] == ex[a][0 .. n - 2], which a one-word entry meets at every step --
// and the entries that match put their last word behind the list, in entry order.  A word can stand in the list twice.
__device__ __forceinline__ void beam_ban_exclusions(const int* hist, int t, const int* ex_s, const int* n_s, int NE, int P, int* ban,
                                                    int* nban) {
    const int lane = threadIdx.x & 63;
    __builtin_amdgcn_wave_barrier();                           // (lane 0 of this wave has just stored the count)
    int cnt = *nban;
    for (int a0 = 0; a0 < NE; a0 += 64) {
        const int a = a0 + lane;
        const int n = a < NE ? n_s[a] : 0;
        bool hit = n > 0 && n - 1 <= t;
        for (int j = 0; j < P - 1; ++j) hit = hit && (j >= n - 1 || hist[t - n + 1 + j] == ex_s[a * P + j]);
        const unsigned long long m = __ballot(hit);
        if (hit) ban[cnt + __popcll(m & ((1ull << lane) - 1ull))] = ex_s[a * P + n - 1];
        cnt += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) *nban = cnt;
}

// A ban list by residue, ONE wave.  The row's wave gives lane l the classes l, l + 64, ... (beam_row_topk, beam_ens_row_topk), so
// a lane needs only the banned classes congruent to it: ban[0 .. n) is copied into `sorted` as a counting sort by class & 63 -- lane
// i of a round holds entry 64 * round + i, six ballots over the bits of its residue tell every lane which entries of the round share
// a residue -- and lane l gets its own stretch sorted[off .. off + cnt).  A lane scans its stretch, typically none or one class,
// where it would scan all n.
__device__ __forceinline__ void beam_ban_buckets(const int* ban, int n, int* sorted, int& off, int& cnt) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the entries (lanes) of a round whose residue is `want`
    auto same = [](const unsigned long long* bit, unsigned long long valid, int want) {
        unsigned long long m = valid;
#pragma unroll
        for (int b = 0; b < 6; ++b) m &= ((want >> b) & 1) ? bit[b] : ~bit[b];
        return m;
    };
    __builtin_amdgcn_wave_barrier();                           // (the list was stored by lanes of this wave)
    n = __builtin_amdgcn_readfirstlane(n);
    cnt = 0;
    for (int a0 = 0; a0 < n; a0 += 64) {
        const bool have = a0 + lane < n;
        const int r = have ? ban[a0 + lane] & 63 : 0;
        unsigned long long bit[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) bit[b] = __ballot(have && ((r >> b) & 1));
        cnt += __popcll(same(bit, __ballot(have), lane));
    }
    int incl = cnt;                                            // the stretches lie in residue order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        incl += lane >= o ? up : 0;
    }
    off = incl - cnt;
    int fill = off;                                            // lane l: where the next class of residue l goes
    for (int a0 = 0; a0 < n; a0 += 64) {
        const bool have = a0 + lane < n;
        const int c = have ? ban[a0 + lane] : 0;
        const int r = c & 63;
        unsigned long long bit[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) bit[b] = __ballot(have && ((r >> b) & 1));
        const unsigned long long valid = __ballot(have);
        const int dst = __shfl(fill, r, 64) + __popcll(same(bit, valid, r) & below);
        if (have) sorted[dst] = c;
        fill += __popcll(same(bit, valid, lane));
    }
    __builtin_amdgcn_wave_barrier();
}

// beam_row_bans for the wider list (every wave calls it: two barriers, the first of which also ends phase 0).  tok: token `lane` of
// the row's history (-1 behind it), which goes into LDS whatever g is -- a context is matched against it; the caller loads it
// before it stages the tables, so that the two trips to memory overlap.  Then beam_ban_list and beam_ban_exclusions for a row that
// is `live`.  -> the list the calling lane scans and its length: the whole list while it is short, from BEAM_BUCKET_MIN classes on
// the lane's stretch of the list by residue (beam_ban_buckets into sorted[w]), which costs about as much as scanning two classes.
constexpr int BEAM_BUCKET_MIN = 3;
template <int K>
__device__ __forceinline__ const int* beam_row_bans_excl(int tok, int t, int g, int min_len, int end, bool live, const int* ex_s,
                                                         const int* n_s, int NE, int P, int (&hist)[K][BEAM_MAXL],
                                                         int (&ban)[K][BEAM_BAN_EXCL], int (&nban)[K], int (&sorted)[K][BEAM_BAN_EXCL],
                                                         int& cnt) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    hist[w][lane] = tok;
    const int* list = ban[w];
    cnt = 0;
    __syncthreads();
    if (live) {
        beam_ban_list(hist[w], t, g, min_len, end, ban[w], &nban[w]);
        beam_ban_exclusions(hist[w], t, ex_s, n_s, NE, P, ban[w], &nban[w]);
        __builtin_amdgcn_wave_barrier();
        cnt = nban[w];
        if (cnt >= BEAM_BUCKET_MIN) {
            int off;
            beam_ban_buckets(ban[w], cnt, sorted[w], off, cnt);
            list = sorted[w] + off;
        }
    }
    __syncthreads();
    return list;
}

}  // namespace dlsg

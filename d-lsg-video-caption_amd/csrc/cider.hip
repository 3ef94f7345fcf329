// Self-critical training's reward on the device (gfx950): CIDEr-D of caption rows given as vocabulary ids against the fixed
// corpus tables of scoring.DeviceCiderD, and the baseline / advantages that turn the rewards into the CrossEntropy's weights.
// Everything in float64 like the host scorer, every reduction in a fixed order: the same inputs give the same bits on every
// launch and on graph replay.
#include <math.h>

#include <mutex>

#include "common.hpp"
#include "dlsg.h"
#include "ngram.hpp"

using namespace dlsg;

namespace {

constexpr int CIDER_STAGE = 2048;       // reference entries staged in LDS per pass (16 KiB keys + 16 KiB weights)

// index of `key` in keys[0, n) (sorted ascending), -1 if absent; reads only inside [0, n)
__device__ __forceinline__ int64_t find_key(const uint64_t* keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && keys[lo] == key ? lo : -1;
}

// One workgroup per row.  The row front end (RowNgrams, ngram.hpp) gives lane i of wave k the order-(k + 1) n-gram at position
// i, its count, and whether it is kept (its first position); every kept n-gram weighs in the norm, one with a word outside the
// vocabulary is looked up nowhere.  Per reference of the row's clip each kept n-gram
// looks itself up in the reference's sorted entries (staged in LDS) and adds min(w_h, w_r) w_r, divided by the two norms when
// both are nonzero, times the length penalty.  The n per-order sums are added in order by one thread.
__global__ __launch_bounds__(NGRAM_THREADS) void cider_d_kernel(const int64_t* __restrict__ ids, int64_t ld, int L,
                                                                const int32_t* __restrict__ clip_idx, int64_t end_id,
                                                                const dlsg_cider_tables t, double* __restrict__ scores) {
    __shared__ uint64_t skey[CIDER_STAGE];
    __shared__ double sw[CIDER_STAGE];
    __shared__ double stot[4];
    const int row = blockIdx.x;
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int n = t.n;
    const int c = clip_idx[row];
    const int64_t rb = (c >= 0 && c < t.n_clips) ? t.clip_off[c] : 0;
    const int64_t re = (c >= 0 && c < t.n_clips) ? t.clip_off[c + 1] : 0;
    if (re <= rb) {                                           // the same for the whole workgroup: no barrier is skipped by some
        if (threadIdx.x == 0) scores[row] = NAN;
        return;
    }
    const int64_t id = lane < L ? ids[(int64_t)row * ld + lane] : end_id;
    const RowNgrams g(id, L, end_id, t.vocab, lane, k);
    const int len = g.len, tf = g.tf;
    const uint64_t key = g.key;
    const bool live = k < n;                                  // wave-uniform
    const bool first = live && g.first;
    const bool look = first && !g.kbad;                       // a key with a bad word may alias a shorter n-gram's: no lookups
    double idf = t.log_n;                                     // not in the corpus: df = 0, max(1, df) = 1
    if (look && t.n_grams > 0) {
        const int64_t p = find_key(t.gram_keys, t.n_grams, key);
        if (p >= 0) idf = t.gram_idf[p];
    }
    const double wh = first ? (double)tf * idf : 0.0;
    const double nh = sqrt(wave_sum_f64(wh * wh));
    const int lh = n >= 2 ? (len > 0 ? len - 1 : 0) : 0;     // the reference scorer's "length": the bigram count
    const double two_s2 = 2.0 * (t.sigma * t.sigma);

    double acc = 0.0;
    for (int64_t r = rb; r < re;) {
        // as many whole references as fit in LDS; one that does not fit alone is searched in HBM
        const int64_t e0 = t.ref_off[r];
        int64_t r1 = r + 1;
        while (r1 < re && t.ref_off[r1 + 1] - e0 <= CIDER_STAGE) ++r1;
        const int64_t cnt = t.ref_off[r1] - e0;
        const bool staged = cnt <= CIDER_STAGE;
        if (staged) {
            for (int64_t i = threadIdx.x; i < cnt; i += NGRAM_THREADS) {
                skey[i] = t.ent_keys[e0 + i];
                sw[i] = t.ent_w[e0 + i];
            }
        }
        __syncthreads();
        if (live) {
            for (int64_t q = r; q < r1; ++q) {
                const int64_t a = t.ref_off[q], m = t.ref_off[q + 1] - a;
                const double nr = t.ref_norm[4 * q + k];
                const double d = (double)(lh - t.ref_len[q]);
                const double pen = exp(-(d * d) / two_s2);
                double cq = 0.0;
                if (look) {
                    double wr = 0.0;
                    if (staged) {
                        const int64_t p = find_key(skey + (a - e0), m, key);
                        if (p >= 0) wr = sw[a - e0 + p];
                    } else {
                        const int64_t p = find_key(t.ent_keys + a, m, key);
                        if (p >= 0) wr = t.ent_w[a + p];
                    }
                    cq = fmin(wh, wr) * wr;
                }
                if (nh != 0.0 && nr != 0.0) cq /= nh * nr;
                acc += cq * pen;
            }
        }
        __syncthreads();
        r = r1;
    }
    const double tot = wave_sum_f64(acc);
    if (lane == 0 && live) stot[k] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int kk = 0; kk < n; ++kk) s += stot[kk];
        scores[row] = s / (double)n / (double)(re - rb) * 10.0;
    }
}

// One workgroup of 256: thread-strided rows, then wave and workgroup sums in a fixed order.
__global__ __launch_bounds__(256) void scst_advantage_kernel(const double* __restrict__ r, const int64_t* __restrict__ lens,
                                                             const double* __restrict__ greedy, int B, int n,
                                                             float* __restrict__ adv, double* __restrict__ stats) {
    __shared__ double red[3][4];
    const int N = B * n;
    double sr = 0.0, sb = 0.0, sl = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const int b = i / n;
        double base;
        if (greedy) {
            base = greedy[b];
        } else {
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += r[b * n + j];
            base = (s - r[i]) / (double)(n - 1);
        }
        adv[i] = (float)(r[i] - base);
        sr += r[i];
        sb += base;
        sl += (double)lens[i];
    }
    block256_put(sr, red[0]);
    block256_put(sb, red[1]);
    block256_put(sl, red[2]);
    __syncthreads();
    if (threadIdx.x < 3) stats[threadIdx.x] = block256_get(red[threadIdx.x]) / (double)N;
}

// find_key for NQ keys in lockstep (n >= 1): the halving lower bound probes at a sequence of lengths that is the same for every
// key, so the NQ loads of a step do not depend on one another and are in flight together; reads only inside [0, n)
template <int NQ>
__device__ __forceinline__ void find_keys(const uint64_t* keys, int64_t n, const uint64_t (&key)[NQ], int64_t (&pos)[NQ]) {
    int64_t base[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) base[q] = 0;
    for (int64_t len = n; len > 1;) {
        const int64_t half = len >> 1;
#pragma unroll
        for (int q = 0; q < NQ; ++q) base[q] += keys[base[q] + half] < key[q] ? half : 0;
        len -= half;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int64_t p = base[q] + (keys[base[q]] < key[q] ? 1 : 0);
        pos[q] = p < n && keys[p] == key[q] ? p : -1;
    }
}

constexpr int CONS_MAXN = 32;           // candidates per clip: 32 x 4 orders x 64 positions x 16 B = 128 KiB of staged vectors

// dynamic LDS of cider_consensus_kernel for n candidates: keys and weights [n][4][64], norms and per-order sums [n][4], weight,
// utility row and expected utility [n], length [n]; every carve offset is a multiple of 8, the total of 16
constexpr int cons_lds_bytes(int n) { return (n * (4 * NGRAM_MAXL * 16 + 4 * 8 * 2 + 3 * 8 + 4) + 15) & ~15; }

// One workgroup per clip, its n candidates' tf-idf vectors staged in LDS.
// Phase A, per candidate: the row front end (RowNgrams, ngram.hpp), then the candidate's (key, count) entries, one per position
// (0 away from a first position), and its length go to LDS; the counts become weights by a bisection for the idf in the corpus
// table, the entries dealt over all threads; wave k sums the candidates' order-(k + 1) norms.  A word outside the vocabulary
// MATCHES itself here (within the candidate and across candidates, keys being compared within one order only): a `kbad` key
// keeps its entry and only its corpus lookup is left out.
// Phase B, per ordered pair (i, j): the lane holding position p of i scans j's entries of its order (one LDS read per lane, then
// at most 64 lane reads) for its key; min(w_i, w_j) w_j is summed over the wave by a butterfly; thread j folds the orders
// (norms, length penalty, x10 / n) into U[i][j]; thread 0 forms i's expected utility over j != i in index order.  Ranks are
// counted at the end.
__global__ __launch_bounds__(NGRAM_THREADS) void cider_consensus_kernel(const int64_t* __restrict__ ids, int64_t ld, int n, int L,
                                                                        int64_t end_id, const dlsg_cider_tables t,
                                                                        const float* __restrict__ scores, double temperature,
                                                                        double* __restrict__ util, double* __restrict__ expected,
                                                                        int64_t* __restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) char cons_smem[];
    uint64_t* skey = reinterpret_cast<uint64_t*>(cons_smem);
    double* sw = reinterpret_cast<double*>(skey + n * 4 * NGRAM_MAXL);
    double* snorm = sw + n * 4 * NGRAM_MAXL;
    double* stot = snorm + n * 4;
    double* sq = stot + n * 4;                                // weight of a candidate; -1: invalid
    double* surow = sq + n;
    double* sexp = surow + n;
    int* slen = reinterpret_cast<int*>(sexp + n);
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int no = t.n;
    const bool live = k < no;                                 // wave-uniform

    int64_t next = lane < L ? ids[(int64_t)b * n * ld + lane] : end_id;
    for (int c = 0; c < n; ++c) {
        const int64_t id = next;                              // (the next candidate's words are on their way meanwhile)
        if (c + 1 < n && lane < L) next = ids[((int64_t)b * n + c + 1) * ld + lane];
        const RowNgrams g(id, L, end_id, t.vocab, lane, k);
        if (live) {                                           // the count for now; negative: no corpus lookup for this key
            skey[(c * 4 + k) * NGRAM_MAXL + lane] = g.key;
            sw[(c * 4 + k) * NGRAM_MAXL + lane] = g.first ? (g.kbad ? -(double)g.tf : (double)g.tf) : 0.0;
        }
        if (threadIdx.x == 0) slen[c] = g.len;
    }
    __syncthreads();
    // The idf lookups, dealt round-robin over the 256 threads, four to a thread at a time: captions are short, so a
    // lane-per-position bisection per candidate would leave most lanes idle through n dependent chains of global loads; over the
    // (candidate, order, position < longest caption) entries they are a few rounds.
    int maxlen = 0;
    for (int c = 0; c < n; ++c) maxlen = max(maxlen, slen[c]);
    const int total = n * no * maxlen;
    for (int e0 = threadIdx.x; e0 < total; e0 += 4 * NGRAM_THREADS) {
        int at[4];
        double tf[4];
        uint64_t key[4];
        int64_t pos[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = e0 + q * NGRAM_THREADS;
            at[q] = 0;
            tf[q] = 0.0;
            if (e < total) {
                const int c = e / (no * maxlen), r = e - c * (no * maxlen);
                at[q] = (c * 4 + r / maxlen) * NGRAM_MAXL + r % maxlen;
                tf[q] = sw[at[q]];
            }
            key[q] = skey[at[q]];
            pos[q] = -1;
        }
        if (t.n_grams > 0) find_keys<4>(t.gram_keys, t.n_grams, key, pos);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (tf[q] == 0.0) continue;
            double idf = t.log_n;                             // not in the corpus, or with the outside word: df = 0
            if (tf[q] > 0.0 && pos[q] >= 0) idf = t.gram_idf[pos[q]];
            sw[at[q]] = fabs(tf[q]) * idf;
        }
    }
    __syncthreads();
    if (live) {
        for (int c = 0; c < n; ++c) {
            const double wh = sw[(c * 4 + k) * NGRAM_MAXL + lane];
            const double nh = sqrt(wave_sum_f64(wh * wh));
            if (lane == 0) snorm[c * 4 + k] = nh;
        }
    }
    if (threadIdx.x < n) {
        double q = 1.0;
        if (scores) {
            const float* s = scores + (int64_t)b * n;
            float mx = -INFINITY;
            for (int j = 0; j < n; ++j)
                if (s[j] > -INFINITY) mx = fmaxf(mx, s[j]);   // (a NaN fails the comparison)
            const float sc = s[threadIdx.x];
            if (!(sc > -INFINITY)) q = -1.0;
            else if (sc == mx || isinf(temperature)) q = 1.0;
            else q = exp(((double)sc - (double)mx) / temperature);
        }
        sq[threadIdx.x] = q;
    }
    __syncthreads();

    const double two_s2 = 2.0 * (t.sigma * t.sigma);
    for (int i = 0; i < n; ++i) {
        if (live) {
            const uint64_t key = skey[(i * 4 + k) * NGRAM_MAXL + lane];
            const double wh = sw[(i * 4 + k) * NGRAM_MAXL + lane];
            for (int j = 0; j < n; ++j) {
                const int m = __builtin_amdgcn_readfirstlane(slen[j]) - k;     // j's entries of this order: wave-uniform
                const uint64_t kj = skey[(j * 4 + k) * NGRAM_MAXL + lane];     // lane p holds j's entry p; those below m are read
                const double wj = sw[(j * 4 + k) * NGRAM_MAXL + lane];
                double wr = 0.0;                              // at most one match has a nonzero weight: the sum is exact
                for (int p = 0; p < m; ++p) {
                    const double wp = lane_f64(wj, p);
                    wr += lane_u64(kj, p) == key ? wp : 0.0;
                }
                const double tot = wave_sum_f64(fmin(wh, wr) * wr);
                if (lane == 0) stot[j * 4 + k] = tot;
            }
        }
        __syncthreads();
        if (threadIdx.x < n) {
            const int j = threadIdx.x;
            const int li = no >= 2 ? (slen[i] > 0 ? slen[i] - 1 : 0) : 0;      // the scorer's "length": the bigram count
            const int lj = no >= 2 ? (slen[j] > 0 ? slen[j] - 1 : 0) : 0;
            const double d = (double)(li - lj);
            const double pen = exp(-(d * d) / two_s2);
            double s = 0.0;
            for (int kk = 0; kk < no; ++kk) {
                double v = stot[j * 4 + kk];
                const double ni = snorm[i * 4 + kk], nj = snorm[j * 4 + kk];
                if (ni != 0.0 && nj != 0.0) v /= ni * nj;
                s += v * pen;
            }
            const double u = s / (double)no * 10.0;
            surow[j] = u;
            if (util) util[((int64_t)b * n + i) * n + j] = u;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double e = -INFINITY;
            if (sq[i] >= 0.0) {
                double num = 0.0, den = 0.0;
                for (int j = 0; j < n; ++j) {
                    if (j == i || !(sq[j] > 0.0)) continue;
                    num += sq[j] * surow[j];
                    den += sq[j];
                }
                e = den > 0.0 ? num / den : 0.0;
            }
            sexp[i] = e;
        }
    }
    __syncthreads();
    if (threadIdx.x < n) {
        const int i = threadIdx.x;
        const double e = sexp[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += sexp[j] > e || (sexp[j] == e && j < i);
        expected[(int64_t)b * n + i] = e;
        order[(int64_t)b * n + rank] = i;
    }
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

// the tables every CIDEr-D kernel reads: the orders, the vocabulary and the corpus n-grams; need_refs: the references as well
static bool cider_tables_ok(const dlsg_cider_tables* t, bool need_refs) {
    if (!t || t->n < 1 || t->n > 4 || t->vocab < 1 || t->vocab > 65535 || t->n_grams < 0) return false;
    if (t->n_grams > 0 && (!t->gram_keys || !t->gram_idf)) return false;
    if (!need_refs) return true;
    return t->n_clips >= 0 && !(t->n_clips > 0 && (!t->clip_off || !t->ref_off || !t->ref_norm || !t->ref_len));
}

extern "C" int dlsg_cider_d(const int64_t* ids, int64_t ld, int rows, int L, const int32_t* clip_idx, int64_t end_id,
                            const dlsg_cider_tables* t, double* scores, void* stream) {
    if (rows == 0) return DLSG_OK;
    if (!ids || !clip_idx || !scores || rows < 0 || L < 0 || L > NGRAM_MAXL || (L > 0 && ld < L)) return DLSG_EINVAL;
    if (!cider_tables_ok(t, true)) return DLSG_EINVAL;
    hipLaunchKernelGGL(cider_d_kernel, dim3(rows), dim3(NGRAM_THREADS), 0, ST(stream), ids, ld, L, clip_idx, end_id, *t, scores);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_scst_advantage(const double* rewards, const int64_t* lens, const double* greedy, int B, int n, float* adv,
                                   double* stats, void* stream) {
    if (B < 0 || n < 1 || (!greedy && n < 2) || !rewards || !lens || !adv || !stats) return DLSG_EINVAL;
    if (B == 0) return DLSG_OK;
    hipLaunchKernelGGL(scst_advantage_kernel, dim3(1), dim3(256), 0, ST(stream), rewards, lens, greedy, B, n, adv, stats);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_cider_consensus(const int64_t* ids, int64_t ld, int B, int n, int L, int64_t end_id, const dlsg_cider_tables* t,
                                    const float* scores, double temperature, double* util, double* expected, int64_t* order,
                                    void* stream) {
    if (n < 1 || n > CONS_MAXN || L < 1 || L > NGRAM_MAXL || B < 0) return DLSG_EINVAL;
    if (B == 0) return DLSG_OK;
    if (!ids || !expected || !order || ld < L || !(temperature > 0.0) || !cider_tables_ok(t, false)) return DLSG_EINVAL;
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(cider_consensus_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   cons_lds_bytes(CONS_MAXN));
    });
    if (attr != hipSuccess) return DLSG_ELAUNCH;
    hipLaunchKernelGGL(cider_consensus_kernel, dim3(B), dim3(NGRAM_THREADS), cons_lds_bytes(n), ST(stream), ids, ld, n, L, end_id, *t,
                       scores, temperature, util, expected, order);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

// Minimum-risk training over a candidate list (gfx950): the expected reward under the model renormalised over each clip's n
// candidates (dlsg_risk_rows, dlsg_risk_grad; include/addons/dlsg_risk.h states the arithmetic).  Rows, layout and the ragged rule
// are ce_ragged_kernel's (rowops.hip).  No atomics, every reduction in a fixed order: the same inputs give the same bits on every
// launch and on graph replay.
//
// Bytes per counted row of V floats: risk_rows reads it (the second pass over a row of a few tens of KB is served by the L2),
// risk_grad reads it once and writes the gradient row once; a row behind its caption's end, and a row whose weight c is exactly 0
// (a masked candidate, a clip without a valid candidate, n = 1, alpha = 0), is a plain zero fill that reads nothing.
#include <math.h>

#include "addons/dlsg_risk.h"
#include "common.hpp"

namespace {
using dlsg::block_max;
using dlsg::block_sum;
using dlsg::block256_get;
using dlsg::block256_put;
using dlsg::wave_sum_xor;

constexpr int RISK_MAXN = 32, RISK_MAXL = 64;   // candidates per clip (one lane each), words per caption

// A row of V floats at x as |head scalars| 16-byte vectors |tail scalars|: head = the elements in front of the first 16-byte
// boundary (all V when `other`, the row written beside it, is misaligned differently: then there is no common vector body)
struct RowSplit { int head, nvec, tail0; };
__device__ __forceinline__ RowSplit split_row(const void* x, const void* other, int V) {
    const int mx = (int)(((uintptr_t)x >> 2) & 3), mo = (int)(((uintptr_t)other >> 2) & 3);
    RowSplit r;
    r.head = mx == mo ? min(V, (4 - mx) & 3) : V;
    r.nvec = (V - r.head) >> 2;
    r.tail0 = r.head + 4 * r.nvec;
    return r;
}

__device__ __forceinline__ void zero_row(float* dx, int V) {
    const RowSplit sp = split_row(dx, dx, V);
    f32x4* d4 = reinterpret_cast<f32x4*>(dx + sp.head);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int j = threadIdx.x; j < sp.head; j += 256) dx[j] = 0.f;
    for (int j = threadIdx.x; j < sp.nvec; j += 256) d4[j] = z;
    for (int j = sp.tail0 + threadIdx.x; j < V; j += 256) dx[j] = 0.f;
}

// caption row r and position t of logits row `row`; where (t, r) lives in lse / tok_lp (the logits' own row order)
__device__ __forceinline__ void row_of(int row, int rows, int L, int tm, int& r, int& t) {
    r = tm ? row % rows : row / L;
    t = tm ? row / rows : row % L;
}
__device__ __forceinline__ int64_t slot_of(int r, int t, int rows, int L, int tm) {
    return tm ? (int64_t)t * rows + r : (int64_t)r * L + t;
}

// lse[row] = log sum_j exp(x_j), tok_lp[row] = x[target] - lse; both 0 behind the caption's end, both NaN for a target outside [0, V)
__global__ __launch_bounds__(256) void risk_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                        const int64_t* __restrict__ lens, float* __restrict__ lse,
                                                        float* __restrict__ tok_lp, int rows, int L, int V, int tm) {
    __shared__ float red[16];
    const int row = blockIdx.x;
    int r, t;
    row_of(row, rows, L, tm, r, t);
    int64_t len = lens[r];
    if (len > L) len = L;
    if (t >= len) {
        if (threadIdx.x == 0) lse[row] = tok_lp[row] = 0.f;
        return;
    }
    const float* x = logits + (int64_t)row * V;
    const RowSplit sp = split_row(x, x, V);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + sp.head);
    float m = -INFINITY;
    for (int j = threadIdx.x; j < sp.head; j += 256) m = fmaxf(m, x[j]);
    for (int j = threadIdx.x; j < sp.nvec; j += 256) {
        const f32x4 v = x4[j];
        m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (int j = sp.tail0 + threadIdx.x; j < V; j += 256) m = fmaxf(m, x[j]);
    m = block_max(m, red);
    float s = 0.f;
    for (int j = threadIdx.x; j < sp.head; j += 256) s += __expf(x[j] - m);
    for (int j = threadIdx.x; j < sp.nvec; j += 256) {
        const f32x4 v = x4[j];
        s += (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m));
    }
    for (int j = sp.tail0 + threadIdx.x; j < V; j += 256) s += __expf(x[j] - m);
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        const int64_t tgt = targets[(int64_t)r * L + t];
        const bool bad = tgt < 0 || tgt >= V;       // no out-of-bounds read (ce_ragged_kernel's rule)
        const float l = logf(s) + m;
        lse[row] = bad ? NAN : l;
        tok_lp[row] = bad ? NAN : x[tgt] - l;
    }
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// One workgroup per logits row.  Wave 0 rebuilds the clip's distribution over its n candidates (lane i: candidate i; its token
// terms summed over t in float64, t ascending), every lane of it ends with the clip's R_b; the weight c of this row's candidate
// goes through LDS to the workgroup, which then streams the row once: dx = c * (exp(x - lse) - onehot).
__global__ __launch_bounds__(256) void risk_grad_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                        const int64_t* __restrict__ lens, const float* __restrict__ lse,
                                                        const float* __restrict__ tok_lp, const double* __restrict__ rewards,
                                                        const uint8_t* __restrict__ valid, float* __restrict__ dlogits,
                                                        double* __restrict__ Q, double* __restrict__ S, double* __restrict__ R,
                                                        int rows, int n, int L, int V, int tm, double alpha, double lp) {
    __shared__ float c_s;
    const int row = blockIdx.x;
    int r, t;
    row_of(row, rows, L, tm, r, t);
    float* dx = dlogits + (int64_t)row * V;
    int64_t len = lens[r];
    if (len > L) len = L;
    const bool first = t == 0 && r % n == 0;        // this workgroup also writes the clip's Q, s and R
    if (t >= len && !first) {
        zero_row(dx, V);
        return;
    }
    if (threadIdx.x < 64) {
        const int i = threadIdx.x, b = r / n, cr = b * n + i;
        const bool act = i < n;
        int64_t li = act ? lens[cr] : 0;
        if (li > L) li = L;
        double s = 0.0;
        for (int u = 0; u < (int)li; ++u) s += (double)tok_lp[slot_of(cr, u, rows, L, tm)];
        // counted: flagged valid, at least one word, a log-probability above -inf (a NaN stays in and reaches the loss)
        const bool v = act && li >= 1 && (!valid || valid[cr]) && s != -INFINITY;
        const double a = v ? alpha / pow((double)li, lp) : 0.0;
        const double z = v ? a * s : -INFINITY;
        const double m = wave_max_f64(z);
        const double e = v ? exp(z - m) : 0.0;
        const double Z = wave_sum_xor(e);
        const double q = v ? e / Z : 0.0;
        const double rew = v ? rewards[cr] : 0.0;
        const double Rb = wave_sum_xor(q * rew);
        const double c = v ? a * q * (rew - Rb) / (double)(rows / n) : 0.0;
        if (i == r % n) c_s = (float)c;
        if (first) {
            if (act) { Q[cr] = q; S[cr] = s; }
            if (i == 0) R[b] = Rb;
        }
    }
    __syncthreads();
    const float c = c_s;
    if (t >= len || c == 0.f) {
        zero_row(dx, V);
        return;
    }
    const float* x = logits + (int64_t)row * V;
    const float l = lse[row];
    const int64_t tgt = targets[(int64_t)r * L + t];
    const RowSplit sp = split_row(x, dx, V);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + sp.head);
    f32x4* d4 = reinterpret_cast<f32x4*>(dx + sp.head);
    for (int j = threadIdx.x; j < sp.head; j += 256) dx[j] = c * (__expf(x[j] - l) - (j == tgt ? 1.f : 0.f));
    for (int j = threadIdx.x; j < sp.nvec; j += 256) {
        const f32x4 v = x4[j];
        const int64_t j0 = sp.head + 4 * (int64_t)j;
        f32x4 o;
        o.x = c * (__expf(v.x - l) - (j0 == tgt ? 1.f : 0.f));
        o.y = c * (__expf(v.y - l) - (j0 + 1 == tgt ? 1.f : 0.f));
        o.z = c * (__expf(v.z - l) - (j0 + 2 == tgt ? 1.f : 0.f));
        o.w = c * (__expf(v.w - l) - (j0 + 3 == tgt ? 1.f : 0.f));
        d4[j] = o;                                  // (a plain store: the backward GEMMs read dlogits next)
    }
    for (int j = sp.tail0 + threadIdx.x; j < V; j += 256) dx[j] = c * (__expf(x[j] - l) - (j == tgt ? 1.f : 0.f));
}

// One workgroup of 256, in scst_advantage_kernel's style: stats = {loss = -mean_b R_b, mean reward and mean length over the
// counted candidates (0 without one), mean_b R_b}; loss32 = (float)loss
__global__ __launch_bounds__(256) void risk_reduce_kernel(const double* __restrict__ rewards, const uint8_t* __restrict__ valid,
                                                          const int64_t* __restrict__ lens, const double* __restrict__ S,
                                                          const double* __restrict__ R, int rows, int n, int L,
                                                          float* __restrict__ loss32, double* __restrict__ stats) {
    __shared__ double red[4][4];
    const int B = rows / n;
    double sr = 0.0, sl = 0.0, sR = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < rows; i += 256) {
        const int64_t li = lens[i] > L ? L : lens[i];
        if (li >= 1 && (!valid || valid[i]) && S[i] != -INFINITY) {
            sr += rewards[i];
            sl += (double)li;
            cnt += 1.0;
        }
    }
    for (int b = threadIdx.x; b < B; b += 256) sR += R[b];
    block256_put(sr, red[0]);
    block256_put(sl, red[1]);
    block256_put(sR, red[2]);
    block256_put(cnt, red[3]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double N = block256_get(red[3]), ER = block256_get(red[2]) / (double)B;
        stats[0] = -ER;
        stats[1] = N > 0.0 ? block256_get(red[0]) / N : 0.0;
        stats[2] = N > 0.0 ? block256_get(red[1]) / N : 0.0;
        stats[3] = ER;
        loss32[0] = (float)-ER;
    }
}

bool shape_ok(int rows, int n, int L, int V) {
    return rows >= 0 && L >= 0 && L <= RISK_MAXL && n >= 1 && n <= RISK_MAXN && rows % n == 0 && V >= 1 &&
           (int64_t)rows * L <= 0x7fffffff;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dlsg_risk_rows(const float* logits, const int64_t* targets, const int64_t* lens, float* lse, float* tok_lp, int rows,
                              int n, int L, int V, int time_major, void* stream) {
    if (!shape_ok(rows, n, L, V)) return DLSG_EINVAL;
    if (rows * L == 0) return DLSG_OK;
    if (!logits || !targets || !lens || !lse || !tok_lp) return DLSG_EINVAL;
    hipLaunchKernelGGL(risk_rows_kernel, dim3(rows * L), dim3(256), 0, ST(stream), logits, targets, lens, lse, tok_lp, rows, L, V,
                       time_major);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_risk_grad(const float* logits, const int64_t* targets, const int64_t* lens, const float* lse, const float* tok_lp,
                              const double* rewards, const void* valid, float* dlogits, double* Q, double* s, double* R, float* loss,
                              double* stats, int rows, int n, int L, int V, int time_major, double alpha, double length_penalty,
                              void* stream) {
    if (!shape_ok(rows, n, L, V) || !(alpha >= 0.0) || isinf(alpha) || !isfinite(length_penalty)) return DLSG_EINVAL;
    if (rows * L == 0) return DLSG_OK;
    if (!logits || !targets || !lens || !lse || !tok_lp || !rewards || !dlogits || !Q || !s || !R || !loss || !stats) return DLSG_EINVAL;
    const uint8_t* v = static_cast<const uint8_t*>(valid);
    hipLaunchKernelGGL(risk_grad_kernel, dim3(rows * L), dim3(256), 0, ST(stream), logits, targets, lens, lse, tok_lp, rewards, v,
                       dlogits, Q, s, R, rows, n, L, V, time_major, alpha, length_penalty);
    hipLaunchKernelGGL(risk_reduce_kernel, dim3(1), dim3(256), 0, ST(stream), rewards, v, lens, s, R, rows, n, L, loss, stats);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

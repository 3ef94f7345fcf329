// Ragged CrossEntropy against a soft target row (gfx950): label smoothing and word-level distillation of an ensemble
// (dlsg_ce_ragged_soft).  Rows, layout and the ragged rule are ce_ragged_kernel's (rowops.hip); the target row is
//   r = (1 - alpha) * ((1 - eps) * onehot(tgt) + eps / V) + alpha * q,
// q the teachers' combined word distribution.  One workgroup per row, no atomics, every reduction in a fixed order: the same
// inputs give the same bits on every launch and on graph replay.
#include <math.h>

#include "common.hpp"
#include "dlsg.h"

namespace {
using dlsg::block_max;
using dlsg::block_sum;

// two block-wide sums behind one pair of barriers, each in block_sum's order (`red` >= 32 floats)
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
    a = dlsg::wave_sum(a); b = dlsg::wave_sum(b);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) { red[w] = a; red[16 + w] = b; }
    __syncthreads();
    float ra = 0.f, rb = 0.f;
    for (int i = 0; i < nw; ++i) { ra += red[i]; rb += red[16 + i]; }
    a = ra; b = rb;
}

// the M teacher rows' bases, strides and normalised weights: by value in the argument block (a captured launch keeps them)
struct SoftPack {
    const float* x[DLSG_ENS_MAX];
    int64_t ld[DLSG_ENS_MAX];
    float w[DLSG_ENS_MAX];
    int M;
};

// MODE -1: no teacher (the teacher code is compiled out; the row is read three times and dlogits written once, as
// ce_ragged_kernel does).  MODE 0 ('prob'): q_j = sum_m w_m softmax(x_m)_j.  MODE 1 ('logprob'): q_j = exp(a_j) / Z with
// a_j = sum_m w_m (x_mj - lse_m), Z taken around the row maximum of a, so that members that disagree completely still give a
// distribution.  Per member the row is read for its maximum, for its exponential sum and in the closing pass; mode 1 reads
// it once more for (max a, Z), found in one pass by a running maximum per thread.
// row_loss holds three blocks of B*L floats: mixed loss, NLL of the targets, CrossEntropy against q -- each times weights[b] / ntot.
template <int MODE>
__global__ __launch_bounds__(256) void ce_soft_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                      const int64_t* __restrict__ lens, const float* __restrict__ weights,
                                                      float* __restrict__ dlogits, float* __restrict__ row_loss, const SoftPack e,
                                                      int B, int L, int V, int tm, float eps, float alpha) {
    __shared__ float red[32];
    __shared__ float mx_s[DLSG_ENS_MAX], sum_s[DLSG_ENS_MAX];   // (in LDS: the member loop that fills them is not unrolled)
    const int row = blockIdx.x, rows = B * L;
    const int b = tm ? row % B : row / L, t = tm ? row / B : row % L;
    const float* x = logits + (int64_t)row * V;
    float* dx = dlogits + (int64_t)row * V;
    int64_t len = lens[b];
    if (len > L) len = L;
    if (t >= len) {
        for (int j = threadIdx.x; j < V; j += blockDim.x) dx[j] = 0.f;
        if (threadIdx.x == 0) row_loss[row] = row_loss[rows + row] = row_loss[2 * rows + row] = 0.f;
        return;
    }
    int64_t ntot = 0;
    for (int i = 0; i < B; ++i) ntot += (lens[i] > L ? L : lens[i]);
    float m = -INFINITY;
    for (int j = threadIdx.x; j < V; j += blockDim.x) m = fmaxf(m, x[j]);
    m = block_max(m, red);
    float s = 0.f, sx = 0.f;
    for (int j = threadIdx.x; j < V; j += blockDim.x) {
        const float v = x[j];
        s += __expf(v - m);
        sx += v;
    }
    block_sum2(s, sx, red);                                 // (sx serves the eps term: it rides on the pass and on the barriers)
    const int64_t tgt = targets[(int64_t)b * L + t];
    // a target outside [0, V): no out-of-bounds read; the row's losses and its gradient are NaN (ce_ragged_kernel's rule)
    const bool bad = tgt < 0 || tgt >= V;
    const float inv = bad ? NAN : 1.f / s;
    float invn = 1.f / (float)ntot;
    if (weights) invn = weights[b] * invn;
    const float lse = logf(s) + m;
    const float nll = bad ? NAN : lse - x[tgt];
    // the hard part of the target row, h = (1 - eps) onehot + eps / V (torch's label_smoothing): sum_j h_j (lse - x_j)
    const float hard = eps != 0.f ? (1.f - eps) * nll + eps * (lse - sx / (float)V) : nll;
    const float on = (1.f - alpha) * (1.f - eps), off = (1.f - alpha) * eps / (float)V;      // r_j = off + [j == tgt] on + alpha q_j
    float kd = 0.f;
    if constexpr (MODE < 0) {
        for (int j = threadIdx.x; j < V; j += blockDim.x) {
            const float p = __expf(x[j] - m) * inv;
            dx[j] = (p - (j == tgt ? on + off : off)) * invn;
        }
    } else {
        for (int k = 0; k < e.M; ++k) {
            const float* y = e.x[k] + (int64_t)row * e.ld[k];
            float mk = -INFINITY;
            for (int j = threadIdx.x; j < V; j += blockDim.x) mk = fmaxf(mk, y[j]);
            mk = block_max(mk, red);
            float sk = 0.f;
            for (int j = threadIdx.x; j < V; j += blockDim.x) sk += __expf(y[j] - mk);
            sk = block_sum(sk, red);
            if (threadIdx.x == 0) { mx_s[k] = mk; sum_s[k] = sk; }
        }
        __syncthreads();
        // mode 0: q_j = sum_k c_k exp(y_kj - o_k), c_k = w_k / sum_k, o_k = max_k
        // mode 1: a_j = sum_k c_k (y_kj - o_k),     c_k = w_k,         o_k = lse_k
        const float* y[DLSG_ENS_MAX];
        float c[DLSG_ENS_MAX], o[DLSG_ENS_MAX];
#pragma unroll
        for (int k = 0; k < DLSG_ENS_MAX; ++k) {
            const bool on_k = k < e.M;
            y[k] = on_k ? e.x[k] + (int64_t)row * e.ld[k] : nullptr;
            c[k] = on_k ? (MODE == 0 ? e.w[k] / sum_s[k] : e.w[k]) : 0.f;
            o[k] = on_k ? (MODE == 0 ? mx_s[k] : logf(sum_s[k]) + mx_s[k]) : 0.f;
        }
        float amax = 0.f, invz = 1.f;
        if constexpr (MODE == 1) {
            float tmx = -INFINITY, ts = 0.f;
            for (int j = threadIdx.x; j < V; j += blockDim.x) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < DLSG_ENS_MAX; ++k)
                    if (k < e.M) a += c[k] * (y[k][j] - o[k]);
                const float nm = fmaxf(tmx, a);
                if (nm > -INFINITY) ts = ts * __expf(tmx - nm) + __expf(a - nm);
                tmx = nm;
            }
            amax = block_max(tmx, red);
            ts = tmx > -INFINITY ? ts * __expf(tmx - amax) : 0.f;
            invz = 1.f / block_sum(ts, red);
        }
        for (int j = threadIdx.x; j < V; j += blockDim.x) {
            const float v = x[j];
            const float p = __expf(v - m) * inv;
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < DLSG_ENS_MAX; ++k)
                if (k < e.M) q += MODE == 0 ? c[k] * __expf(y[k][j] - o[k]) : c[k] * (y[k][j] - o[k]);
            if constexpr (MODE == 1) q = __expf(q - amax) * invz;
            dx[j] = (p - ((j == tgt ? on + off : off) + alpha * q)) * invn;
            kd += q * (lse - v);
        }
        kd = block_sum(kd, red);
    }
    if (bad) kd = NAN;
    if (threadIdx.x == 0) {
        row_loss[row] = (MODE < 0 ? hard : (1.f - alpha) * hard + alpha * kd) * invn;
        row_loss[rows + row] = nll * invn;
        row_loss[2 * rows + row] = kd * invn;
    }
}

// out[i] = sum of v[i * n .. i * n + n), i = blockIdx.x, in sum_to_scalar_kernel's order
__global__ __launch_bounds__(256) void sum_blocks_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ float red[16];
    const float* src = v + (int64_t)blockIdx.x * n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += src[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dlsg_ce_ragged_soft(const float* logits, const int64_t* targets, const int64_t* lens, const float* weights,
                                   float* dlogits, float* row_loss, float* loss, int B, int L, int V, int time_major, float smoothing,
                                   float alpha, const float* const* teacher, const int64_t* teacher_ld, const float* w,
                                   const float* logw, int M, int mode, void* stream) {
    if (M < 0 || M > DLSG_ENS_MAX || (mode != 0 && mode != 1)) return DLSG_EINVAL;
    if (!(smoothing >= 0.f && smoothing < 1.f) || !(alpha >= 0.f && alpha <= 1.f)) return DLSG_EINVAL;
    if ((alpha > 0.f) != (M > 0)) return DLSG_EINVAL;
    if (M > 0 && (!teacher || !teacher_ld || !w || !logw)) return DLSG_EINVAL;
    SoftPack e = {};
    for (int k = 0; k < M; ++k) {
        if (!teacher[k]) return DLSG_EINVAL;
        e.x[k] = teacher[k]; e.ld[k] = teacher_ld[k]; e.w[k] = w[k];
    }
    e.M = M;
    if (B < 0 || L < 0) return DLSG_EINVAL;
    if (B * L == 0) return DLSG_OK;
    if (V < 1 || !logits || !targets || !lens || !dlogits || !row_loss || !loss) return DLSG_EINVAL;
#define SOFT_CE_LAUNCH(MODE)                                                                                                     \
    hipLaunchKernelGGL(ce_soft_kernel<MODE>, dim3(B * L), dim3(256), 0, ST(stream), logits, targets, lens, weights, dlogits, row_loss, \
                       e, B, L, V, time_major, smoothing, alpha)
    if (M == 0) SOFT_CE_LAUNCH(-1);
    else if (mode == 0) SOFT_CE_LAUNCH(0);
    else SOFT_CE_LAUNCH(1);
#undef SOFT_CE_LAUNCH
    hipLaunchKernelGGL(sum_blocks_kernel, dim3(3), dim3(256), 0, ST(stream), row_loss, B * L, loss);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

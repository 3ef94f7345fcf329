// The phases of choosing a word from a row of logits and writing its embedding (gfx950), one definition each.  The kernels of
// sample.hip (argmax, select_embed, sample_embed, sample_filter_embed) are compositions of them and embed_fwd_kernel (rowops.hip)
// calls the row writer, so greedy decoding, the plain and the filtered sampler agree on ties, on rows without a maximum, on the
// noise of a word and on the word-dropout stream because they run the same statements.  One workgroup of 256 (four waves) per row.
#pragma once
#include <math.h>

#include "common.hpp"

namespace dlsg {

// ------------------------------------------------------------------------------------------------ first maximum
// A thread's running (value, index) pair starts at (-inf, WP_NONE).  First maximum wins (torch.max / argmax tie rule on CPU and
// GPU for exact ties: lowest index); NaN never wins.
constexpr int WP_NONE = 0x7fffffff;

__device__ __forceinline__ void first_max_update(float& best, int& idx, float v, int j) {
    if (v > best || (v == best && j < idx)) { best = v; idx = j; }
}
// the wave's pair, to every lane
__device__ __forceinline__ void first_max_wave(float& best, int& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first_max_update(best, idx, __shfl_xor(best, o, 64), __shfl_xor(idx, o, 64));
}
// The workgroup's word from the four waves' pairs, to thread 0 only (every thread calls it: one barrier, which also publishes
// what the caller's lanes 0 wrote to LDS before the call).  No maximum (a row of NaN / -inf, nothing kept): word 0, as
// torch.argmax gives for -inf rows, not an out-of-range row of E.
__device__ __forceinline__ int first_max_block(float best, int idx, float (&bv)[4], int (&bi)[4]) {
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < 4; ++k) first_max_update(best, idx, bv[k], bi[k]);
    return idx == WP_NONE ? 0 : idx;
}
// a row's first maximum (thread 0 only): argmax_kernel's choice, and select_embed_kernel's at a step that is not teacher-forced
__device__ __forceinline__ int first_max_row(const float* __restrict__ x, int V, float (&bv)[4], int (&bi)[4]) {
    float best = -INFINITY;
    int idx = WP_NONE;
    for (int j = threadIdx.x; j < V; j += blockDim.x) first_max_update(best, idx, x[j], j);
    first_max_wave(best, idx);
    return first_max_block(best, idx, bv, bi);
}

// ------------------------------------------------------------------------------------------------ online log-sum-exp
// (m, s) = (max, sum of exp(z - max)) of the values seen; starts at (-inf, 0).  A -inf or NaN value adds nothing; FINITE: the
// caller shows finite values only and the test for it is compiled out (in the filtered sampler's loop, where most lanes skip
// their word, it cost 1.2 us of 51 at V = 10000).
template <bool FINITE>
__device__ __forceinline__ void lse_update(float& m, float& s, float z) {
    if (z > m) { s = s * __expf(m - z) + 1.f; m = z; }
    else if (FINITE || z > -INFINITY) s += __expf(z - m);
}
// (m, s) merged with (om, os); an empty side (max -inf) contributes nothing
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
    m = nm;
}

// ------------------------------------------------------------------------------------------------ the draw
// Gumbel-max key of a word with tempered logit z: z + g, g = -log(-log u), u from the counter hash keyed (seed, site, ctr) -- the
// same word whatever the reduction order (a replayed graph draws what the eager launch drew).  A -inf logit stays -inf: never drawn.
__device__ __forceinline__ float gumbel_key(float z, uint64_t seed, uint32_t site, uint64_t ctr) {
    // u = (hi + 1/2) 2^-24 in (0, 1).  hi + 1/2 needs 25 bits above 2^23: there -log u = -log1p(-(1 - u)) with
    // 1 - u = (2^24 - 1 - hi + 1/2) 2^-24 exact, so u never rounds to 1 and the noise stays finite
    const uint32_t hi = counter_hash(seed, site, ctr) >> 8;
    const float e = hi < (1u << 23) ? -logf(((float)hi + 0.5f) * (1.0f / 16777216.0f))
                                    : -log1pf(-((float)(0xFFFFFFu - hi) + 0.5f) * (1.0f / 16777216.0f));
    return z - logf(e);
}

// A sampled step's view of its row: id = argmax_j (x_j / tau + g_j) over the words it is shown, in one pass that also keeps the
// online max / sum-exp of x / tau for logp = log softmax(x / tau)[id].  tau == 0: no noise and sc = 1, first_max_row's choice
// and the log-prob of the untempered softmax.  The noise of word j is keyed (row0 + r) * V + j: it does not depend on which
// other words are shown, so the filtered sampler (which shows the kept words only) draws with the plain sampler's noise.
struct WordDraw {
    bool gumbel;
    float sc;
    uint64_t seed, key0;
    uint32_t site;
    float best = -INFINITY, m = -INFINITY, s = 0.f;          // this thread's pair and (max, sum-exp), then the wave's
    int idx = WP_NONE;

    __device__ __forceinline__ WordDraw(float tau, uint64_t seed_, uint32_t site_sample, int64_t row, int V)
        : gumbel(tau > 0.f), sc(gumbel ? 1.f / tau : 1.f), seed(seed_), key0((uint64_t)row * (uint64_t)V), site(site_sample) {}
    // one word of the row (FINITE: x_j / tau is known to be finite)
    template <bool FINITE>
    __device__ __forceinline__ void step(int j, float xj) {
        const float z = xj * sc;
        first_max_update(best, idx, gumbel ? gumbel_key(z, seed, site, key0 + j) : z, j);
        lse_update<FINITE>(m, s, z);
    }
    __device__ __forceinline__ void wave() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            first_max_update(best, idx, __shfl_xor(best, o, 64), __shfl_xor(idx, o, 64));
            lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
        }
    }
    // The row's word and (m, s), to thread 0 only (every thread calls it after wave(): first_max_block's one barrier).
    __device__ __forceinline__ int block(float (&bv)[4], int (&bi)[4], float (&bm)[4], float (&bs)[4]) {
        if ((threadIdx.x & 63) == 0) { bm[threadIdx.x >> 6] = m; bs[threadIdx.x >> 6] = s; }
        const int id = first_max_block(best, idx, bv, bi);
        if (threadIdx.x == 0)
            for (int k = 1; k < 4; ++k) lse_merge(m, s, bm[k], bs[k]);
        return id;
    }
    // Thread 0 commits the choice: the word, its log-prob (0 when `certain`: one word was left, probability 1 whatever x * sc
    // rounds to), and lens[r] (L on entry) becomes t + 1 at the row's first end_id.
    __device__ __forceinline__ void commit(int64_t id, const float* __restrict__ x, bool certain, int r, int64_t* __restrict__ ids_out,
                                           float* __restrict__ logp, int64_t* __restrict__ lens, int t, int64_t end_id) const {
        ids_out[r] = id;
        logp[r] = certain ? 0.f : x[id] * sc - m - logf(s);
        if (id == end_id && lens[r] > t) lens[r] = t + 1;
    }
};

// ------------------------------------------------------------------------------------------------ embedding row
// out[r, :W] = E[id, :] under the word-dropout stream (seed, site) of row row0 + r, by the whole workgroup, `threads` wide:
// blockDim.x (unsigned) or a constant (int), each in its own type, because the loop the compiler builds depends on it
template <class T>
__device__ __forceinline__ void embed_row(const float* __restrict__ E, int64_t id, float* __restrict__ out, int64_t ldo, int W, int r,
                                          float p, uint64_t seed, uint32_t site, int64_t row0, T threads) {
    for (int j = threadIdx.x; j < W; j += threads) {
        float v = E[id * W + j];
        if (p > 0.f) v *= drop_scale(seed, site, (uint64_t)(row0 + r) * W + j, p);
        out[(int64_t)r * ldo + j] = v;
    }
}

}  // namespace dlsg

// Caption metrics on the device (gfx950): sentence-level BLEU-1..4 and ROUGE_L of caption rows given as vocabulary ids against
// the reference words of scoring.DeviceCaptionMetrics, the integer statistics of corpus BLEU, and a weighted mix with CIDEr-D as
// the self-critical reward.  Float64 in the order of scoring.bleu / scoring.rouge_l, no atomics, every reduction in a fixed
// order: the same inputs give the same bits on every launch and on graph replay.
#include <math.h>

#include <type_traits>

#include "common.hpp"
#include "dlsg.h"
#include "ngram.hpp"

using namespace dlsg;

namespace {

constexpr int METRICS_STAGE = DLSG_METRICS_STAGE;   // reference words staged in LDS per pass
constexpr uint32_t REF_OOV = NGRAM_NONE;        // a reference word outside the vocabulary (no id reaches it: vocab <= 65535)
constexpr uint32_t HYP_BAD = 0x10000u;          // an id outside [0, vocab): no 16-bit reference word equals it

struct mix_weights {
    double w[6];                                // base (CIDEr-D), BLEU-1..4, ROUGE_L
};

// One workgroup per row.  The row front end (RowNgrams, ngram.hpp) gives lane i of wave k the order-(k + 1) n-gram at position
// i and its count in the row; it is kept at its first position, and not at all with a word outside the vocabulary.  The
// references of the row's clip pass through LDS in pieces of whole references (at most 63, at most METRICS_STAGE words; one
// longer than that is read from HBM).
// Per reference every wave takes the words 64 at a time into a register, slides its order's window over them and counts in
// each lane the windows equal to the lane's n-gram; the count joins the clip (the maximum over the references) and the
// reference's length joins the closest-length search.  Wave w also runs the bit-parallel LCS (Hyyro's form of
// Allison-Dix: bit i of V is clear where the LCS grows at hypothesis word i) of references w, w + 4, ...  The four waves'
// results meet in LDS and one thread does the float64 arithmetic of the host code.
__global__ __launch_bounds__(NGRAM_THREADS) void caption_metrics_kernel(
    const int64_t* __restrict__ ids, int64_t ld, int L, const int32_t* __restrict__ clip_idx, int64_t end_id,
    const int64_t* __restrict__ clip_off, const int64_t* __restrict__ ref_off, const uint16_t* __restrict__ ref_words, int n_clips,
    int vocab, const mix_weights mix, const double* __restrict__ base, double* __restrict__ scores, int32_t* __restrict__ stats,
    double* __restrict__ reward) {
#pragma clang fp contract(off)                                // the host's roundings: no fused multiply-add
    __shared__ uint16_t sref[METRICS_STAGE];
    __shared__ int scorrect[4];
    __shared__ double sprec[4], srec[4];
    const int row = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform, and known to the compiler as such
    const int c = clip_idx[row];
    const int64_t rb = (c >= 0 && c < n_clips) ? clip_off[c] : 0;
    const int64_t re = (c >= 0 && c < n_clips) ? clip_off[c + 1] : 0;
    if (re <= rb) {                                           // the same for the whole workgroup: no barrier is skipped by some
        if (scores && threadIdx.x < 5) scores[(int64_t)row * 5 + threadIdx.x] = NAN;
        if (stats && threadIdx.x < 10) stats[(int64_t)row * 10 + threadIdx.x] = 0;
        if (reward && threadIdx.x == 0) reward[row] = NAN;
        return;
    }
    const int64_t id = lane < L ? ids[(int64_t)row * ld + lane] : end_id;
    const RowNgrams g(id, L, end_id, vocab, lane, k);
    const int len = g.len, tf = g.tf;
    const uint64_t key = g.key;
    const bool first = g.first && !g.kbad;                    // an n-gram with a word outside the vocabulary matches no reference
    const uint32_t hcode = (g.bad || lane >= len) ? HYP_BAD : (uint32_t)id;
    const uint64_t past = k < 3 ? ~0ull << (16 * (k + 1)) : 0ull;       // the key slots past the order, all ones

    int clip = 0;                                             // max over the references of the n-gram's count there
    int best_d = 0x7fffffff, best_len = 0;                    // closest reference length, shorter on ties (wave-uniform)
    int prec_l = 0;                                           // this wave's best LCS (precision = LCS / len)
    int rec_l = 0, rec_m = 1;                                 // and its best recall LCS / m, kept as the fraction
    const uint64_t low = len >= 64 ? ~0ull : ((1ull << len) - 1ull);
    for (int64_t r = rb; r < re;) {
        // lane i holds the word offset of reference r + i: the piece is the run of whole references that fits the stage
        const int64_t qi = r + lane < re ? r + lane : re;
        const int64_t oi = ref_off[qi];
        const int64_t e0 = (int64_t)lane_u64((uint64_t)oi, 0);
        const unsigned long long fits = __ballot(lane >= 1 && r + lane <= re && oi >= e0 && oi - e0 <= METRICS_STAGE) | 1ull;
        int nr = ~fits ? __builtin_ctzll(~fits) - 1 : 63;
        const bool staged = nr > 0;
        if (!staged) nr = 1;                                  // one reference longer than the stage: its words stay in HBM
        const int64_t di = oi - e0;
        const int rel = di < 0 ? 0 : (di > 0x7fffffff ? 0x7fffffff : (int)di);    // where reference r + i starts in the piece
        const int cnt = __builtin_amdgcn_readlane(rel, nr);                       // the piece's words
        if (staged)
            for (int i = threadIdx.x; i < cnt; i += NGRAM_THREADS) sref[i] = ref_words[e0 + i];
        __syncthreads();
        // reference by reference, its words 64 at a time in a register: the window count in every wave, the LCS in one
        auto scan = [&](auto from_lds) {
            int end = 0;
            for (int i = 0; i < nr; ++i) {
                const int start = end;
                end = __builtin_amdgcn_readlane(rel, i + 1);
                const int m = end > start ? end - start : 0;
                const bool mine = ((r + i - rb) & 3) == k;
                uint64_t V = ~0ull, rk = ~0ull;               // rk: the last four words, all REF_OOV before the first
                int hits = 0;                                 // per lane: windows of this reference equal to the lane's n-gram
                for (int c0 = 0; c0 < m; c0 += 64) {
                    uint32_t wreg = REF_OOV;
                    if (c0 + lane < m) {
                        if constexpr (decltype(from_lds)::value) wreg = sref[start + c0 + lane];
                        else wreg = ref_words[e0 + start + c0 + lane];
                    }
                    const int nj = m - c0 < 64 ? m - c0 : 64;
                    for (int j = 0; j < nj; ++j) {
                        const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)wreg, j);
                        rk = (rk >> 16) | ((uint64_t)wj << 48);                   // the newest word on top
                        const uint64_t kr = (rk >> (16 * (3 - k))) | past;        // the window that ends here, as a key
                        hits += kr == key ? 1 : 0;
                    }
                    if (mine) {
                        for (int j = 0; j < nj; ++j) {
                            const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)wreg, j);
                            const uint64_t M = __ballot(hcode == wj);
                            const uint64_t U = V & M;
                            V = (V + U) | (V & ~M);
                        }
                    }
                }
                clip = hits > clip ? hits : clip;
                const int d = m > len ? m - len : len - m;
                if (d < best_d || (d == best_d && m < best_len)) {
                    best_d = d;
                    best_len = m;
                }
                if (mine && m > 0) {
                    const int lcs = __builtin_popcountll(~V & low);
                    prec_l = lcs > prec_l ? lcs : prec_l;
                    if ((int64_t)lcs * rec_m > (int64_t)rec_l * m) {
                        rec_l = lcs;
                        rec_m = m;
                    }
                }
            }
        };
        if (staged) scan(std::true_type());
        else scan(std::false_type());
        __syncthreads();
        r += nr;
    }
    // the maximum of the quotients is the quotient of the maximal fraction: division rounds monotonically
    const double prec = len > 0 ? (double)prec_l / (double)len : 0.0;
    const double rec = (double)rec_l / (double)rec_m;
    const int correct = wave_sum_xor(first ? (tf < clip ? tf : clip) : 0);
    if (lane == 0) {
        scorrect[k] = correct;
        sprec[k] = prec;
        srec[k] = rec;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double small = 1e-9, tiny = 1e-15;
        double s5[5];
        double b = 1.0;
        const double ratio = ((double)len + tiny) / ((double)best_len + small);
        for (int kk = 0; kk < 4; ++kk) {
            const int g = len > kk ? len - kk : 0;
            b *= ((double)scorrect[kk] + tiny) / ((double)g + small);
            const double s = pow(b, 1.0 / (double)(kk + 1));
            s5[kk] = ratio < 1.0 ? s * exp(1.0 - 1.0 / ratio) : s;
            if (stats) {
                stats[(int64_t)row * 10 + kk] = scorrect[kk];
                stats[(int64_t)row * 10 + 4 + kk] = g;
            }
        }
        const double p = fmax(fmax(sprec[0], sprec[1]), fmax(sprec[2], sprec[3]));
        const double q = fmax(fmax(srec[0], srec[1]), fmax(srec[2], srec[3]));
        const double beta2 = 1.2 * 1.2;
        s5[4] = (p != 0.0 && q != 0.0) ? (1.0 + beta2) * p * q / (q + beta2 * p) : 0.0;
        if (stats) {
            stats[(int64_t)row * 10 + 8] = len;
            stats[(int64_t)row * 10 + 9] = best_len;
        }
        if (scores)
            for (int j = 0; j < 5; ++j) scores[(int64_t)row * 5 + j] = s5[j];
        if (reward) {
            double acc = 0.0;
            if (mix.w[0] != 0.0) acc += mix.w[0] * base[row];
            for (int j = 0; j < 5; ++j)
                if (mix.w[j + 1] != 0.0) acc += mix.w[j + 1] * s5[j];
            reward[row] = acc;
        }
    }
}

// One workgroup of 256: thread-strided rows, then wave and workgroup sums in a fixed order.
__global__ __launch_bounds__(256) void caption_corpus_kernel(const int32_t* __restrict__ stats, const double* __restrict__ scores,
                                                             const double* __restrict__ base, int rows, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ long long ired[10][4];
    __shared__ double fred[2][4];
    long long s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double sr = 0.0, sb = 0.0;
    for (int i = threadIdx.x; i < rows; i += 256) {
#pragma unroll
        for (int j = 0; j < 10; ++j) s[j] += stats[(int64_t)i * 10 + j];
        sr += scores[(int64_t)i * 5 + 4];
        if (base) sb += base[i];
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) block256_put(s[j], ired[j]);
    block256_put(sr, fred[0]);
    block256_put(sb, fred[1]);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t[10];
        for (int j = 0; j < 10; ++j) t[j] = block256_get(ired[j]);
        const double small = 1e-9, tiny = 1e-15;
        const double ratio = ((double)t[8] + tiny) / ((double)t[9] + small);
        double b = 1.0;
        for (int kk = 0; kk < 4; ++kk) {
            b *= ((double)t[kk] + tiny) / ((double)t[4 + kk] + small);
            const double sk = pow(b, 1.0 / (double)(kk + 1));
            out[kk] = ratio < 1.0 ? sk * exp(1.0 - 1.0 / ratio) : sk;
        }
        out[4] = block256_get(fred[0]) / (double)rows;
        out[5] = base ? block256_get(fred[1]) / (double)rows : NAN;
    }
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dlsg_caption_metrics(const int64_t* ids, int64_t ld, int rows, int L, const int32_t* clip_idx, int64_t end_id,
                                    const int64_t* clip_off, const int64_t* ref_off, const uint16_t* ref_words, int n_clips, int vocab,
                                    const double* weights, const double* base, double* scores, int32_t* stats, double* reward,
                                    void* stream) {
    if (rows == 0) return DLSG_OK;
    if (!ids || !clip_idx || rows < 0 || L < 0 || L > NGRAM_MAXL || (L > 0 && ld < L)) return DLSG_EINVAL;
    if (vocab < 1 || vocab > 65535 || n_clips < 0) return DLSG_EINVAL;
    if (n_clips > 0 && (!clip_off || !ref_off || !ref_words)) return DLSG_EINVAL;
    if (reward && (!weights || (weights[0] != 0.0 && !base))) return DLSG_EINVAL;
    mix_weights mix = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    if (reward)
        for (int j = 0; j < 6; ++j) mix.w[j] = weights[j];
    hipLaunchKernelGGL(caption_metrics_kernel, dim3(rows), dim3(NGRAM_THREADS), 0, ST(stream), ids, ld, L, clip_idx, end_id, clip_off,
                       ref_off, ref_words, n_clips, vocab, mix, base, scores, stats, reward);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

extern "C" int dlsg_caption_corpus(const int32_t* stats, const double* scores, const double* base, int rows, double* out,
                                   void* stream) {
    if (rows < 1 || !stats || !scores || !out) return DLSG_EINVAL;
    hipLaunchKernelGGL(caption_corpus_kernel, dim3(1), dim3(256), 0, ST(stream), stats, scores, base, rows, out);
    DLSG_CHECK_LAUNCH();
    return DLSG_OK;
}

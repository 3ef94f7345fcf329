// The row front end of the caption-metric kernels (cider_d_kernel, cider_consensus_kernel, caption_metrics_kernel): what a
// caption row's words are, what an id outside the vocabulary means and where an n-gram is counted, once.  Integer work only.
#pragma once
#include "common.hpp"

namespace dlsg {

constexpr int NGRAM_THREADS = 256;          // wave k holds the n-grams of order k + 1: n <= 4
constexpr int NGRAM_MAXL = 64;              // lane i holds word position i
constexpr uint32_t NGRAM_NONE = 0xFFFFu;    // "no word": a key slot past the order, and an id outside [0, vocab) (vocab <= 65535)

// Lane i of every wave holds word i of one row: `id` = the row's id at position `lane`, end_id at and past L (the caller loads
// it, so it may load the next row's early).  The row's words (decode_tokens) are those before the first end_id, all L without
// one.  Wave k packs the order-(k + 1) n-gram that starts at its position into a 64-bit key, 16 bits a word; a word outside the
// vocabulary keeps NGRAM_NONE in a used slot, so equal keys within one order still mean equal word sequences, but such a key
// may equal a shorter n-gram's: `kbad` says so and the caller looks it up nowhere.  The row has max(len - k, 0) n-grams of the
// order; `tf` counts the lane's key among them and `first` holds at a key's first position, whatever `kbad` is.
struct RowNgrams {
    int len;            // words in the row (wave-uniform)
    bool bad;           // this lane's id is outside [0, vocab): matches nothing, never indexes a table
    uint32_t w;         // the word's 16-bit code
    uint64_t key;
    bool kbad;          // a used slot of the key holds a word outside the vocabulary
    int tf;
    bool first;

    __device__ __forceinline__ RowNgrams(int64_t id, int L, int64_t end_id, int vocab, int lane, int k) {
        const unsigned long long ends = __ballot(lane >= L || id == end_id);
        len = ends ? __builtin_ctzll(ends) : NGRAM_MAXL;
        bad = id < 0 || id >= vocab;
        w = bad ? NGRAM_NONE : (uint32_t)id;
        key = 0;
        kbad = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t wj = (uint32_t)__shfl((int)w, (lane + j) & 63, 64);
            const int bj = __shfl((int)bad, (lane + j) & 63, 64);
            const bool used = j <= k;
            key |= (uint64_t)(used ? wj : NGRAM_NONE) << (16 * j);
            kbad |= used && bj;
        }
        const int m = __builtin_amdgcn_readfirstlane(len > k ? len - k : 0);     // wave-uniform, and known to the compiler as such
        tf = 0;
        first = lane < m;
        for (int j = 0; j < m; ++j) {
            if (lane_u64(key, j) == key) {
                ++tf;
                if (j < lane) first = false;
            }
        }
    }
};

}  // namespace dlsg

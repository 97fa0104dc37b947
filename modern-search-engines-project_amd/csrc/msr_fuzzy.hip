// K15: typo-tolerant lookup (msr_bind_vocab / msr_fuzzy_terms; include/msretr.h).  The pieces K16
// (msr_wildcard.hip) uses too -- signature bit, 64-bit shuffles, keys, wave_first_keys, the slot store, the merge -- are in
// msr_vocabscan.h.
//
// For every word of a call: the vocabulary terms within its tolerance m <= 2 of it by optimal string alignment (insertion,
// deletion, substitution, swap of two adjacent code points; no substring edited twice), ordered by (distance, weight
// descending, term id), the first `limit` of them and the number of all.  Deterministic and free of atomics: two kernels.
//
// SCAN.  One workgroup owns FZ_SPAN consecutive terms, one lane per term: the lane keeps its term (<= 32 code points, two per
// register), its length, its weight and its 64-bit character-set signature for the whole kernel.  The call's words come
// through LDS FZ_G at a time (staged by the workgroup, their signatures computed while staging).  Per word a lane applies
//   the length test   |len_t - len_w| <= m, and
//   the signature test popcount(sig_w & ~sig_t) <= m and popcount(sig_t & ~sig_w) <= m
// (an edit adds at most one and removes at most one character of the set, a swap neither; hashing 65 535 code points into 64
// bits only merges characters, so the test only passes more: lossless), and only the survivors run the distance: a banded
// dynamic programme over the 5 diagonals |i - j| <= 2, values capped at 3, the rows fully unrolled so that the term's
// characters are static register reads and the word's are LDS broadcasts (every lane of a wave reads the same address).  It is
// exact for distances <= 2, which is all a tolerance <= 2 asks.  A wave whose lanes all fail the tests skips it.
// A candidate is one 64-bit key -- 2 bits distance, 31 bits 0x7FFFFFFF - weight, 31 bits term id: smaller is better, no two
// are equal.  Each wave leaves its first `limit` keys (repeated wave minimum; nearly always none or one) and its candidate
// count in LDS; after a barrier wave v merges the 16 waves' lists of word v of the group the same way and writes the
// workgroup's slot of the scratch: keys [word][span][limit] (absent: all ones) and counts [word][span].
//
// MERGE.  One workgroup per word sums the counts of its spans and sorts their keys with msr_sort.h's bitonic network, 2048 keys
// at a time, the best `limit` so far riding along; a block of spans without any key is not sorted.  It writes the word's row:
// term ids, distances, -1 behind them, n and the total.  A word that is not valid (length 0 or > 32, tolerance outside 0 .. 2)
// matches nothing in SCAN and gets an empty row here: no host round trip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_sort.h"
#include "msr_vocabscan.h"

namespace {

using namespace msr_vocabscan;                               // sig_bit, the 64-bit shuffles, the keys, wave_first_keys, the merge

constexpr int FZ_SPAN = VS_SPAN;
constexpr int FZ_WAVES = VS_WAVES;
constexpr int FZ_G = VS_G;
constexpr int FZ_LEN = VS_LEN;
constexpr int FZ_LIM = VS_LIM;
constexpr int FZ_PAD = 4;                                    // code points of padding on either side of a staged word
constexpr int FZ_ROW = FZ_LEN + 2 * FZ_PAD;
constexpr uint64_t FZ_NONE = VS_NONE;

struct FuzzyArgs {
    const int64_t* char_off; const uint16_t* chars; const uint32_t* weight; const uint64_t* sig;
    int64_t n_terms; int32_t n_spans;
    int32_t n_words; const int32_t* word_off; const uint16_t* word_chars; const int32_t* word_max; int32_t limit;
    uint64_t* keys; int32_t* counts;                         // the scratch: [n_words][n_spans][limit], [n_words][n_spans]
    int32_t* out_term; int32_t* out_dist; int32_t* out_n; int32_t* out_total;
};

// min(d(term, word), 3): tc = the term's L <= 32 code points, two per register; w = the word's LDS row (code point j, 1-based,
// at w[FZ_PAD + j - 1]; the padding never matches and is never inside a valid cell), n its length.  Row i, band slot k is the
// cell (i, j = i + k - 2); a cell outside the matrix or the band is 3.  Called by the lanes that passed the filters: the
// ballot sees those lanes only.
__device__ __forceinline__ int osa_le2(const uint32_t (&tc)[FZ_LEN / 2], int L, const uint16_t* w, int n) {
    int prev[5], pp[5], cur[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int j = k - 2;
        prev[k] = (j >= 0 && j <= n) ? j : 3;
        pp[k] = 3;
    }
    int res = L == 0 ? imin(n, 3) : 3;
    const int slot = n - L + 2;                              // in 0 .. 4: the length test has passed
    uint32_t t_before = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 1; i <= FZ_LEN; ++i) {
        if (__ballot(i <= L) == 0) break;
        const uint32_t ti = (tc[(i - 1) >> 1] >> (((i - 1) & 1) * 16)) & 0xFFFFu;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int j = i + k - 2;                         // (a constant once unrolled)
            int v = 3;
            if (j == 0) {
                v = imin(i, 3);
            } else if (j >= 1 && j <= FZ_LEN) {
                const uint32_t wj = w[FZ_PAD + j - 1];
                int best = prev[k] + (ti != wj ? 1 : 0);                     // substitution: (i - 1, j - 1)
                if (k < 4) best = imin(best, prev[k + 1] + 1);               // deletion: (i - 1, j)
                if (k > 0) best = imin(best, cur[k - 1] + 1);                // insertion: (i, j - 1)
                if (i >= 2 && j >= 2) {                                      // swap: (i - 2, j - 2)
                    const uint32_t wb = w[FZ_PAD + j - 2];
                    if (ti == wb && t_before == wj) best = imin(best, pp[k] + 1);
                }
                v = j <= n ? imin(best, 3) : 3;
            }
            cur[k] = v;
        }
        if (i == L) res = slot == 0 ? cur[0] : slot == 1 ? cur[1] : slot == 2 ? cur[2] : slot == 3 ? cur[3] : cur[4];
#pragma unroll
        for (int k = 0; k < 5; ++k) { pp[k] = prev[k]; prev[k] = cur[k]; }
        t_before = ti;
    }
    return res;
}

__global__ __launch_bounds__(FZ_SPAN) void fuzzy_scan_kernel(const FuzzyArgs a) {
    __shared__ uint16_t s_wch[FZ_G][FZ_ROW];
    __shared__ int32_t s_wlen[FZ_G], s_wmax[FZ_G];           // length 0: not a valid word
    __shared__ uint64_t s_wsig[FZ_G];
    __shared__ uint64_t s_key[FZ_G][FZ_WAVES * FZ_LIM];
    __shared__ int32_t s_cnt[FZ_G][FZ_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int span = (int)blockIdx.x, limit = a.limit;
    const int64_t t = (int64_t)span * FZ_SPAN + tid;

    // the lane's term; a lane without one (past n_terms, weight 0, too long) stays to the end: it takes part in every barrier
    bool term_ok = false;
    int L = 0;
    uint32_t tc[FZ_LEN / 2];
#pragma unroll
    for (int k = 0; k < FZ_LEN / 2; ++k) tc[k] = 0;
    uint64_t st = 0, key_low = 0;
    if (t < a.n_terms) {
        const uint32_t wt = a.weight[t];
        const int64_t o0 = a.char_off[t], len = a.char_off[t + 1] - o0;
        if (wt > 0 && wt < 0x80000000u && len >= 0 && len <= FZ_LEN) {
            term_ok = true;
            L = (int)len;
            st = a.sig[t];
            key_low = msr_vocabscan::key_low(wt, t);
#pragma unroll
            for (int i = 0; i < FZ_LEN; ++i) {
                const uint32_t c = i < L ? a.chars[o0 + i] : 0u;
                tc[i >> 1] |= c << ((i & 1) * 16);
            }
        }
    }

    for (int g0 = 0; g0 < a.n_words; g0 += FZ_G) {
        const int ng = imin(FZ_G, a.n_words - g0);
        if (tid < FZ_G * 32) {                               // 32 threads stage one word: whole waves, two words each
            const int g = tid >> 5, c = tid & 31;
            int len = 0, mx = 0, o = 0;
            bool ok = false;
            if (g < ng) {
                o = a.word_off[g0 + g];
                len = a.word_off[g0 + g + 1] - o;
                mx = a.word_max[g0 + g];
                ok = len >= 1 && len <= FZ_LEN && mx >= 0 && mx <= 2;
            }
            const bool have = ok && c < len;
            const uint32_t ch = have ? a.word_chars[o + c] : 0xFFFFu;
            s_wch[g][FZ_PAD + c] = (uint16_t)ch;
            if (c < FZ_PAD) { s_wch[g][c] = 0xFFFFu; s_wch[g][FZ_PAD + FZ_LEN + c] = 0xFFFFu; }
            uint64_t sb = have ? sig_bit(ch) : 0ull;
            for (int m = 16; m; m >>= 1) sb |= shfl_xor_u64(sb, m);          // (stays inside the 32 lanes of the word)
            if (c == 0) { s_wlen[g] = ok ? len : 0; s_wmax[g] = ok ? mx : 0; s_wsig[g] = sb; }
        }
        __syncthreads();
        for (int g = 0; g < ng; ++g) {
            const int n = s_wlen[g], m = s_wmax[g];
            const uint64_t sw = s_wsig[g];
            const int dl = L - n;
            const bool pass = term_ok && n > 0 && dl <= m && -dl <= m && __popcll(sw & ~st) <= m && __popcll(st & ~sw) <= m;
            uint64_t key[1] = {FZ_NONE};
            if (pass) {
                const int d = osa_le2(tc, L, &s_wch[g][0], n);
                if (d <= m) key[0] = ((uint64_t)d << 62) | key_low;
            }
            const uint64_t found = __ballot(key[0] != FZ_NONE);
            uint64_t keep = FZ_NONE;
            if (found) keep = wave_first_keys<1>(key, limit, lane);
            if (lane < limit) s_key[g][wave * limit + lane] = keep;
            if (lane == 0) s_cnt[g][wave] = __popcll(found);
        }
        __syncthreads();
        if (wave < ng) {                                     // wave v merges word v of the group
            const int g = wave;
            const int64_t slot = (int64_t)(g0 + g) * a.n_spans + span;
            span_slot_store(&s_key[g][0], &s_cnt[g][0], limit, lane, slot, a.keys, a.counts);
        }
        // (no barrier: the next group's staging writes what this merge does not read, and the barrier behind the staging
        // stands between this merge and the next group's lists)
    }
}

__global__ __launch_bounds__(MG_THREADS) void fuzzy_merge_kernel(const FuzzyArgs a) {
    merge_rows<true>(a.keys, a.counts, a.n_spans, a.limit, a.out_term, a.out_dist, a.out_n, a.out_total);
}

// *flag <- max(*flag, code): 1 char_off does not run from 0 to n_chars, 2 it descends, 3 a weight of 2^31 or more
__global__ void vocab_validate_kernel(const int64_t* char_off, const uint32_t* weight, int64_t n_terms, int64_t n_chars,
                                      int32_t* flag) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    int code = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_terms; t += step) {
        const int64_t o = char_off[t];
        if ((t == 0 && o != 0) || (t == n_terms && o != n_chars)) code = code > 1 ? code : 1;
        if (t < n_terms) {
            if (o > char_off[t + 1]) code = code > 2 ? code : 2;
            if (weight[t] >= 0x80000000u) code = 3;
        }
    }
    if (code) atomicMax(flag, code);
}

// sig[t] = the character-set signature of term t (0 for a term the lookup never matches: longer than FZ_LEN); the offsets
// have been validated
__global__ void vocab_signature_kernel(const int64_t* char_off, const uint16_t* chars, int64_t n_terms, uint64_t* sig) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_terms) return;
    const int64_t o = char_off[t], len = char_off[t + 1] - o;
    uint64_t s = 0;
    if (len <= FZ_LEN)
        for (int i = 0; i < (int)len; ++i) s |= sig_bit(chars[o + i]);
    sig[t] = s;
}

}  // namespace

hipError_t msr_vocab_validate(const int64_t* char_off, const uint32_t* weight, int64_t n_terms, int64_t n_chars, int32_t* flag,
                              hipStream_t stream) {
    const unsigned blocks = (unsigned)std::min<int64_t>((n_terms + 256) / 256, 4096);
    hipLaunchKernelGGL(vocab_validate_kernel, dim3(blocks), dim3(256), 0, stream, char_off, weight, n_terms, n_chars, flag);
    return hipGetLastError();
}

hipError_t msr_vocab_signatures(const int64_t* char_off, const uint16_t* chars, int64_t n_terms, uint64_t* sig,
                                hipStream_t stream) {
    if (n_terms <= 0) return hipSuccess;
    hipLaunchKernelGGL(vocab_signature_kernel, dim3((unsigned)((n_terms + 255) / 256)), dim3(256), 0, stream, char_off, chars,
                       n_terms, sig);
    return hipGetLastError();
}

int64_t msr_fuzzy_spans(int64_t n_terms) { return (n_terms + FZ_SPAN - 1) / FZ_SPAN; }

hipError_t msr_fuzzy_terms_run(const int64_t* char_off, const uint16_t* chars, const uint32_t* weight, const uint64_t* sig,
                               int64_t n_terms, int n_words, const int32_t* word_off, const uint16_t* word_chars,
                               const int32_t* word_max, int limit, int32_t* out_term, int32_t* out_dist, int32_t* out_n,
                               int32_t* out_total, void* scratch, hipStream_t stream) {
    if (n_words <= 0) return hipSuccess;
    const int64_t n_spans = msr_fuzzy_spans(n_terms);
    uint64_t* keys = (uint64_t*)scratch;
    int32_t* counts = (int32_t*)(keys + (int64_t)n_words * n_spans * limit);
    const FuzzyArgs a{char_off, chars, weight, sig, n_terms, (int32_t)n_spans, n_words, word_off, word_chars, word_max, limit,
                      keys, counts, out_term, out_dist, out_n, out_total};
    hipLaunchKernelGGL(fuzzy_scan_kernel, dim3((unsigned)n_spans), dim3(FZ_SPAN), 0, stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(fuzzy_merge_kernel, dim3((unsigned)n_words), dim3(MG_THREADS), 0, stream, a);
    return hipGetLastError();
}

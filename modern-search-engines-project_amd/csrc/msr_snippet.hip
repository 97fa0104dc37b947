// K14: query-biased snippets (msr_best_windows; include/msretr.h).
//
// Pair i = (document, row): the start of the window of `span` tokens of the document's OWN stream with the largest (cover, hits)
// -- cover = the summed weights of the row's distinct ids that stand in the window, hits = the positions of the window that
// hold one of them -- the smallest start among equal ones; with it the window's position mask and the row's term bits (the
// definitions stand in msretr.h).
//
// One wave owns one pair, four waves make a workgroup, and there is no workgroup-level step: no LDS, no barrier, a wave
// without a pair or with an invalid one writes its answer and leaves.  Lane j loads term j and weight j of the row; a repeated
// id loses its weight and its bit before the scan (lane j compares its id with the lanes below it).
//
// The scan is the chunk walker of msr_tokscan.h (shared with K13; the read bound, the ballots and a lane's 128-bit view of a
// term are explained there) with another evaluation.  Lane l's view of term j is cut to `span` bits; cover = the sum of w[j]
// over non-zero views, hits = the popcount of the OR of the views (a position holds one token: the union counts every hit
// once), and that OR is the window's mask.  Every lane keeps the best key of the starts it has seen, packed (cover, hits,
// -start) into one 64-bit integer, with that start's mask and term bits; ONE wave reduction at the document's end picks the
// winner, and lane 0 stores the five values.  Every chunk is read: there is no early exit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_tokscan.h"

namespace {

constexpr int SN_WAVES = 4;
constexpr int SN_THREADS = SN_WAVES * 64;
constexpr int SN_MAX = tokscan::MAX_TERMS;
static_assert(SN_MAX <= 32, "lane j of a wave holds term j, and out_terms has a bit per term");
// the key: cover in bits 38 .. 62, hits in bits 31 .. 37, 0x7FFFFFFF - start in bits 0 .. 30
static_assert((int64_t)SN_MAX * MSR_SNIPPET_MAX_WEIGHT < (1ll << 25), "cover has 25 bits of the key");
static_assert(MSR_PROX_MAX_SPAN < (1 << 7), "hits has 7 bits of the key");
constexpr int KEY_COVER = 38, KEY_HITS = 31;
constexpr uint32_t KEY_START = 0x7FFFFFFFu;

struct SnipArgs {
    const int64_t* tok_off;
    const int32_t* tok_ids;
    int64_t n_docs, n_terms;
    int32_t n_pairs; const int32_t* pair_doc; const int32_t* pair_row;
    int32_t n_rows; const int32_t* row_off; const int32_t* row_terms; const int32_t* row_weights; const int32_t* row_span;
    int32_t* out_start; int32_t* out_cover; int32_t* out_hits; uint64_t* out_mask; uint32_t* out_terms;
};

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void store(const SnipArgs& a, int i, int32_t start, int32_t cover, int32_t hits, uint64_t mask,
                                      uint32_t terms) {
    a.out_start[i] = start; a.out_cover[i] = cover; a.out_hits[i] = hits; a.out_mask[i] = mask; a.out_terms[i] = terms;
}

// One wave's walk of document [s, e), a row of at most LM terms.  mine / myw: lane j's id and weight, a lane without a term (or
// with a repeated one) holds -2 and 0.
template <int LM>
__device__ __forceinline__ void scan_document(const SnipArgs& a, int i, int64_t s, int64_t e, int lane, int32_t mine, int32_t myw,
                                              int L, int span) {
    using namespace tokscan;
    const uint64_t cut = window_cut(span);
    uint64_t cur[LM], nxt[LM];                               // (never members of a struct: msr_tokscan.h)
    int64_t pos;
    int32_t t_nxt;
    walk_start<LM>(a.tok_ids, s, e, lane, mine, L, cur, nxt, pos, t_nxt);
    uint64_t best = 0, best_mask = 0;                        // 0: no start with a hit seen yet
    uint32_t best_terms = 0;
    for (int64_t b0 = s; b0 < e; b0 += 64) {
        const int32_t t_far = load_token(a.tok_ids, pos += 64, e);   // the chunk after the next
        uint64_t any = 0;
#pragma unroll
        for (int j = 0; j < LM; ++j)
            if (j < L) {
                nxt[j] = term_mask(t_nxt, mine, j);
                any |= cur[j] | nxt[j];
            }
        if (any) {                                           // (a start of this chunk sees a hit only in these two chunks)
            uint64_t un = 0;
            uint32_t tb = 0;
            int32_t cover = 0;
#pragma unroll
            for (int j = 0; j < LM; ++j)
                if (j < L && (cur[j] | nxt[j]) != 0) {
                    const uint64_t v = view(cur[j], nxt[j], lane) & cut;
                    un |= v;
                    cover += v ? __builtin_amdgcn_readlane(myw, j) : 0;
                    tb |= v ? 1u << j : 0u;
                }
            const int hits = __popcll((unsigned long long)un);
            const int64_t start = b0 - s + lane;             // < e - s when this lane stands inside the document
            const uint64_t key = ((uint64_t)(uint32_t)cover << KEY_COVER) | ((uint64_t)(uint32_t)hits << KEY_HITS) |
                                 (uint64_t)(KEY_START - (uint32_t)start);
            if (b0 + lane < e && hits > 0 && key > best) { best = key; best_mask = un; best_terms = tb; }
        }
        walk_roll<LM>(cur, nxt, t_nxt, t_far);
    }
    uint64_t top = best;
    for (int m = 32; m; m >>= 1) {
        const uint64_t o = shfl_xor_u64(top, m);
        top = o > top ? o : top;
    }
    if (top == 0) {                                          // no position of the document holds a term of the row
        if (lane == 0) store(a, i, -1, 0, 0, 0, 0);
        return;
    }
    // the starts differ, so the keys do: exactly one lane holds the winner
    const int win = __ffsll((unsigned long long)__ballot(best == top)) - 1;
    const uint64_t mask = shfl_u64(best_mask, win);
    const uint32_t terms = (uint32_t)__shfl((int)best_terms, win);
    if (lane == 0)
        store(a, i, (int32_t)(KEY_START - (uint32_t)(top & KEY_START)), (int32_t)(top >> KEY_COVER),
              (int32_t)((top >> KEY_HITS) & 127u), mask, terms);
}

__global__ __launch_bounds__(SN_THREADS) void best_windows_kernel(const SnipArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int64_t i64 = (int64_t)blockIdx.x * SN_WAVES + wave;
    if (i64 >= a.n_pairs) return;                            // a wave without a pair
    const int i = (int)i64;
    const int64_t d = a.pair_doc[i];
    const int32_t r = a.pair_row[i];
    if (d < 0 || d >= a.n_docs || r < 0 || r >= a.n_rows) {
        if (lane == 0) store(a, i, -1, 0, 0, 0, 0);
        return;
    }
    // the row: 1 .. SN_MAX ids inside [0, n_terms), weights inside [0, MSR_SNIPPET_MAX_WEIGHT] and a span of 1 .. 64 tokens,
    // else the pair has no window (the row's scalars and the document's bounds are read together: one round trip)
    const int p0 = a.row_off[r], L = a.row_off[r + 1] - p0;
    const int span = a.row_span[r];
    const int64_t s = a.tok_off[d], e = a.tok_off[d + 1];
    bool bad = L < 1 || L > SN_MAX || span < 1 || span > MSR_PROX_MAX_SPAN;
    int32_t mine = -2, myw = 0;
    if (!bad && lane < L) {
        mine = a.row_terms[p0 + lane];
        myw = a.row_weights[p0 + lane];
        bad = mine < 0 || mine >= a.n_terms || myw < 0 || myw > MSR_SNIPPET_MAX_WEIGHT;
    }
    if (__ballot(bad) != 0) {
        if (lane == 0) store(a, i, -1, 0, 0, 0, 0);
        return;
    }
    // a repeated id counts once, with the weight and the bit of its first occurrence: the later lanes drop out
    bool dup = false;
#pragma unroll
    for (int j = 0; j < SN_MAX - 1; ++j) {
        const int32_t t = __builtin_amdgcn_readlane(mine, j);
        dup = dup || (j < lane && lane < L && t == mine);
    }
    if (dup) { mine = -2; myw = 0; }
    // the widest row decides the scan (wave-uniform: a branch per wave)
    if (L <= 4) scan_document<4>(a, i, s, e, lane, mine, myw, L, span);
    else if (L <= 8) scan_document<8>(a, i, s, e, lane, mine, myw, L, span);
    else scan_document<SN_MAX>(a, i, s, e, lane, mine, myw, L, span);
}

}  // namespace

hipError_t msr_best_windows_run(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_terms, int n_pairs,
                                const int32_t* pair_doc, const int32_t* pair_row, int n_rows, const int32_t* row_off,
                                const int32_t* row_terms, const int32_t* row_weights, const int32_t* row_span, int32_t* out_start,
                                int32_t* out_cover, int32_t* out_hits, uint64_t* out_mask, uint32_t* out_terms,
                                hipStream_t stream) {
    if (n_pairs <= 0) return hipSuccess;
    const SnipArgs a{tok_off, tok_ids, n_docs, n_terms, n_pairs, pair_doc, pair_row, n_rows, row_off, row_terms, row_weights,
                     row_span, out_start, out_cover, out_hits, out_mask, out_terms};
    const unsigned grid = (unsigned)(((int64_t)n_pairs + SN_WAVES - 1) / SN_WAVES);
    hipLaunchKernelGGL(best_windows_kernel, dim3(grid), dim3(SN_THREADS), 0, stream, a);
    return hipGetLastError();
}

// K19: "at least m of these words" as document sets (msr_match_sets, include/msretr_match.h).
//
// Row r of the output is  base(r)  AND  { d : the number of row r's groups with a term whose list holds d  >=  need(r) },  in the
// layout and under the write contract of K11's rows: the producer that COUNTS.  A group is a list of term ids -- a word, or the
// expansions of a pattern -- and is filled by a document that stands in any of its lists.
//
// The ownership is K11's (msr_tokscan.h): one workgroup owns (row, span of MSR_TERMSET_SPAN_DOCS documents), one 32-bit word per
// thread.  Per group the workgroup ORs every list of the group into the span's LDS words (the ranges of up to 256 terms are found
// side by side, one thread per term: for a row of at most 256 terms all of them up front, whatever groups they belong to, as
// K11 does for its must lists), then each thread adds ITS word into a bit-sliced counter that lives in its
// registers: PLANES words, plane i holding bit i of the count of each of the thread's 32 documents, added by ripple carry.  After
// the last group a bit-sliced compare against need(r) -- the same instructions in every thread -- gives the word.  The OR in LDS
// is order-independent and everything else is per thread, so the bytes do not depend on the schedule; plain stores of whole
// words, no global atomics, nothing to zero beforehand.
//
// Early exit: once so few groups are left that a document needs a count above 0 to still reach need(r), a span in which no
// document of the base can reach it skips the remaining lists (with need == G this is K11's exit).  The test -- one compare and
// one barrier -- is made only from that group on: a row with need == 1 never pays for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr_match.h"
#include "msr_internal.h"
#include "msr_tokscan.h"

namespace {

using namespace tokscan;

constexpr int PLANES = 7;                                // counts 0 .. MSR_MATCH_MAX_GROUPS
static_assert(MSR_MATCH_MAX_GROUPS < (1 << PLANES), "the planes hold every count a row can reach");

struct MatchArgs {
    const int64_t* term_off;
    const int32_t* post_doc;
    const int32_t* heavy_id;     // nullable
    const uint32_t* tile_off;
    int64_t n_terms, n_docs;
    int32_t n_tiles;
    const int32_t* row_group_off; const int32_t* group_term_off; const int32_t* group_terms; const int32_t* row_need;
    const uint32_t* base_bits; int32_t n_base; int64_t base_stride; const int32_t* row_base;
    uint32_t* out_bits; int64_t out_stride;
    int32_t row0;
};

// the documents (of a thread's 32) whose count is >= thr, 0 <= thr < 2^PLANES: compared from the top plane down
__device__ __forceinline__ uint32_t at_least(const uint32_t (&p)[PLANES], int thr) {
    uint32_t gt = 0, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int i = PLANES - 1; i >= 0; --i) {
        const uint32_t tb = (thr >> i & 1) ? 0xFFFFFFFFu : 0u;
        gt |= eq & p[i] & ~tb;
        eq &= ~(p[i] ^ tb);
    }
    return gt | eq;
}

// thread j < cnt: the span's postings of term group_terms[first + j] -> r_lo[j], r_hi[j] (an id the index lacks: none)
__device__ __forceinline__ void find_ranges(const MatchArgs& a, int first, int cnt, int64_t d0, int tid, int64_t* r_lo, int64_t* r_hi) {
    if (tid < cnt) {
        const int32_t t = a.group_terms[first + tid];
        int64_t lo = 0, hi = 0;
        if (t >= 0 && t < a.n_terms) span_postings(a, t, d0, &lo, &hi);
        r_lo[tid] = lo; r_hi[tid] = hi;
    }
}

__global__ __launch_bounds__(THREADS) void match_sets_kernel(const MatchArgs a) {
    __shared__ uint32_t bits[THREADS];
    __shared__ int64_t r_lo[THREADS], r_hi[THREADS];         // the span's postings of up to THREADS terms, found side by side
    const int tid = (int)threadIdx.x;
    const int r = a.row0 + (int)blockIdx.y;
    const int64_t d0 = (int64_t)blockIdx.x * SPAN;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (d0 >> 5) + tid;                   // this thread's word of the row
    const int g0 = a.row_group_off[r], g1 = a.row_group_off[r + 1], need = a.row_need[r];
    const int G = g1 - g0;

    // base(r), without the bits at or above n_docs
    uint32_t acc = set_word(a.base_bits, a.n_base, a.base_stride, a.n_base > 0 ? a.row_base[r] : -1, w, W, a.n_docs);
    if (need > 0) {                                      // (need <= 0: the base itself)
        if (G > MSR_MATCH_MAX_GROUPS || need > G) {      // more groups than the planes count, or more asked for than there are
            acc = 0;
        } else {
            uint32_t p[PLANES];
#pragma unroll
            for (int i = 0; i < PLANES; ++i) p[i] = 0;
            // The row's terms are one run of group_terms, [T0, T1), that its groups cut.  A row of at most THREADS terms -- every
            // row of single words -- has the spans' postings of ALL its terms found in one round up front (thread j: term T0 +
            // j), so the searches' dependent loads run side by side and not one group after the other; a longer row finds them
            // group by group, in rounds of THREADS.
            const int T0 = a.group_term_off[g0], T1 = a.group_term_off[g1];
            const bool one_round = T1 - T0 <= THREADS;
            if (one_round) find_ranges(a, T0, T1 - T0, d0, tid, r_lo, r_hi);
            int alive = 1;
            for (int g = g0; g < g1 && alive; ++g) {
                const int t0 = max(a.group_term_off[g], T0), t1 = min(a.group_term_off[g + 1], T1);
                bits[tid] = 0;
                if (one_round) {
                    __syncthreads();                     // every word of bits is zero, the ranges are there
                    for (int k = t0; k < t1; ++k) or_postings(a.post_doc, r_lo[k - T0], r_hi[k - T0], d0, bits);
                    __syncthreads();
                } else {
                    for (int i0 = t0; i0 < t1; i0 += THREADS) {
                        const int cnt = min(THREADS, t1 - i0);
                        find_ranges(a, i0, cnt, d0, tid, r_lo, r_hi);
                        __syncthreads();                 // (also: every word of bits is zero before the first OR)
                        for (int k = 0; k < cnt; ++k) or_postings(a.post_doc, r_lo[k], r_hi[k], d0, bits);
                        __syncthreads();
                    }
                }
                uint32_t c = bits[tid];                  // the group's documents among this thread's 32: add 1 to each
#pragma unroll
                for (int j = 0; j < PLANES; ++j) {
                    const uint32_t t = p[j] & c;
                    p[j] ^= c;
                    c = t;
                }
                // with `left` groups to come a document still reaches need iff its count is >= need - left
                const int left = g1 - 1 - g;
                if (left > 0 && need - left > 0) alive = __syncthreads_or((at_least(p, need - left) & acc) != 0);
            }
            acc = alive ? acc & at_least(p, need) : 0;
        }
    }
    if (w < W) a.out_bits[(int64_t)r * a.out_stride + w] = acc;
}

}  // namespace

hipError_t msr_match_sets_run(const Bm25Index& ix, int n_rows, const int32_t* row_group_off, const int32_t* group_term_off,
                              const int32_t* group_terms, const int32_t* row_need, const uint32_t* base_bits, int n_base,
                              int64_t base_stride, const int32_t* row_base, uint32_t* out_bits, int64_t out_stride,
                              hipStream_t stream) {
    const MatchArgs a{ix.term_off, ix.post_doc, ix.heavy_id, ix.tile_off, ix.n_terms, ix.n_docs, ix.n_tiles, row_group_off,
                      group_term_off, group_terms, row_need, base_bits, n_base, base_stride, row_base, out_bits, out_stride, 0};
    return launch_rows(match_sets_kernel, span_count(ix.n_docs), THREADS, n_rows, a, stream);
}

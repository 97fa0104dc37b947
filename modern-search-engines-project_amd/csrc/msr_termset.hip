// K11: document sets from posting lists (msr_term_sets, include/msretr.h).
//
// Row r of the output is  base(r)  AND  D(t) for every must term t  AND NOT  D(t) for every not term t,  as a bitset in the
// layout of K8 (document d = bit d & 31 of word d >> 5): the producer of the rows that msr_*_topk_within consume.
//
// One workgroup owns (row, span of MSR_TERMSET_SPAN_DOCS consecutive documents): one 32-bit word per thread (the ownership
// rule, its constants and the base word of a row stand in msr_tokscan.h, which K12 and K13 share; so do span_postings and
// or_postings below, which K17's count kernel in msr_facet.hip uses as well).  The row's accumulator word
// lives in a register of its thread, the bits of ONE posting list (or of all not lists together) in LDS.
// Per term one thread finds the postings of the span -- two loads of the BM25 skip table for a long list, a binary search
// on post_doc otherwise; up to 256 terms' searches run side by side -- then the workgroup streams post_doc (4 bytes per
// posting) and ORs a bit per posting into LDS: an OR is order-independent, so the words do not depend on the schedule.
// The span is stored with plain stores of whole words; no word of the output belongs to two workgroups, so there are no
// global atomics and nothing to zero beforehand.  A span whose accumulator is empty skips every remaining list.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_tokscan.h"

namespace {

using namespace tokscan;

struct TermSetArgs {
    const int64_t* term_off;
    const int32_t* post_doc;
    const int32_t* heavy_id;     // nullable
    const uint32_t* tile_off;
    int64_t n_terms, n_docs;
    int32_t n_tiles;
    const int32_t* must_off; const int32_t* must_terms;
    const int32_t* not_off; const int32_t* not_terms;
    const uint32_t* base_bits; int32_t n_base; int64_t base_stride; const int32_t* row_base;
    uint32_t* out_bits; int64_t out_stride;
    int32_t row0;
};

__global__ __launch_bounds__(THREADS) void term_sets_kernel(const TermSetArgs a) {
    __shared__ uint32_t bits[THREADS];
    __shared__ int64_t r_lo[THREADS], r_hi[THREADS];         // the span's postings of up to THREADS terms, found side by side
    const int tid = (int)threadIdx.x;
    const int r = a.row0 + (int)blockIdx.y;
    const int64_t d0 = (int64_t)blockIdx.x * SPAN;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (d0 >> 5) + tid;                   // this thread's word of the row
    const int m0 = a.must_off[r], m1 = a.must_off[r + 1], x0 = a.not_off[r], x1 = a.not_off[r + 1];

    // base(r), without the bits at or above n_docs
    uint32_t acc = set_word(a.base_bits, a.n_base, a.base_stride, a.n_base > 0 ? a.row_base[r] : -1, w, W, a.n_docs);
    // a must term the index lacks (or whose list is empty) empties the row whatever the others hold
    int lacks = 0;
    for (int i = m0 + tid; i < m1; i += THREADS) {
        const int32_t t = a.must_terms[i];
        if (t < 0 || t >= a.n_terms || a.term_off[t] == a.term_off[t + 1]) lacks = 1;
    }
    if (__syncthreads_or(lacks)) acc = 0;
    int alive = __syncthreads_or(acc != 0);

    // must terms: thread j finds the span's postings of the round's j-th term (the searches' dependent loads run side by side
    // instead of one term after the other), then the lists are folded in one at a time
    for (int i0 = m0; i0 < m1 && alive; i0 += THREADS) {
        const int cnt = min(THREADS, m1 - i0);
        if (tid < cnt) span_postings(a, a.must_terms[i0 + tid], d0, &r_lo[tid], &r_hi[tid]);   // (alive: every must id is valid)
        __syncthreads();
        for (int k = 0; k < cnt && alive; ++k) {
            bits[tid] = 0;
            __syncthreads();
            or_postings(a.post_doc, r_lo[k], r_hi[k], d0, bits);
            __syncthreads();
            acc &= bits[tid];
            alive = __syncthreads_or(acc != 0);          // (also: every thread is done with bits and r_* of this term)
        }
    }
    if (alive && x0 < x1) {                              // the not lists share one OR
        bits[tid] = 0;
        for (int i0 = x0; i0 < x1; i0 += THREADS) {
            const int cnt = min(THREADS, x1 - i0);
            if (tid < cnt) {
                const int32_t t = a.not_terms[i0 + tid];
                int64_t lo = 0, hi = 0;
                if (t >= 0 && t < a.n_terms) span_postings(a, t, d0, &lo, &hi);
                r_lo[tid] = lo; r_hi[tid] = hi;
            }
            __syncthreads();
            for (int k = 0; k < cnt; ++k) or_postings(a.post_doc, r_lo[k], r_hi[k], d0, bits);
            __syncthreads();
        }
        acc &= ~bits[tid];
    }
    if (w < W) a.out_bits[(int64_t)r * a.out_stride + w] = acc;
}

}  // namespace

hipError_t msr_term_sets_run(const Bm25Index& ix, int n_rows, const int32_t* must_off, const int32_t* must_terms,
                             const int32_t* not_off, const int32_t* not_terms, const uint32_t* base_bits, int n_base,
                             int64_t base_stride, const int32_t* row_base, uint32_t* out_bits, int64_t out_stride,
                             hipStream_t stream) {
    const TermSetArgs a{ix.term_off, ix.post_doc, ix.heavy_id, ix.tile_off, ix.n_terms, ix.n_docs, ix.n_tiles, must_off,
                        must_terms, not_off, not_terms, base_bits, n_base, base_stride, row_base, out_bits, out_stride, 0};
    return launch_rows(term_sets_kernel, span_count(ix.n_docs), THREADS, n_rows, a, stream);
}

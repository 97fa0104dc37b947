// K13: proximity search (msr_proximity_sets; include/msretr.h).
//
// Row r is the documents of a candidate set whose OWN token stream holds the row's terms inside a window of `span` tokens, in
// the row's order or in any order (the definitions stand in msretr.h), as a bitset in the layout of K8 / K11 / K12.
//
// Ownership is K12's, with K12's code (msr_tokscan.h): one workgroup of 256 threads owns (row, span of MSR_TERMSET_SPAN_DOCS
// consecutive documents), thread j loads candidate word j, a span without a candidate stores zeros and leaves, the candidates
// are compacted into an LDS list, one wave takes one candidate document at a time, one lane ORs the document's bit into an LDS
// word and after one barrier thread j stores word j.
//
// The per-document scan is the chunk walker of msr_tokscan.h (shared with K14; the read bound, the ballots and a lane's 128-bit
// view of a term are explained there): bit k of view j cut to `span` bits = "p[j] stands at this lane's position + k".  Any
// order: a window starts at lane l iff every view is non-zero.  Ordered: a lane whose token is p[0] walks j = 1 .. L - 1, each
// time to the lowest set bit of view j above the last one (for a fixed start the earliest next occurrence minimises the end,
// and every start is tried).  Ordered with span == L is the exact phrase and needs no lane's view: AND over j of
// (pair j >> j) != 0, scalar arithmetic on the ballots.  The wave stops at the first chunk with a match.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_tokscan.h"

namespace {

using namespace tokscan;

struct ProxArgs {
    const int64_t* tok_off;
    const int32_t* tok_ids;
    int64_t n_docs, n_terms;
    const int32_t* phrase_off; const int32_t* phrase_terms; const int32_t* row_span; const int32_t* row_ordered;
    const uint32_t* cand_bits; int32_t n_cand; int64_t cand_stride; const int32_t* row_cand;
    uint32_t* out_bits; int64_t out_stride;
    int32_t row0;
};

// One wave's walk of the block's candidate list, rows of at most LM terms.
template <int LM>
__device__ __forceinline__ void scan_candidates(const ProxArgs& a, int64_t d0, const uint16_t* list, int total, int wave, int lane,
                                                int32_t mine, int L, int span, bool ordered, uint32_t* found) {
    const uint64_t cut = window_cut(span);
    const bool exact = ordered && span == L;
    for (int c = wave; c < total; c += WAVES) {          // one wave per candidate document (c is uniform in the wave)
        const int dl = __builtin_amdgcn_readfirstlane((int)list[c]);
        const int64_t d = d0 + dl;                       // < n_docs: the candidate word was masked
        const int64_t s = a.tok_off[d], e = a.tok_off[d + 1];
        uint64_t cur[LM], nxt[LM];                       // (never members of a struct: msr_tokscan.h)
        int64_t pos;
        int32_t t_nxt;
        walk_start<LM>(a.tok_ids, s, e, lane, mine, L, cur, nxt, pos, t_nxt);
        bool hit = false;
        for (int64_t b0 = s; b0 < e && !hit; b0 += 64) {
            const int32_t t_far = load_token(a.tok_ids, pos += 64, e);   // the chunk after the next
            bool all = !ordered || cur[0] != 0;          // every term stands in the two chunks; ordered: a start in this one
#pragma unroll
            for (int j = 0; j < LM; ++j)
                if (j < L) {
                    nxt[j] = term_mask(t_nxt, mine, j);
                    all = all && (cur[j] | nxt[j]) != 0;
                }
            if (all) {
                if (exact) {                             // the exact phrase: wave-uniform, bit i = a match starting at b0 + i
                    uint64_t m = cur[0];
#pragma unroll
                    for (int j = 1; j < LM; ++j)
                        if (j < L) m &= (cur[j] >> j) | (nxt[j] << (64 - j));
                    hit = m != 0;
                } else if (!ordered) {
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < LM; ++j)
                        if (j < L) ok = ok && (view(cur[j], nxt[j], lane) & cut) != 0;
                    hit = __ballot(ok) != 0;
                } else {
                    bool ok = (cur[0] >> lane) & 1;
                    int at = 0;                          // the offset of term j - 1 from this lane's position
#pragma unroll
                    for (int j = 1; j < LM; ++j)
                        if (j < L) {
                            const uint64_t m = view(cur[j], nxt[j], lane) & cut & ~((2ull << at) - 1ull);   // above `at`
                            ok = ok && m != 0;
                            at = m ? __ffsll((unsigned long long)m) - 1 : 63;
                        }
                    hit = __ballot(ok) != 0;
                }
            }
            walk_roll<LM>(cur, nxt, t_nxt, t_far);
        }
        if (hit && lane == 0) atomicOr(&found[dl >> 5], 1u << (dl & 31));
    }
}

__global__ __launch_bounds__(THREADS) void proximity_sets_kernel(const ProxArgs a) {
    __shared__ uint32_t found[THREADS];
    __shared__ uint16_t list[SPAN];                      // the span's candidate documents (offset in the span), ascending
    __shared__ int32_t ph[MAX_TERMS];
    __shared__ int32_t wave_cnt[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = a.row0 + (int)blockIdx.y;
    const int64_t d0 = (int64_t)blockIdx.x * SPAN;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (d0 >> 5) + tid;                   // this thread's word of the row
    // the row: 1 .. MAX_TERMS ids inside [0, n_terms) and a span of 1 .. 64 tokens, else it is empty (the row's scalars are read
    // together, in front of the candidate word: one round trip, not one per array)
    const int32_t sel = a.n_cand > 0 ? a.row_cand[r] : -1;
    const int p0 = a.phrase_off[r], L = a.phrase_off[r + 1] - p0;
    const int span = a.row_span[r];
    const bool ordered = a.row_ordered[r] != 0;
    uint32_t acc = set_word(a.cand_bits, a.n_cand, a.cand_stride, sel, w, W, a.n_docs);
    int bad = (L < 1 || L > MAX_TERMS || span < 1 || span > MSR_PROX_MAX_SPAN);
    if (!bad && tid < L) {
        const int32_t t = a.phrase_terms[p0 + tid];
        ph[tid] = t;
        bad = (t < 0 || t >= a.n_terms);
    }
    if (__syncthreads_or(bad)) acc = 0;                  // (also: ph is visible)
    if (!__syncthreads_or(acc != 0)) {
        if (w < W) a.out_bits[(int64_t)r * a.out_stride + w] = 0;
        return;
    }

    const int total = compact_candidates(acc, tid, lane, wave, found, list, wave_cnt);

    // lane j holds term j; the scan reads it with a constant lane index: no LDS in the scan
    const int32_t mine = lane < L ? ph[lane] : -2;
    if (L <= 4) scan_candidates<4>(a, d0, list, total, wave, lane, mine, L, span, ordered, found);
    else if (L <= 8) scan_candidates<8>(a, d0, list, total, wave, lane, mine, L, span, ordered, found);
    else scan_candidates<MAX_TERMS>(a, d0, list, total, wave, lane, mine, L, span, ordered, found);
    __syncthreads();
    if (w < W) a.out_bits[(int64_t)r * a.out_stride + w] = found[tid];
}

}  // namespace

hipError_t msr_proximity_sets_run(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_terms, int n_rows,
                                  const int32_t* phrase_off, const int32_t* phrase_terms, const int32_t* row_span,
                                  const int32_t* row_ordered, const uint32_t* cand_bits, int n_cand, int64_t cand_stride,
                                  const int32_t* row_cand, uint32_t* out_bits, int64_t out_stride, hipStream_t stream) {
    const ProxArgs a{tok_off, tok_ids, n_docs, n_terms, phrase_off, phrase_terms, row_span, row_ordered, cand_bits, n_cand,
                     cand_stride, row_cand, out_bits, out_stride, 0};
    return launch_rows(proximity_sets_kernel, span_count(n_docs), THREADS, n_rows, a, stream);
}

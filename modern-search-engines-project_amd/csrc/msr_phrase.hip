// K12: phrase search (msr_bind_tokens, msr_phrase_sets, msr_combine_sets; include/msretr.h).
//
// The forward index is the token-id stream of every document (tok_off int64 [N + 1], tok_ids int32 [T]).  Row r of
// msr_phrase_sets is the documents of a candidate set whose OWN stream holds the row's phrase at consecutive positions, as a
// bitset in the layout of K8 / K11 (document d = bit d & 31 of word d >> 5).
//
// One workgroup owns (row, span of MSR_TERMSET_SPAN_DOCS consecutive documents): one 32-bit word per thread, K11's ownership
// (msr_tokscan.h: the rule, the candidate word and the compaction, shared with K11 and K13).  Thread j loads candidate word j;
// a span without a candidate stores zeros and leaves (a phrase's intersection leaves most spans empty).  Otherwise the
// candidates are compacted into an LDS list and the four waves take documents from it, one wave per document: the lanes
// stride the stream 64 tokens at a time (one coalesced 256-byte load),
// a lane whose token equals the phrase's first id reads the following ids (lines the wave has just loaded) and leaves at the
// first mismatch.  THE BOUND OF EVERY READ IS THE DOCUMENT'S END tok_off[d + 1]: a lane at position i tests only if
// i + L <= len(d), so a match never crosses into the next document and the last document never reads past the buffer.  The
// wave stops at the first hit; one lane ORs the document's bit into an LDS word; after one barrier thread j stores word j.
// Plain stores of whole words, no global atomics, nothing to zero beforehand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_tokscan.h"

namespace {

using namespace tokscan;

struct PhraseArgs {
    const int64_t* tok_off;
    const int32_t* tok_ids;
    int64_t n_docs, n_terms;
    const int32_t* phrase_off; const int32_t* phrase_terms;
    const uint32_t* cand_bits; int32_t n_cand; int64_t cand_stride; const int32_t* row_cand;
    uint32_t* out_bits; int64_t out_stride;
    int32_t row0;
};

__global__ __launch_bounds__(THREADS) void phrase_sets_kernel(const PhraseArgs a) {
    __shared__ uint32_t found[THREADS];
    __shared__ uint16_t list[SPAN];                      // the span's candidate documents (offset in the span), ascending
    __shared__ int32_t ph[MAX_TERMS];
    __shared__ int32_t wave_cnt[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = a.row0 + (int)blockIdx.y;
    const int64_t d0 = (int64_t)blockIdx.x * SPAN;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (d0 >> 5) + tid;                   // this thread's word of the row
    uint32_t acc = set_word(a.cand_bits, a.n_cand, a.cand_stride, a.n_cand > 0 ? a.row_cand[r] : -1, w, W, a.n_docs);

    // the phrase: 1 .. MAX_TERMS ids inside [0, n_terms), else the row is empty
    const int p0 = a.phrase_off[r], L = a.phrase_off[r + 1] - p0;
    int bad = (L < 1 || L > MAX_TERMS);
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

    const int32_t first = ph[0];
    for (int c = wave; c < total; c += WAVES) {          // one wave per candidate document (c is uniform in the wave)
        const int dl = list[c];
        const int64_t d = d0 + dl;                       // < n_docs: the candidate word was masked
        const int64_t s = a.tok_off[d], e = a.tok_off[d + 1];
        if (e - s < L) continue;                         // the phrase is longer than the document
        const int64_t last = e - L;                      // the last position a phrase can start at; every read is below e
        bool hit = false;
        for (int64_t b0 = s; b0 <= last && !hit; b0 += 64) {
            const int64_t pos = b0 + lane;
            int m = 0;
            if (pos <= last && a.tok_ids[pos] == first) {
                m = 1;
                for (int j = 1; j < L; ++j)
                    if (a.tok_ids[pos + j] != ph[j]) { m = 0; break; }
            }
            hit = __ballot(m) != 0;
        }
        if (hit && lane == 0) atomicOr(&found[dl >> 5], 1u << (dl & 31));
    }
    __syncthreads();
    if (w < W) a.out_bits[(int64_t)r * a.out_stride + w] = found[tid];
}

struct CombineArgs {
    const int32_t* and_off; const int32_t* and_rows; const int32_t* not_off; const int32_t* not_rows;
    const uint32_t* in_bits; int32_t n_in; int64_t in_stride;
    uint32_t* out_bits; int64_t out_stride;
    int64_t n_docs;
    int32_t row0;
};

// out[r] = AND of the listed rows AND NOT (OR of the listed rows): one word per thread
__global__ __launch_bounds__(256) void combine_sets_kernel(const CombineArgs a) {
    const int r = a.row0 + (int)blockIdx.y;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= W) return;
    uint32_t acc = tail_mask(w, W, a.n_docs);
    for (int i = a.and_off[r]; i < a.and_off[r + 1]; ++i) {
        const int32_t s = a.and_rows[i];
        if (s >= 0 && s < a.n_in) acc &= a.in_bits[(int64_t)s * a.in_stride + w];
        else acc = 0;
    }
    uint32_t x = 0;
    for (int i = a.not_off[r]; i < a.not_off[r + 1]; ++i) {
        const int32_t s = a.not_rows[i];
        if (s >= 0 && s < a.n_in) x |= a.in_bits[(int64_t)s * a.in_stride + w];
    }
    a.out_bits[(int64_t)r * a.out_stride + w] = acc & ~x;
}

// *flag <- max(*flag, code): 1 offsets do not start at 0 / end at n_tokens, 2 a descent, 3 an id outside [0, n_terms)
__global__ void tokens_validate_kernel(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_tokens,
                                       int64_t n_terms, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    int code = 0;
    if (i == 0 && (tok_off[0] != 0 || tok_off[n_docs] != n_tokens)) code = 1;
    for (int64_t d = i; d < n_docs; d += step)
        if (tok_off[d + 1] < tok_off[d]) code = max(code, 2);
    for (int64_t p = i; p < n_tokens; p += step) {
        const int32_t t = tok_ids[p];
        if (t < 0 || t >= n_terms) code = max(code, 3);
    }
    if (code) atomicMax(flag, code);
}

}  // namespace

hipError_t msr_tokens_validate(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_tokens, int64_t n_terms,
                               int32_t* flag, hipStream_t stream) {
    const int64_t n = std::max(n_docs, n_tokens);
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 4096);
    hipLaunchKernelGGL(tokens_validate_kernel, dim3(blocks), dim3(256), 0, stream, tok_off, tok_ids, n_docs, n_tokens, n_terms, flag);
    return hipGetLastError();
}

hipError_t msr_phrase_sets_run(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_terms, int n_rows,
                               const int32_t* phrase_off, const int32_t* phrase_terms, const uint32_t* cand_bits, int n_cand,
                               int64_t cand_stride, const int32_t* row_cand, uint32_t* out_bits, int64_t out_stride,
                               hipStream_t stream) {
    const PhraseArgs a{tok_off, tok_ids, n_docs, n_terms, phrase_off, phrase_terms, cand_bits, n_cand, cand_stride, row_cand,
                       out_bits, out_stride, 0};
    return launch_rows(phrase_sets_kernel, span_count(n_docs), THREADS, n_rows, a, stream);
}

hipError_t msr_combine_sets_run(int64_t n_docs, int n_rows, const int32_t* and_off, const int32_t* and_rows,
                                const int32_t* not_off, const int32_t* not_rows, const uint32_t* in_bits, int n_in,
                                int64_t in_stride, uint32_t* out_bits, int64_t out_stride, hipStream_t stream) {
    const CombineArgs a{and_off, and_rows, not_off, not_rows, in_bits, n_in, in_stride, out_bits, out_stride, n_docs, 0};
    return launch_rows(combine_sets_kernel, ((n_docs + 31) / 32 + 255) / 256, 256, n_rows, a, stream);
}

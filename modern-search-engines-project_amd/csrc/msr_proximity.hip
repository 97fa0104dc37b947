// K13: proximity search (msr_proximity_sets; include/msretr.h).
//
// Row r is the documents of a candidate set whose OWN token stream holds the row's terms inside a window of `span` tokens, in
// the row's order or in any order (the definitions stand in msretr.h), as a bitset in the layout of K8 / K11 / K12.
//
// Ownership is K12's, restated here so that msr_phrase.hip and its recorded resources stay what they are: one workgroup of
// 256 threads owns (row, span of MSR_TERMSET_SPAN_DOCS consecutive documents), thread j loads candidate word j, a span without
// a candidate stores zeros and leaves, the candidates are compacted into an LDS list, one wave takes one candidate document
// at a time, one lane ORs the document's bit into an LDS word and after one barrier thread j stores word j.
//
// The per-document scan is the new part.  It has no dependent load and touches no LDS: the wave walks the document in chunks
// of 64 tokens, lane l = position b0 + l, one coalesced 256-byte load per chunk.  THE BOUND OF EVERY READ IS THE DOCUMENT'S END
// tok_off[d + 1]: a lane at or past it loads nothing and holds -1, which equals no term of a valid row, so a window never
// leaves the document and the last document never reads past the buffer.  Per chunk and term j one __ballot(tok == p[j]) gives
// a wave-uniform 64-bit mask; the masks of the current and of the next chunk are kept (span <= 64: two chunks hold every
// window that starts in the current one), and the load of the chunk after the next is in flight while the current one is
// evaluated.  Lane l's view of term j is the 128-bit pair shifted right by l and cut to `span` bits: bit k = "p[j] stands at
// this lane's position + k".  Any order: a window starts at lane l iff every view is non-zero.  Ordered: a lane whose token is
// p[0] walks j = 1 .. L - 1, each time to the lowest set bit of view j above the last one (for a fixed start the earliest next
// occurrence minimises the end, and every start is tried).  Ordered with span == L is the exact phrase and needs no lane's
// view: AND over j of (pair j >> j) != 0, scalar arithmetic on the ballots.  The wave stops at the first chunk with a match.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"

namespace {

constexpr int PX_SPAN = MSR_TERMSET_SPAN_DOCS;
constexpr int PX_THREADS = PX_SPAN / 32;                 // one word of the span per thread
constexpr int PX_WAVES = PX_THREADS / 64;
constexpr int PX_MAX = MSR_PHRASE_MAX_TERMS;
static_assert(PX_THREADS == 256, "the candidate compaction assumes four waves of 64");
static_assert(PX_SPAN <= 65536, "a candidate's offset in its span is kept in 16 bits");
static_assert(PX_MAX <= 64, "lane j of a wave holds term j");
static_assert(MSR_PROX_MAX_SPAN == 64, "a window spans at most the current chunk and the next");

struct ProxArgs {
    const int64_t* tok_off;
    const int32_t* tok_ids;
    int64_t n_docs, n_terms;
    const int32_t* phrase_off; const int32_t* phrase_terms; const int32_t* row_span; const int32_t* row_ordered;
    const uint32_t* cand_bits; int32_t n_cand; int64_t cand_stride; const int32_t* row_cand;
    uint32_t* out_bits; int64_t out_stride;
    int32_t row0;
};

// the words of row_sel's set below n_docs: -1 (or no rows at all) = every document, a row of `bits`, anything else = empty
__device__ __forceinline__ uint32_t set_word(const uint32_t* bits, int32_t n_rows, int64_t stride, int32_t sel, int64_t w,
                                             int64_t W, int64_t n_docs) {
    if (w >= W) return 0;
    uint32_t acc = (w == W - 1 && (n_docs & 31)) ? (1u << (n_docs & 31)) - 1u : 0xFFFFFFFFu;
    if (n_rows > 0) {
        if (sel >= 0 && sel < n_rows) acc &= bits[(int64_t)sel * stride + w];
        else if (sel != -1) acc = 0;
    }
    return acc;
}

// this lane's view of a term: bit k = the term stands at (chunk start + lane + k); a shift by 64 is undefined, lane 0 takes cur
__device__ __forceinline__ uint64_t view(uint64_t cur, uint64_t nxt, int lane) {
    return lane ? (cur >> lane) | (nxt << (64 - lane)) : cur;
}

// One wave's walk of the block's candidate list, rows of at most LM terms (the loops over j are unrolled to LM, so that every
// mask has a register of its own: 2 LM wave-uniform 64-bit masks are alive at once).
template <int LM>
__device__ __forceinline__ void scan_candidates(const ProxArgs& a, int64_t d0, const uint16_t* list, int total, int wave, int lane,
                                                int32_t mine, int L, int span, bool ordered, uint32_t* found) {
    const uint64_t cut = span == 64 ? ~0ull : (1ull << span) - 1ull;
    const bool exact = ordered && span == L;
    for (int c = wave; c < total; c += PX_WAVES) {       // one wave per candidate document (c is uniform in the wave)
        const int dl = __builtin_amdgcn_readfirstlane((int)list[c]);
        const int64_t d = d0 + dl;                       // < n_docs: the candidate word was masked
        const int64_t s = a.tok_off[d], e = a.tok_off[d + 1];
        int64_t pos = s + lane;
        const int32_t t_cur = pos < e ? a.tok_ids[pos] : -1;   // chunk 0 ...
        pos += 64;
        int32_t t_nxt = pos < e ? a.tok_ids[pos] : -1;   // ... and chunk 1: both loads are issued before the first ballot
        uint64_t cur[LM], nxt[LM];
#pragma unroll
        for (int j = 0; j < LM; ++j) {
            cur[j] = 0; nxt[j] = 0;
            if (j < L) cur[j] = __ballot(t_cur == __builtin_amdgcn_readlane(mine, j));
        }
        bool hit = false;
        for (int64_t b0 = s; b0 < e && !hit; b0 += 64) {
            pos += 64;
            const int32_t t_far = pos < e ? a.tok_ids[pos] : -1;   // the chunk after the next: in flight during the evaluation
            bool all = !ordered || cur[0] != 0;          // every term stands in the two chunks; ordered: a start in this one
#pragma unroll
            for (int j = 0; j < LM; ++j)
                if (j < L) {
                    nxt[j] = __ballot(t_nxt == __builtin_amdgcn_readlane(mine, j));
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
#pragma unroll
            for (int j = 0; j < LM; ++j) cur[j] = nxt[j];
            t_nxt = t_far;
        }
        if (hit && lane == 0) atomicOr(&found[dl >> 5], 1u << (dl & 31));
    }
}

__global__ __launch_bounds__(PX_THREADS) void proximity_sets_kernel(const ProxArgs a) {
    __shared__ uint32_t found[PX_THREADS];
    __shared__ uint16_t list[PX_SPAN];                   // the span's candidate documents (offset in the span), ascending
    __shared__ int32_t ph[PX_MAX];
    __shared__ int32_t wave_cnt[PX_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = a.row0 + (int)blockIdx.y;
    const int64_t d0 = (int64_t)blockIdx.x * PX_SPAN;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (d0 >> 5) + tid;                   // this thread's word of the row
    // the row: 1 .. PX_MAX ids inside [0, n_terms) and a span of 1 .. 64 tokens, else it is empty (the row's scalars are read
    // together, in front of the candidate word: one round trip, not one per array)
    const int32_t sel = a.n_cand > 0 ? a.row_cand[r] : -1;
    const int p0 = a.phrase_off[r], L = a.phrase_off[r + 1] - p0;
    const int span = a.row_span[r];
    const bool ordered = a.row_ordered[r] != 0;
    uint32_t acc = set_word(a.cand_bits, a.n_cand, a.cand_stride, sel, w, W, a.n_docs);
    int bad = (L < 1 || L > PX_MAX || span < 1 || span > MSR_PROX_MAX_SPAN);
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

    // compact the candidates: exclusive prefix of the words' popcounts (wave scan, then the four wave totals)
    const int cnt = __popc(acc);
    int incl = cnt;
    for (int s = 1; s < 64; s <<= 1) {
        const int v = __shfl_up(incl, s);
        if (lane >= s) incl += v;
    }
    if (lane == 63) wave_cnt[wave] = incl;
    found[tid] = 0;
    __syncthreads();
    int base = incl - cnt, total = 0;
    for (int i = 0; i < PX_WAVES; ++i) {
        if (i < wave) base += wave_cnt[i];
        total += wave_cnt[i];
    }
    for (uint32_t m = acc; m; m &= m - 1) list[base++] = (uint16_t)(tid * 32 + (__ffs(m) - 1));   // base + cnt <= PX_SPAN
    __syncthreads();

    // lane j holds term j; the scan reads it with a constant lane index: no LDS in the scan
    const int32_t mine = lane < L ? ph[lane] : -2;
    if (L <= 4) scan_candidates<4>(a, d0, list, total, wave, lane, mine, L, span, ordered, found);
    else if (L <= 8) scan_candidates<8>(a, d0, list, total, wave, lane, mine, L, span, ordered, found);
    else scan_candidates<PX_MAX>(a, d0, list, total, wave, lane, mine, L, span, ordered, found);
    __syncthreads();
    if (w < W) a.out_bits[(int64_t)r * a.out_stride + w] = found[tid];
}

constexpr int ROWS_PER_LAUNCH = 32768;                   // (the grid's y extent is 16 bits)

}  // namespace

hipError_t msr_proximity_sets_run(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_terms, int n_rows,
                                  const int32_t* phrase_off, const int32_t* phrase_terms, const int32_t* row_span,
                                  const int32_t* row_ordered, const uint32_t* cand_bits, int n_cand, int64_t cand_stride,
                                  const int32_t* row_cand, uint32_t* out_bits, int64_t out_stride, hipStream_t stream) {
    if (n_rows <= 0) return hipSuccess;
    const int64_t n_spans = (n_docs + PX_SPAN - 1) / PX_SPAN;
    if (n_spans <= 0) return hipSuccess;
    ProxArgs a{tok_off, tok_ids, n_docs, n_terms, phrase_off, phrase_terms, row_span, row_ordered, cand_bits, n_cand, cand_stride,
               row_cand, out_bits, out_stride, 0};
    for (int r0 = 0; r0 < n_rows; r0 += ROWS_PER_LAUNCH) {
        a.row0 = r0;
        const dim3 grid((unsigned)n_spans, (unsigned)std::min(ROWS_PER_LAUNCH, n_rows - r0));
        hipLaunchKernelGGL(proximity_sets_kernel, grid, dim3(PX_THREADS), 0, stream, a);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// What K11 - K14 share (msr_termset.hip, msr_phrase.hip, msr_proximity.hip, msr_snippet.hip): the ownership
// of a row's words, the candidate list of a span, the walk of one document's token stream, and the host loop over row slices --
// and what K11 shares with K17 (msr_facet.hip): a term's postings inside a span and their OR into the span's LDS bits.
// Every piece is a correctness rule with ONE definition here; what a kernel does with it stays in the kernel's file.
//
// Everything on the device side is a free __forceinline__ function over values and arrays that the CALLER declares, and the
// instruction streams are the ones of the hand-written loops (profiles/tokscan_shared_header.md).  Three other forms were
// tried and give OTHER kernels than the measured ones (K13 at 28 to 42 VGPRs and half the instructions, K14 with 36 bytes of
// scratch), so do not use them: the walker's cur[] / nxt[] as members of a struct; a callable per term (a lambda that
// captures the arrays is such a struct); the ballots of a chunk in a loop of their own, apart from the kernel's per-term
// summary -- which is why term_mask() makes one mask and the loop over j stays in the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"

namespace tokscan {

// ---- span ownership (K11, K12, K13) ---------------------------------------------------------------------------------------------
// One workgroup owns (row, span of SPAN consecutive documents): thread j owns word (d0 >> 5) + j of the row, loads it, and is
// the only one to store it -- plain stores of whole words, no global atomics, nothing to zero beforehand.
constexpr int SPAN = MSR_TERMSET_SPAN_DOCS;
constexpr int THREADS = SPAN / 32;                       // one word of the span per thread
constexpr int WAVES = THREADS / 64;
constexpr int MAX_TERMS = MSR_PHRASE_MAX_TERMS;
static_assert(THREADS >= 64 && THREADS <= 1024 && THREADS % 64 == 0, "one workgroup of whole waves per span");
static_assert(THREADS == 256, "the candidate compaction assumes four waves of 64");
static_assert(SPAN <= 65536, "a candidate's offset in its span is kept in 16 bits");
static_assert(MAX_TERMS <= 64, "lane j of a wave holds term j");
static_assert(MSR_PROX_MAX_SPAN == 64, "a window spans at most the current chunk and the next");

// word w (< W = ceil(n_docs / 32)) of the set of every document: the bits at or above n_docs stay zero in every output
__device__ __forceinline__ uint32_t tail_mask(int64_t w, int64_t W, int64_t n_docs) {
    return (w == W - 1 && (n_docs & 31)) ? (1u << (n_docs & 31)) - 1u : 0xFFFFFFFFu;
}

// the words of row_sel's set below n_docs: -1 (or no rows at all) = every document, a row of `bits`, anything else = empty
__device__ __forceinline__ uint32_t set_word(const uint32_t* bits, int32_t n_rows, int64_t stride, int32_t sel, int64_t w,
                                             int64_t W, int64_t n_docs) {
    if (w >= W) return 0;
    uint32_t acc = tail_mask(w, W, n_docs);
    if (n_rows > 0) {
        if (sel >= 0 && sel < n_rows) acc &= bits[(int64_t)sel * stride + w];
        else if (sel != -1) acc = 0;
    }
    return acc;
}

// ---- a term's postings inside a span (K11, K17) ---------------------------------------------------------------------------------
// [*lo, *hi): the postings of term t (a valid id) whose document lies in [d0, d0 + SPAN).  `a` is the kernel's argument struct:
// term_off, post_doc, heavy_id (nullable), tile_off and n_tiles of the bound postings (Bm25Index).  Two loads of the BM25 skip
// table for a long list, a binary search on post_doc otherwise.
static_assert(SPAN % MSR_BM25_TILE == 0, "a span is a whole number of skip-table tiles");
template <class Args>
__device__ __forceinline__ void span_postings(const Args& a, int32_t t, int64_t d0, int64_t* lo, int64_t* hi) {
    const int64_t p0 = a.term_off[t], p1 = a.term_off[t + 1];
    const int32_t h = a.heavy_id ? a.heavy_id[t] : -1;
    if (h >= 0) {
        const uint32_t* row = a.tile_off + (int64_t)h * (a.n_tiles + 1);
        const int32_t t0 = (int32_t)(d0 / MSR_BM25_TILE);
        const int32_t t1 = min(t0 + SPAN / MSR_BM25_TILE, a.n_tiles);
        *lo = p0 + row[t0];
        *hi = p0 + row[t1];
        return;
    }
    // first posting with document >= d0, then (from there on) the first with document >= d0 + SPAN
    int64_t l = p0, r = p1;
    while (l < r) {
        const int64_t m = l + ((r - l) >> 1);
        if (a.post_doc[m] < d0) l = m + 1; else r = m;
    }
    *lo = l;
    r = min(p1, l + SPAN);                               // documents ascend strictly: a span holds at most SPAN postings
    const int64_t d1 = d0 + SPAN;
    while (l < r) {
        const int64_t m = l + ((r - l) >> 1);
        if (a.post_doc[m] < d1) l = m + 1; else r = m;
    }
    *hi = l;
}

// bits |= the documents of postings [lo, hi) (all inside the span; the range test keeps a malformed table out of LDS)
__device__ __forceinline__ void or_postings(const int32_t* __restrict__ post_doc, int64_t lo, int64_t hi, int64_t d0,
                                            uint32_t* bits) {
    for (int64_t p = lo + threadIdx.x; p < hi; p += THREADS) {
        const int64_t d = (int64_t)post_doc[p] - d0;
        if (d >= 0 && d < SPAN) atomicOr(&bits[d >> 5], 1u << (d & 31));
    }
}

// ---- candidate compaction (K12, K13) --------------------------------------------------------------------------------------------
// The set bits of the workgroup's THREADS words `acc`, as offsets in the span, ascending, into list[0 .. total): exclusive prefix
// of the words' popcounts (wave scan, then the four wave totals).  found[] is zeroed on the way.  Two barriers: every thread of
// the workgroup calls this, and on return list, found and the total are visible to all.  base + cnt <= SPAN: the popcounts of
// THREADS words sum to at most 32 * THREADS, so no store leaves list[SPAN].
__device__ __forceinline__ int compact_candidates(uint32_t acc, int tid, int lane, int wave, uint32_t* found, uint16_t* list,
                                                  int32_t* wave_cnt) {
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
    for (int i = 0; i < WAVES; ++i) {
        if (i < wave) base += wave_cnt[i];
        total += wave_cnt[i];
    }
    for (uint32_t m = acc; m; m &= m - 1) list[base++] = (uint16_t)(tid * 32 + (__ffs(m) - 1));
    __syncthreads();
    return total;
}

// ---- chunk walker (K13, K14) ----------------------------------------------------------------------------------------------------
// One wave walks document [s, e) of the forward index in chunks of 64 tokens, lane l = position b0 + l, one coalesced 256-byte
// load per chunk, no dependent load and no LDS.  Lane j holds term j of the row in `mine` (a lane without one holds -2); per
// chunk and term j one __ballot(tok == term j) gives a wave-uniform 64-bit mask.  The masks of the current chunk (cur[]) and of
// the next (nxt[]) are kept -- span <= 64: two chunks hold every window that starts in the current one -- and the load of the
// chunk after the next is in flight while the current one is evaluated.  The loops over j are unrolled to LM, so that every
// mask has a register of its own: 2 LM wave-uniform 64-bit masks are alive at once.  A kernel's loop reads
//
//     uint64_t cur[LM], nxt[LM];  int64_t pos;  int32_t t_nxt;
//     walk_start<LM>(tok_ids, s, e, lane, mine, L, cur, nxt, pos, t_nxt);
//     for (int64_t b0 = s; b0 < e; b0 += 64) {
//         const int32_t t_far = load_token(tok_ids, pos += 64, e);
//         for j < LM, unrolled:  if (j < L) { nxt[j] = term_mask(t_nxt, mine, j);  ... the kernel's own summary of term j ... }
//         ... evaluate the starts of chunk b0 from view(cur[j], nxt[j], lane) & window_cut(span) ...
//         walk_roll<LM>(cur, nxt, t_nxt, t_far);
//     }

// THE BOUND OF EVERY READ IS THE DOCUMENT'S END e = tok_off[d + 1]: a lane at or past it loads nothing and holds -1, which
// equals no term of a valid row, so a window never leaves the document and the last document never reads past the buffer.
__device__ __forceinline__ int32_t load_token(const int32_t* tok_ids, int64_t pos, int64_t e) {
    return pos < e ? tok_ids[pos] : -1;
}

// the lanes of the chunk whose token is term j (wave-uniform; j is a constant once the caller's loop is unrolled, and every
// lane of the wave calls this)
__device__ __forceinline__ uint64_t term_mask(int32_t tok, int32_t mine, int j) {
    return __ballot(tok == __builtin_amdgcn_readlane(mine, j));
}

// chunks 0 and 1 are loaded (both loads are issued before the first ballot), cur[] holds chunk 0, nxt[] is zero, t_nxt chunk 1
template <int LM>
__device__ __forceinline__ void walk_start(const int32_t* tok_ids, int64_t s, int64_t e, int lane, int32_t mine, int L,
                                           uint64_t (&cur)[LM], uint64_t (&nxt)[LM], int64_t& pos, int32_t& t_nxt) {
    pos = s + lane;
    const int32_t t_cur = load_token(tok_ids, pos, e);
    pos += 64;
    t_nxt = load_token(tok_ids, pos, e);
#pragma unroll
    for (int j = 0; j < LM; ++j) {
        cur[j] = 0; nxt[j] = 0;
        if (j < L) cur[j] = term_mask(t_cur, mine, j);
    }
}

// the end of an iteration: the next chunk becomes the current one
template <int LM>
__device__ __forceinline__ void walk_roll(uint64_t (&cur)[LM], const uint64_t (&nxt)[LM], int32_t& t_nxt, int32_t t_far) {
#pragma unroll
    for (int j = 0; j < LM; ++j) cur[j] = nxt[j];
    t_nxt = t_far;
}

// This lane's view of a term is the 128-bit pair (nxt, cur) shifted right by the lane: bit k = the term stands at (chunk start
// + lane + k).  A shift by 64 is undefined, so lane 0 takes cur.
__device__ __forceinline__ uint64_t view(uint64_t cur, uint64_t nxt, int lane) {
    return lane ? (cur >> lane) | (nxt << (64 - lane)) : cur;
}

// the low `span` bits (1 <= span <= 64): a view cut to the window that starts at the lane's position
__device__ __forceinline__ uint64_t window_cut(int span) { return span == 64 ? ~0ull : (1ull << span) - 1ull; }

// ---- row slices (host) ----------------------------------------------------------------------------------------------------------
constexpr int ROWS_PER_LAUNCH = 32768;                   // (the grid's y extent is 16 bits)

inline int64_t span_count(int64_t n_docs) { return (n_docs + SPAN - 1) / SPAN; }

// kernel<<<(grid_x, rows of the slice), threads>>>(a) for slices of at most ROWS_PER_LAUNCH rows, a.row0 = the slice's first row
// (the kernel's row is row0 + blockIdx.y).  Nothing to do (no rows, or a grid without a column) is a success.
template <class Args>
hipError_t launch_rows(void (*kernel)(Args), int64_t grid_x, int threads, int n_rows, Args a, hipStream_t stream) {
    if (grid_x <= 0) return hipSuccess;
    for (int r0 = 0; r0 < n_rows; r0 += ROWS_PER_LAUNCH) {
        a.row0 = r0;
        const dim3 grid((unsigned)grid_x, (unsigned)std::min(ROWS_PER_LAUNCH, n_rows - r0));
        hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, stream, a);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace tokscan

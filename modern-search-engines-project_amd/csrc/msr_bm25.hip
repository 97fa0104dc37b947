// K1 -- BM25 term-at-a-time scoring over HBM-resident CSR postings (gfx950).
//
// Replaces the per-query SQL fetch + Python grouping + scoring loop of the reference
// (indexer/bm25_indexer.py:434-481).  The dense doc index is cut into tiles of TILE documents; a WAVE scores one query
// over a span of up to 8 consecutive tiles in ONE pass: it marks the span's touched documents in an LDS bitmap, ranks them,
// and accumulates in float64 slots indexed by a document's RANK among the touched documents of the span -- a few hundred
// slots cover 8192 documents.  Waves are independent: no workgroup barrier anywhere.
//
// What is streamed and what is looked up.  A posting is read as {doc, tf_component} (12 bytes): the tf_component
// (tf (k1 + 1)) / (tf + k1 (1 - b + b dl / avgdl)) (:473-475) depends on (tf, document) only and is evaluated ONCE at bind
// time with the reference's own operations (bm25_post_comp_kernel), so the kernel neither divides nor looks a length up.
// A term whose idf is NEGATIVE (document frequency above half the corpus: the city term that search_api.py:160-164 puts
// into every query) can only lower a score: every one of its contributions (idf * tf_component) * qtf is < 0.  With
// min_score >= 0 (:480) a document matched by such terms alone is never a candidate, so their lists -- 96 % of the
// postings a benchmark query names -- are not streamed at all: the candidates are the documents touched by the OTHER terms
// ("streamed" terms), and a negative term's contribution to one of them is looked up in a dense per-document table of its
// tf_components (built at bind for the long negative lists, 8 B per document).  With min_score < 0, or for a negative
// term without a table, every list is streamed; the result is the same either way, bit for bit.
//
// Summation order.  The reference adds the contributions of a document's terms in the query's first-occurrence order
// (:466-478) in float64.  Every slot starts at 0.0 (:466) and the wave walks its query's terms in that order:
//   streamed term j: for each posting of the span, acc[rank] += (idf * tfc) * qtf as an LDS read-modify-write (a wave's
//     LDS operations execute in order; a document occurs at most once per list, PRIMARY KEY (doc_id, term) :100-104, so
//     the lanes of a step hold distinct slots: no atomics);
//   looked-up term i: for every slot, acc[rank] += (idf * table_i[document of the slot]) * qtf if the table has it.
// So every candidate's sum is the reference's sum operation by operation; this file is compiled with -ffp-contract=off.
//
// Phases of a (query, span) wave, each over the WHOLE span with all its loads in flight:
//   plan    where each term's slice of the span is: the two ends of a skip-table row segment for long lists, the whole list
//           for <= 64 postings, ONE round of 64 probes for the lists in between; lane-parallel (lane j = term j);
//   load    the slices in chunks of 64 postings; the first BM25_RES chunks stay in registers, a span with more re-reads the
//           rest in each later phase;
//   mark    one bit per document (LDS atomic OR);   rank  pre[w] = touched documents below bitmap word w (one wave scan),
//           rank(d) = pre[d / 32] + popcount(bits of the word below d), slot[rank] = d: the slots are in document order;
//   gather  the table values of the looked-up terms need only slot[]: issued here, ahead of the accumulation;
//   accumulate in query order, as above;   emit  the slots with score >= min_score (:480), ballot-compacted.
// Rounds: there are MSR_BM25_ROUND_CAP slots.  A span that touches more (min_score < 0, untabled negative lists, dense
// positive lists) runs rank .. emit in rounds over consecutive whole bitmap words; a word joins the round while the touched
// count up to its end fits, so every rank is below the cap by construction.  One round is the common case and pays only
// wave-uniform branches for the general one.
//
// Output: the candidates of a (query, span) go to a segment of the query's candidate row that belongs to that wave alone
// -- no atomics, no counters to clear; the top-k select (msr_topk.hip) walks the segments.
//
// HBM traffic per query: 12 B per posting of its streamed terms + 8 B per (touched document, looked-up term) from tables
// that stay in the L2 / Infinity Cache + 12 B per candidate (the (score, doc) list consumed by the top-k select).
#include <stdio.h>

#include "msr_common.h"
#include "msr_internal.h"

namespace {

constexpr int BM25_TILE = MSR_BM25_TILE;
#ifndef BM25_WPW
#define BM25_WPW 1                                             // one-wave workgroups: work items differ by an order of magnitude (a long
#endif                                                         // positive list or not) and a workgroup holds its LDS until its slowest
constexpr int BM25_WAVES = BM25_WPW;                          // wave is done (measured per 256 queries: 1 wave 0.23 ms, 2 waves 0.32)
constexpr int BM25_THREADS = 64 * BM25_WAVES;
constexpr int BM25_TPW = 8;                                   // at most this many consecutive tiles per work item
constexpr int BM25_MAX_TERMS = 64;                            // MSR_MAX_QUERY_TERMS: one lane per term
constexpr int BM25_CAP = MSR_BM25_ROUND_CAP;                  // rank-indexed accumulators: the touched documents of one round
constexpr int BM25_RES = 4;                                   // R: 64-posting chunks of a span held in registers (measured, per 256
                                                              // queries: R = 4 0.19 ms, 6 0.20, 8 0.20, 12 0.29 with scratch)
#ifndef BM25_U
#define BM25_U 4                                               // chunks per step of the postings beyond the resident ones (8: 0.20-0.23)
#endif
#ifndef BM25_UM
#define BM25_UM 8                                              // the same in the mark phase, which reads the documents only (4, 8
#endif                                                         // and 16 measure the same)
constexpr int BM25_WORDS = BM25_TPW * BM25_TILE / 32;         // the span's bitmap: one bit per document
static_assert(BM25_WORDS == 4 * 64, "four bitmap words per lane");
static_assert(BM25_CAP % 128 == 0 && BM25_CAP >= 128 && BM25_CAP <= BM25_TILE, "whole batches of slots; a word (32) always fits");

// Between two phases of a wave that hand values from lane to lane through LDS: a wave's LDS operations execute in order, so
// this emits no instruction; it only keeps the compiler from moving LDS accesses across the phase boundary.
__device__ __forceinline__ void lds_phase() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int64_t lane_i64(int64_t v, int j) {          // v of lane j (j wave-uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), j);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double lane_f64(double v, int j) {
    return __longlong_as_double(lane_i64(__double_as_longlong(v), j));
}
__device__ __forceinline__ int lane_rank(unsigned long long m) {         // number of set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// one posting = one 12-byte load
__device__ __forceinline__ double post_comp(const Bm25Post& x) { return __hiloint2double((int)x.comp_hi, (int)x.comp_lo); }
// a table row as a GLOBAL pointer: rebuilt from the integer a lane carries it would be a flat pointer, and flat loads return
// out of order -- every one of them makes the wave wait for ALL its outstanding memory operations (vmcnt(0) + lgkmcnt(0))
typedef const __attribute__((address_space(1))) double* gtable;
__device__ __forceinline__ gtable table_of(int64_t bits) { return (gtable)(uint64_t)bits; }

enum : int { K_DEAD = 0, K_LOOKUP = 1, K_HEAVY = 2, K_RANGE = 3 };

// What the scoring kernel does with one term of a query -- shared by the kernel's plan phase and by bm25_plan_kernel, which
// weighs a query by the postings the scoring kernel will stream for it: the two must agree on which lists those are.
// K_DEAD: unknown term or empty list; K_LOOKUP: every contribution < 0 and a dense table exists (looked up, never streamed);
// K_HEAVY: streamed, its slice of a span comes from skip-table row h; K_RANGE: streamed, short or probed.
struct Bm25Term {
    int klass, dh, h;                                // dh: row of the dense tables, h: row of the skip table (or -1)
    int64_t s, e;                                    // the posting list
    double idf, qtf;
};
__device__ __forceinline__ Bm25Term bm25_classify(const Bm25Index& ix, int32_t t, int32_t qtf, bool prune) {
    Bm25Term r{K_DEAD, -1, -1, 0, 0, 0.0, 0.0};
    if (t < 0 || t >= ix.n_terms) return r;
    r.s = ix.term_off[t];                            // (the five loads of a known term are independent: one round trip)
    r.e = ix.term_off[t + 1];
    const double idf = (double)ix.idf[t];
    const int dh = prune ? ix.dense_id[t] : -1;
    const int h = ix.heavy_id ? ix.heavy_id[t] : -1;
    if (r.e <= r.s) return r;
    r.idf = idf;
    r.qtf = (double)qtf;
    r.dh = dh;
    r.h = h;
    r.klass = dh >= 0 && idf < 0.0 && r.qtf > 0.0 ? K_LOOKUP : (h >= 0 ? K_HEAVY : K_RANGE);
    return r;
}
// prune: a negative term's list need not be streamed when nothing below 0 can be a candidate (:480)
__device__ __forceinline__ bool bm25_prune(const Bm25Index& ix, double min_score) {
    return min_score >= 0.0 && ix.dense_id != nullptr;
}

#ifndef BM25_WPE
#define BM25_WPE 4                                             // waves per SIMD the register budget is cut for (5 and 6, with a cap
#endif                                                         // of 640 / 512 and no scratch, measure within 3 % of 4)
// Set: empty (the unrestricted kernel) or one MsrSetView (msr_bm25_topk_within): a touched document outside the query's set is
// not emitted.  Only the emission at the end of a round differs; the scores are the same operations either way.
template <typename... Set>
__global__ __launch_bounds__(BM25_THREADS) __attribute__((amdgpu_waves_per_eu(BM25_WPE, BM25_WPE))) void bm25_taat_kernel(Bm25Index ix,
                                                                  const int32_t* __restrict__ q_term_off,
                                                                  const int32_t* __restrict__ q_terms,
                                                                  const int32_t* __restrict__ q_qtf,
                                                                  int q_first, int nq, double min_score, int tpw, int n_spans,
                                                                  double* __restrict__ cand_score,
                                                                  int32_t* __restrict__ cand_doc,
                                                                  int32_t* __restrict__ seg_n,
                                                                  const int32_t* __restrict__ order, int dbg_arg, Set... set) {
#ifdef MSR_DIAG
    const int dbg = dbg_arg;   // timing experiments (wrong results): 1 no table gathers, 2 no accumulation of streamed postings,
                               // 4 nothing read beyond the resident chunks, 16 no emission, 64 stream every list (no pruning);
                               // 8 (the parent's "no prefetch") is retired: the resident chunks are the only first read there is
#else
    constexpr int dbg = 0;
#endif
    __shared__ __attribute__((aligned(16))) double acc_all[BM25_WAVES][BM25_CAP];      // by rank inside the round
    __shared__ __attribute__((aligned(16))) uint32_t bits_all[BM25_WAVES][BM25_WORDS];   // one bit per document of the span
    __shared__ uint16_t pre_all[BM25_WAVES][BM25_WORDS];                               // touched documents below each word
    __shared__ uint16_t slot_all[BM25_WAVES][BM25_CAP];                                // rank -> document (span-relative)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // work item = (query, span of tiles), the query running fastest: the waves of a workgroup and of its neighbours score the
    // SAME tiles for different queries, so the table lines and the slices of terms the queries share come from the L2.
    // LONG ITEMS FIRST: the items of a slice differ by an order of magnitude (a query with a long positive list streams dozens
    // of chunks per span, a typical one fits the resident chunks) and the kernel ends with its last long item, so the items of
    // the n_heavy = order[nq] queries that stream more than the resident chunks per span (bm25_plan_kernel: order[] = the
    // queries by descending weight) come first, span-major among themselves, then those of the other queries, span-major:
    // the long items start while the grid is full and the short ones fill in behind them.  Two scalar loads per wave.
    const int item = (int)blockIdx.x * BM25_WAVES + wave;
    if (item >= nq * n_spans) return;                          // (wave-uniform; there is no barrier in this kernel)
    const int n_heavy = order[nq], heavy_items = n_heavy * n_spans;
    int span, qj;
    if (item < heavy_items) {
        span = item / n_heavy;
        qj = item - span * n_heavy;
    } else {
        const int n_light = nq - n_heavy, r = item - heavy_items;
        span = r / n_light;
        qj = n_heavy + (r - span * n_light);
    }
    const int q = order[qj];                                   // q: row of the candidate lists
    // The candidates of this item go to segment `span` of row q of the candidate arrays: positions [span tpw TILE, ...) of
    // the row belong to this wave alone (a span cannot yield more candidates than it has documents), so nothing is reserved
    // with an atomic; the segment's length is written once, at the end.
    int32_t* seg_len = seg_n + (int64_t)q * n_spans + span;
    int seg_cnt = 0;
    constexpr bool WITHIN = sizeof...(Set) > 0;
    MsrSetRow srow{nullptr, 0};                                // the query's set (wave-uniform: one query per wave)
    if constexpr (WITHIN) {
        srow = msr_set_row(q_first + q, set...);
        if (srow.mode == 2) {                                  // the empty set: no candidate
            if (lane == 0) *seg_len = 0;
            return;
        }
    }
    const int tile0 = span * tpw;                              // this wave's tiles: tile0 .. tile0 + n_my - 1
    const int n_my = tile0 + tpw <= ix.n_tiles ? tpw : ix.n_tiles - tile0;
    double* acc = acc_all[wave];
    uint32_t* bits = bits_all[wave];
    uint16_t* pre = pre_all[wave];
    uint16_t* slot = slot_all[wave];
    // the span's documents: [lo_span, lo_span + n_span), n_span <= 8192
    const int64_t lo_span = (int64_t)tile0 * BM25_TILE;
    const int64_t hi_span = lo_span + (int64_t)n_my * BM25_TILE < ix.n_docs ? lo_span + (int64_t)n_my * BM25_TILE : ix.n_docs;
    const uint32_t n_span = (uint32_t)(hi_span - lo_span);
    // a negative term's list need not be streamed when nothing below 0 can be a candidate (:480)
    const bool prune = bm25_prune(ix, min_score) && !(dbg & 64);
    // ---- 1. the query's plan, ONCE for the span; lane j = term j ----
    int nt = 0, klass = K_DEAD;
    int64_t s_v = 0;                                 // long list: its first posting; looked-up term: its table row
    int h_v = -1;                                    // long list: its row of the skip table
    int64_t ps_v = 0, pe_v = 0;                      // streamed list: the postings to look at for the whole span
    double idf_v = 0.0, qtf_v = 0.0;
    bool medium = false;
    {
        const int t0 = q_term_off[q_first + q];
        nt = q_term_off[q_first + q + 1] - t0;
        if (nt > BM25_MAX_TERMS) nt = BM25_MAX_TERMS;        // the host never sends more
        if (lane < nt) {
            const Bm25Term tm = bm25_classify(ix, q_terms[t0 + lane], q_qtf[t0 + lane], prune);
            klass = tm.klass;
            idf_v = tm.idf;
            qtf_v = tm.qtf;
            if (klass == K_LOOKUP) {                         // every contribution < 0: looked up, never streamed
                s_v = (int64_t)(ix.dense_comp + (int64_t)tm.dh * ix.dense_stride);
            } else if (klass == K_HEAVY) {                   // long list: the span's slice comes from the skip table, the
                s_v = tm.s;                                  // two ends of one row segment
                h_v = tm.h;
                const uint32_t* row = ix.tile_off + (int64_t)tm.h * (ix.n_tiles + 1) + tile0;
                ps_v = tm.s + row[0];
                pe_v = tm.s + row[n_my];
            } else if (klass == K_RANGE) {
                ps_v = tm.s;                                 // short list: all of it (postings of other spans are masked)
                pe_v = tm.e;
                medium = tm.e - tm.s > 64;
            }
        }
    }
    const unsigned long long look_mask = __ballot(klass == K_LOOKUP);
    const unsigned long long stream_mask = __ballot(klass >= K_HEAVY);
    if (stream_mask == 0) {                          // no streamed term: no document can reach min_score (or no known term)
        if (lane == 0) *seg_len = 0;
        return;
    }
    const int64_t seg_base = (int64_t)q * ix.n_docs + lo_span;
    // ---- 2. lists of 65 .. HEAVY_DF-1 postings: one round of 64 probes narrows [ps, pe) to the chunks that can hold
    //         documents of the span; MED lists side by side (the probes are independent loads) ----
    {
        const int64_t lo8 = lo_span, hi8 = hi_span;
        constexpr int MED = 4;
        unsigned long long todo = __ballot(medium);
        while (todo) {
            int jj[MED];
            int64_t s_[MED], e_[MED], ch_[MED];
            int32_t probe[MED];
#pragma unroll
            for (int m = 0; m < MED; ++m) {
                jj[m] = todo ? __ffsll((long long)todo) - 1 : -1;
                if (todo) todo &= todo - 1;
                probe[m] = 0; s_[m] = e_[m] = ch_[m] = 0;
                if (jj[m] >= 0) {                            // wave-uniform
                    s_[m] = lane_i64(ps_v, jj[m]);
                    e_[m] = lane_i64(pe_v, jj[m]);
                    ch_[m] = (e_[m] - s_[m] + 63) >> 6;
                    int64_t idx = s_[m] + (int64_t)(lane + 1) * ch_[m] - 1;     // last posting of chunk `lane`
                    if (idx > e_[m] - 1) idx = e_[m] - 1;
                    probe[m] = ix.post[idx].doc;
                }
            }
#pragma unroll
            for (int m = 0; m < MED; ++m) {
                if (jj[m] < 0) continue;                     // wave-uniform
                const unsigned long long ge_lo = __ballot((int64_t)probe[m] >= lo8);
                const unsigned long long ge_hi = __ballot((int64_t)probe[m] >= hi8);
                int64_t ps = e_[m], pe = e_[m];              // nothing >= lo: empty
                if (ge_lo) {
                    ps = s_[m] + (int64_t)(__ffsll((long long)ge_lo) - 1) * ch_[m];
                    if (ps > e_[m]) ps = e_[m];
                    if (ge_hi) {
                        pe = s_[m] + (int64_t)(__ffsll((long long)ge_hi)) * ch_[m];
                        if (pe > e_[m]) pe = e_[m];
                    }
                }
                if (lane == jj[m]) { ps_v = ps; pe_v = pe; }
            }
        }
    }
    // ---- 3. the span's postings.  The slices of the streamed terms, in query order, are cut into chunks of 64 postings (a
    //         chunk belongs to one term: its lanes hold distinct documents).  The first R chunks stay in registers for the
    //         whole item (indexed by constants only); a span with more re-reads the rest in every later phase (the L2 has
    //         them).  All R loads are issued unconditionally, back to back: a lane without a posting, and a chunk that does
    //         not exist, load the sentinel {doc -1, 0.0} the bind step put behind the last posting. ----
    const int64_t null_post = ix.n_postings;
    int cj[BM25_RES];                                          // (wave-uniform) the chunk's term, -1: no such chunk
    int64_t cps[BM25_RES], cpe[BM25_RES];                      // its first posting, the end of its term's slice
    {
        unsigned long long m = stream_mask;
        int j = -1;
        int64_t pos = 0, pe = 0;
#pragma unroll
        for (int k = 0; k < BM25_RES; ++k) {
            while (pos >= pe && m) {
                j = __ffsll((long long)m) - 1;
                m &= m - 1;
                pos = lane_i64(ps_v, j);
                pe = lane_i64(pe_v, j);
            }
            if (pos < pe) { cj[k] = j; cps[k] = pos; cpe[k] = pe; pos += 64; }
            else { cj[k] = -1; cps[k] = null_post; cpe[k] = null_post; }
        }
    }
    if (cj[0] < 0) {                                 // no streamed term has a posting near this span
        if (lane == 0) *seg_len = 0;
        return;
    }
    Bm25Post res[BM25_RES];
#pragma unroll
    for (int k = 0; k < BM25_RES; ++k) {
        const int64_t i = cps[k] + lane;
        res[k] = ix.post[i < cpe[k] ? i : null_post];
    }
    int64_t rs_v = ps_v;                             // lane j: where term j's postings beyond the resident chunks start
#pragma unroll
    for (int k = 0; k < BM25_RES; ++k)
        if (cj[k] >= 0 && lane == cj[k]) rs_v = cps[k] + 64 < cpe[k] ? cps[k] + 64 : cpe[k];
    const bool has_rest = __ballot(klass >= K_HEAVY && rs_v < pe_v) != 0 && !(dbg & 4);      // (wave-uniform)
    constexpr int U = BM25_U;
    // ---- 4. mark: one bit per document of the span that a streamed posting names.  From here on a resident posting carries
    //         its document relative to the span, or -1 (no posting, or a document of another span). ----
    ((uint4*)bits)[lane] = make_uint4(0u, 0u, 0u, 0u);
    lds_phase();
#pragma unroll
    for (int k = 0; k < BM25_RES; ++k) {
        const uint32_t d = (uint32_t)(res[k].doc - (int32_t)lo_span);
        const bool ok = d < n_span;
        if (ok) atomicOr(&bits[d >> 5], 1u << (d & 31));
        res[k].doc = ok ? (int32_t)d : -1;
    }
    if (has_rest) {
        // the postings [rs, pe) of every streamed term beyond the resident chunks: only their documents are read here, UM x 64
        // per step, all loads of a step issued before the first is used
        constexpr int UM = BM25_UM;
        unsigned long long m = __ballot(klass >= K_HEAVY && rs_v < pe_v);
        while (m) {
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int64_t a = lane_i64(rs_v, j), b = lane_i64(pe_v, j);
            for (int64_t at = a; at < b; at += (int64_t)UM * 64) {
                int32_t pd[UM];
#pragma unroll
                for (int u = 0; u < UM; ++u) {
                    const int64_t i = at + lane + (int64_t)u * 64;
                    pd[u] = ix.post[i < b ? i : null_post].doc;
                }
#pragma unroll
                for (int u = 0; u < UM; ++u) {
                    const uint32_t d = (uint32_t)(pd[u] - (int32_t)lo_span);
                    if (d < n_span) atomicOr(&bits[d >> 5], 1u << (d & 31));
                }
            }
        }
    }
    lds_phase();
    // ---- 5. pre[w] = touched documents below word w (one wave scan over four words per lane) ----
    int total;
    {
        const uint4 w4 = ((const uint4*)bits)[lane];
        const int p0 = __popc(w4.x), p1 = __popc(w4.y), p2 = __popc(w4.z), p3 = __popc(w4.w);
        int incl = p0 + p1 + p2 + p3;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const int ex = incl - (p0 + p1 + p2 + p3);
        pre[4 * lane + 0] = (uint16_t)ex;
        pre[4 * lane + 1] = (uint16_t)(ex + p0);
        pre[4 * lane + 2] = (uint16_t)(ex + p0 + p1);
        pre[4 * lane + 3] = (uint16_t)(ex + p0 + p1 + p2);
        total = __builtin_amdgcn_readlane(incl, 63);
    }
    lds_phase();
    // The rank of span document d inside the round that covers the bitmap words [w0, w1) and starts at rank `base` of the
    // span, or -1 for "no posting" and for a document of another round.  It is below the round's touched count, which the
    // round cut keeps at or below BM25_CAP: that bound, not a clamp, is what keeps the LDS indices inside the arrays.
    auto rank_of = [&](int32_t doc, int w0, int w1, int base) -> int {
        const bool ok = doc >= 0;
        const uint32_t d = ok ? (uint32_t)doc : 0u;
        const uint32_t wd = d >> 5;
        const int r = (int)pre[wd] - base + __popc(bits[wd] & ((1u << (d & 31)) - 1u));
        return ok && (int)wd >= w0 && (int)wd < w1 ? r : -1;
    };
    // ---- 6. rounds.  A span's touched documents nearly always fit one round (w0 = 0, w1 = all words, base = 0).  Otherwise
    //         a round takes consecutive whole words while their touched count stays within BM25_CAP: a word has at most 32,
    //         so a round always advances.  Every branch on `multi` is wave-uniform. ----
    const bool multi = total > BM25_CAP;
    int w0 = 0, base = 0;
    while (w0 < BM25_WORDS) {
        int w1 = BM25_WORDS, cnt = total;
        int64_t rs_r = rs_v, pe_r = pe_v;
        if (multi) {
            const uint4 w4 = ((const uint4*)bits)[lane];
            const int lim = base + BM25_CAP;                 // a word belongs to the round if the count up to its END fits
            w1 = __popcll(__ballot((int)pre[4 * lane + 0] + __popc(w4.x) <= lim)) +
                 __popcll(__ballot((int)pre[4 * lane + 1] + __popc(w4.y) <= lim)) +
                 __popcll(__ballot((int)pre[4 * lane + 2] + __popc(w4.z) <= lim)) +
                 __popcll(__ballot((int)pre[4 * lane + 3] + __popc(w4.w) <= lim));
            cnt = __builtin_amdgcn_readfirstlane((int)pre[w1 - 1] + __popc(bits[w1 - 1])) - base;
            if (klass == K_HEAVY) {                          // a long list: only its postings of the round's tiles
                const int t_lo = w0 >> 5, t_hi = ((w1 + 31) >> 5) < n_my ? ((w1 + 31) >> 5) : n_my;
                const uint32_t* row = ix.tile_off + (int64_t)h_v * (ix.n_tiles + 1) + tile0;
                const int64_t a = s_v + row[t_lo], b = s_v + row[t_hi];
                rs_r = rs_v > a ? rs_v : a;
                pe_r = pe_v < b ? pe_v : b;
                if (rs_r > pe_r) rs_r = pe_r;
            }
        }
        if (cnt > 0) {
            // ---- 6a. rank: a resident posting of the round keeps its rank in a register; slot[rank] = document, so the
            //          slots are in document order ----
            int rk[BM25_RES];
#pragma unroll
            for (int k = 0; k < BM25_RES; ++k) {
                rk[k] = rank_of(res[k].doc, w0, w1, base);
                if (rk[k] >= 0) slot[rk[k]] = (uint16_t)res[k].doc;
            }
            if (has_rest) {
                // postings beyond the resident chunks: their slots come from the bitmap, not from another pass over the
                // postings -- lane l takes the words w0 + l, w0 + l + 64, ...; a word's documents get the ranks from
                // pre[w] - base on, all below cnt
                for (int w = w0 + lane; w < w1; w += 64) {
                    uint32_t x = bits[w];
                    int r = (int)pre[w] - base;
                    while (x) {
                        slot[r++] = (uint16_t)(32 * w + __ffs((int)x) - 1);
                        x &= x - 1;
                    }
                }
            }
            lds_phase();
            // ---- 6b. the table values of the first LK looked-up terms for the first LG x 64 slots: the gathers need only
            //          slot[], so they are all issued here, ahead of the accumulation, whatever the term's position ----
            constexpr int LK = 2, LG = 6;
            double tv[LK][LG];
#pragma unroll
            for (int l = 0; l < LK; ++l)
#pragma unroll
                for (int g = 0; g < LG; ++g) tv[l][g] = 0.0;
            if (look_mask && !(dbg & 1)) {
                uint32_t sd[LG];
#pragma unroll
                for (int g = 0; g < LG; ++g) sd[g] = slot[g * 64 + lane < cnt ? g * 64 + lane : 0];
                unsigned long long lm = look_mask;
#pragma unroll
                for (int l = 0; l < LK; ++l) {
                    if (!lm) break;
                    const int i = __ffsll((long long)lm) - 1;
                    lm &= lm - 1;
                    const gtable tbl = table_of(lane_i64(s_v, i)) + lo_span;
#pragma unroll
                    for (int g = 0; g < LG; ++g)
                        if (g * 64 < cnt) tv[l][g] = tbl[sd[g]];     // (wave-uniform; a lane past cnt reads slot 0's entry)
                }
            }
            // ---- 6c. accumulate in query order: bm25_score = 0.0 (:466), then the terms' contributions (:478) ----
            for (int s = 2 * lane; s < cnt; s += 128) *(double2*)(acc + s) = make_double2(0.0, 0.0);
            lds_phase();
            // looked-up term i: its contribution to every slot of the round whose document has the term
            auto lookup = [&](int i) {
                if (dbg & 1) return;
                const double idf = lane_f64(idf_v, i), qtf = lane_f64(qtf_v, i);
                const int li = __popcll(look_mask & ((1ull << i) - 1ull));
                int from = 0;
                if (li < LK) {
#pragma unroll
                    for (int l = 0; l < LK; ++l) {
                        if (li != l) continue;               // wave-uniform
#pragma unroll
                        for (int g = 0; g < LG; ++g) {
                            if (g * 64 >= cnt) break;        // wave-uniform
                            const int s = g * 64 + lane;
                            double t = tv[l][g];
                            // the gathered value is first looked at HERE: without this the compiler hoists the select and
                            // the compare below out of the term loop, and with them the wait for every gather
                            asm volatile("" : "+v"(t));
                            const double tc = s < cnt ? t : 0.0;
                            if (tc != 0.0) acc[s] = acc[s] + (idf * tc) * qtf;       // (0.0: the document lacks term i)
                        }
                    }
                    from = LG * 64;
                }
                if (from >= cnt) return;
                const gtable tbl = table_of(lane_i64(s_v, i)) + lo_span;
                for (int b = from; b < cnt; b += LG * 64) {  // LG batches of gathers in flight
                    double tc[LG];
#pragma unroll
                    for (int g = 0; g < LG; ++g) {
                        const int s = b + g * 64 + lane;
                        tc[g] = tbl[slot[s < cnt ? s : 0]];
                    }
#pragma unroll
                    for (int g = 0; g < LG; ++g) {
                        const int s = b + g * 64 + lane;
                        if (s < cnt && tc[g] != 0.0) acc[s] = acc[s] + (idf * tc[g]) * qtf;
                    }
                }
            };
            for (int j = 0; j < nt; ++j) {
                const int kj = __builtin_amdgcn_readlane(klass, j);
                if (kj == K_DEAD) continue;
                if (kj == K_LOOKUP) { lookup(j); continue; }
                // streamed term j: acc[rank] += (idf * tf_component) * qtf, a plain LDS read-modify-write (the lanes of a
                // step hold distinct documents; a wave's LDS operations execute in order)
                const double idf = lane_f64(idf_v, j), qtf = lane_f64(qtf_v, j);
#pragma unroll
                for (int k = 0; k < BM25_RES; ++k) {
                    if (cj[k] != j) continue;                // wave-uniform
                    const double c = (idf * post_comp(res[k])) * qtf;
                    if (rk[k] >= 0 && !(dbg & 2)) acc[rk[k]] = acc[rk[k]] + c;
                }
                const int64_t a = lane_i64(rs_r, j), b = lane_i64(pe_r, j);
                if (a >= b || (dbg & 4)) continue;
                for (int64_t at = a; at < b; at += (int64_t)U * 64) {
                    int32_t pd[U];
                    double pc[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t i = at + lane + (int64_t)u * 64;
                        const Bm25Post x = ix.post[i < b ? i : null_post];
                        pd[u] = x.doc; pc[u] = post_comp(x);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t d = (uint32_t)(pd[u] - (int32_t)lo_span);
                        const int r = rank_of(d < n_span ? (int32_t)d : -1, w0, w1, base);
                        const double c = (idf * pc[u]) * qtf;
                        if (r >= 0 && !(dbg & 2)) acc[r] = acc[r] + c;
                    }
                }
            }
            lds_phase();
            // ---- 6d. the round's candidates: the slots with score >= min_score (:461,480) as (score, doc) pairs appended
            //          to the item's segment, in document order ----
            for (int b = 0; b < cnt; b += 64) {
                const int s = b + lane;
                const bool in = s < cnt;
                const uint32_t d = slot[in ? s : 0];
                const double sc = acc[in ? s : 0];
                bool keep = in && sc >= min_score && !(dbg & 16);
                if constexpr (WITHIN) {                      // one 32-bit load per candidate from a row that stays in the L2
                    if (keep) keep = msr_in_set(srow, lo_span + d);
                }
                const unsigned long long km = __ballot(keep);
                if (keep) {
                    const int64_t w = seg_base + seg_cnt + lane_rank(km);
                    cand_score[w] = sc;
                    cand_doc[w] = (int32_t)(lo_span + d);
                }
                seg_cnt += __popcll(km);
            }
            lds_phase();
        }
        w0 = w1;
        base += cnt;
    }
    if (lane == 0) *seg_len = seg_cnt;
}

// Bind-time validation of the CSR the scoring kernel trusts: offsets monotone and complete, document indices
// in range and strictly ascending inside every posting list (that is what makes the LDS accumulation
// conflict-free and in-bounds), positive term frequencies, non-negative lengths.  flag starts at 0x7F7F7F7F and
// receives the lowest number among the violated rules.
__global__ __launch_bounds__(256) void validate_postings_kernel(Bm25Index ix, int32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t t = g; t <= ix.n_terms; t += stride) {
        const int64_t o = ix.term_off[t];
        if ((t == 0 && o != 0) || (t == ix.n_terms && o != ix.n_postings) || (t < ix.n_terms && ix.term_off[t + 1] < o))
            atomicMin(flag, 1);
    }
    for (int64_t d = g; d < ix.n_docs; d += stride)
        if (ix.doc_len[d] < 0) atomicMin(flag, 4);
    for (int64_t i = g; i < ix.n_postings; i += stride) {
        const int32_t d = ix.post_doc[i];
        if (d < 0 || d >= ix.n_docs) { atomicMin(flag, 2); continue; }
        if (ix.post_tf[i] <= 0) atomicMin(flag, 5);
        if (i > 0 && d <= ix.post_doc[i - 1]) {
            // a descent is only legal at the first posting of a term: i must be one of the offsets
            int64_t lo = 0, hi = ix.n_terms;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (ix.term_off[mid] < i) lo = mid + 1; else hi = mid;
            }
            if (ix.term_off[lo] != i) atomicMin(flag, 3);
        }
    }
}

// One workgroup per heavy term: tile_off[h][j] = number of postings of the term with document < j * TILE.
__global__ __launch_bounds__(256) void build_skip_kernel(Bm25Index ix, const int32_t* __restrict__ heavy_terms,
                                                          uint32_t* __restrict__ tile_off) {
    const int h = blockIdx.x;
    const int32_t t = heavy_terms[h];
    const int64_t s = ix.term_off[t], e = ix.term_off[t + 1];
    for (int j = threadIdx.x; j <= ix.n_tiles; j += 256) {
        const int64_t target = (int64_t)j * BM25_TILE;
        int64_t lo = s, hi = e;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ix.post_doc[mid] < target) lo = mid + 1; else hi = mid;
        }
        tile_off[(int64_t)h * (ix.n_tiles + 1) + j] = (uint32_t)(lo - s);
    }
}

// post[i] = {post_doc[i], tf_component}: what the scoring kernel streams, one 12-byte load per posting; post[n] = {-1, 0.0}.
// tf_component = (tf * (k1 + 1)) / (tf + k1 * (1 - b + b * doc_length / avg_doc_length))  (:473-475), evaluated here ONCE
// per posting, operation by operation as Python evaluates it (tf is a Python int: it is converted, not truncated)
__global__ __launch_bounds__(256) void bm25_post_comp_kernel(const int32_t* __restrict__ post_doc,
                                                              const int32_t* __restrict__ post_tf,
                                                              const double* __restrict__ dnorm, double k1p1, int64_t n,
                                                              Bm25Post* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (blockIdx.x == 0 && threadIdx.x == 0) {                   // the sentinel behind the last posting: "no posting here"
        Bm25Post z;
        z.doc = -1; z.comp_lo = 0u; z.comp_hi = 0u;
        out[n] = z;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int32_t d = post_doc[i], f = post_tf[i];
        const double tf = (double)f;
        const double comp = (tf * k1p1) / (tf + dnorm[d]);
        Bm25Post p;
        p.doc = d;
        p.comp_lo = (uint32_t)__double2loint(comp);
        p.comp_hi = (uint32_t)__double2hiint(comp);
        out[i] = p;
    }
}

// row h of the dense tables <- the tf_components of term dense_terms[h], by document (the rows are zero on entry: 0.0 marks
// a document without the term; a tf_component itself is never 0: tf >= 1, finite positive denominator)
__global__ __launch_bounds__(256) void bm25_dense_kernel(Bm25Index ix, const int32_t* __restrict__ dense_terms,
                                                          double* __restrict__ dense_comp, int64_t dense_stride) {
    const int h = blockIdx.y;
    const int32_t t = dense_terms[h];
    const int64_t s = ix.term_off[t], e = ix.term_off[t + 1];
    double* row = dense_comp + (int64_t)h * dense_stride;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = s + (int64_t)blockIdx.x * 256 + threadIdx.x; i < e; i += stride) {
        const Bm25Post p = ix.post[i];
        row[p.doc] = post_comp(p);
    }
}

// dnorm[d] = k1 * (1 - b + b * doc_length / avg_doc_length) for every document, padded to whole tiles (1.0 beyond n_docs):
// the scoring kernel's length norm, evaluated ONCE with the expression the reference evaluates per posting (:474)
__global__ __launch_bounds__(256) void bm25_dnorm_kernel(const int32_t* __restrict__ doc_len, int64_t n_docs, int64_t n_pad,
                                                          double k1, double b, double avgdl, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    const double omb = 1.0 - b;
    out[i] = i < n_docs ? k1 * (omb + (b * (double)doc_len[i]) / avgdl) : 1.0;
}

int g_bm25_dbg = 0;

}  // namespace

void msr_bm25_set_dbg(int v) { g_bm25_dbg = v; }      // honoured by -DMSR_DIAG builds only
hipError_t msr_bm25_build_skip(const Bm25Index& ix, const int32_t* heavy_terms, int n_heavy, uint32_t* tile_off,
                               hipStream_t stream) {
    if (n_heavy <= 0) return hipSuccess;
    build_skip_kernel<<<n_heavy, 256, 0, stream>>>(ix, heavy_terms, tile_off);
    return hipGetLastError();
}

hipError_t msr_bm25_post_comp(const int32_t* post_doc, const int32_t* post_tf, const double* dnorm, double k1, int64_t n,
                              Bm25Post* out, hipStream_t stream) {
    if (n < 0) return hipSuccess;
    bm25_post_comp_kernel<<<4096, 256, 0, stream>>>(post_doc, post_tf, dnorm, k1 + 1.0, n, out);   // self.k1 + 1
    return hipGetLastError();
}

hipError_t msr_bm25_build_dense(const Bm25Index& ix, const int32_t* dense_terms, int n_dense, double* dense_comp,
                                int64_t dense_stride, hipStream_t stream) {
    if (n_dense <= 0) return hipSuccess;
    bm25_dense_kernel<<<dim3(256, (unsigned)n_dense), 256, 0, stream>>>(ix, dense_terms, dense_comp, dense_stride);
    return hipGetLastError();
}

hipError_t msr_bm25_dnorm(const int32_t* doc_len, int64_t n_docs, int64_t n_pad, double k1, double b, double avgdl, double* out,
                          hipStream_t stream) {
    if (n_pad <= 0) return hipSuccess;
    bm25_dnorm_kernel<<<(unsigned)((n_pad + 255) / 256), 256, 0, stream>>>(doc_len, n_docs, n_pad, k1, b, avgdl, out);
    return hipGetLastError();
}

hipError_t msr_bm25_validate(const Bm25Index& ix, int32_t* flag, hipStream_t stream) {
    hipError_t err = hipMemsetAsync(flag, 0x7F, sizeof(int32_t), stream);
    if (err != hipSuccess) return err;
    validate_postings_kernel<<<2048, 256, 0, stream>>>(ix, flag);
    return hipGetLastError();
}

int msr_bm25_max_segments(int64_t n_docs) { return (int)((n_docs + BM25_TILE - 1) / BM25_TILE); }

// An upper bound of every score of a query, as the 20-bit key prefix (sign, exponent, 8 mantissa bits of the order-preserving
// key) the select's window pass anchors its 4096 bins to: U = (k1 + 1) * sum over the query's terms with positive idf of
// idf * qtf (a tf_component is below k1 + 1), a little raised; out[q] = prefix(U) - 4094, i.e. U falls into bin 4094 and bin
// 4095 stays empty unless the bound is wrong -- which the select notices (it then takes its general path).
//
// The same walk over a query's terms gives the scoring kernel its ITEM ORDER: weight[q] = the postings of the lists the scoring
// kernel will stream for q (bm25_classify, the kernel's own rule); order[0 .. nq) = the slice's queries by descending weight,
// ties by query number (rank by counting in LDS); order[nq] = n_heavy, the queries whose items are expected to stream more
// than the BM25_RES resident chunks: weight * (documents of a span) / n_docs > BM25_RES * 64.  They are a prefix of order[].
// Equal weights (and nq = 1) leave order[] the identity and n_heavy 0 or nq: the item order (span, query) without a plan.
// Workgroup b ranks the queries [64 b, 64 b + 64): every workgroup weighs ALL queries of the slice into its own LDS (the
// same loads in every workgroup, side by side on different CUs: one chain of round trips, whatever nq), then 16 threads
// per query count over a sixteenth of the weights each.  One workgroup for all of it took 25 us at 256 queries
// (profiles/stage1_query_skew.md), and its counting is nq^2 LDS reads on one CU.
constexpr int PLAN_THREADS = 1024;
constexpr int PLAN_QUERIES = 64;                   // queries a workgroup ranks
constexpr int PLAN_SLICES = PLAN_THREADS / PLAN_QUERIES;
constexpr int PLAN_MAX = 4096;                     // queries of a slice, at most (msr_create: max_queries <= 4096)
__global__ __launch_bounds__(PLAN_THREADS) void bm25_plan_kernel(Bm25Index ix, const int32_t* __restrict__ q_term_off,
                                                                  const int32_t* __restrict__ q_terms,
                                                                  const int32_t* __restrict__ q_qtf, int q_first, int nq,
                                                                  double min_score, int tpw, uint64_t* __restrict__ win_out,
                                                                  int32_t* __restrict__ order) {
    __shared__ unsigned long long weight[PLAN_MAX];
    __shared__ int rank_sh[PLAN_QUERIES];
    __shared__ int n_heavy;
    const int t = threadIdx.x;
    const int q_lo = (int)blockIdx.x * PLAN_QUERIES;             // this workgroup ranks [q_lo, q_lo + PLAN_QUERIES)
    const bool prune = bm25_prune(ix, min_score);
    if (t == 0) n_heavy = 0;
    if (t < PLAN_QUERIES) rank_sh[t] = 0;
    for (int q = t; q < nq; q += PLAN_THREADS) {
        const int t0 = q_term_off[q_first + q];
        int nt = q_term_off[q_first + q + 1] - t0;
        if (nt > BM25_MAX_TERMS) nt = BM25_MAX_TERMS;
        double u = 0.0;
        unsigned long long wt = 0;
        constexpr int TB = 8;                                    // terms side by side: their loads are independent
        for (int j0 = 0; j0 < nt; j0 += TB) {
            int32_t tq[TB], tf[TB];
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                tq[j] = j0 + j < nt ? q_terms[t0 + j0 + j] : -1;
                tf[j] = j0 + j < nt ? q_qtf[t0 + j0 + j] : 0;
            }
            Bm25Term tm[TB];
#pragma unroll
            for (int j = 0; j < TB; ++j) tm[j] = bm25_classify(ix, tq[j], tf[j], prune);
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                if (tq[j] < 0 || tq[j] >= ix.n_terms) continue;
                const double w = (double)ix.idf[tq[j]] * (double)tf[j];
                if (w > 0.0) u += w;
                if (tm[j].klass >= K_HEAVY) wt += (unsigned long long)(tm[j].e - tm[j].s);
            }
        }
        if (q >= q_lo && q < q_lo + PLAN_QUERIES) {
            u = u * (ix.k1 + 1.0) * 1.0000001 + 1e-300;
            const uint64_t pre = msr_ord64(u) >> 44;
            win_out[q] = pre > 4094 ? pre - 4094 : 0;
        }
        weight[q] = wt;
    }
    __syncthreads();
    {
        const int q = q_lo + (t & (PLAN_QUERIES - 1)), slice = t / PLAN_QUERIES;       // (the lanes of a wave share `slice`)
        const int per = (nq + PLAN_SLICES - 1) / PLAN_SLICES;
        const int o_hi = (slice + 1) * per < nq ? (slice + 1) * per : nq;
        if (q < nq) {
            const unsigned long long w = weight[q];
            int above = 0;
            for (int o = slice * per; o < o_hi; ++o) {
                const unsigned long long x = weight[o];
                above += x > w || (x == w && o < q);
            }
            if (above) atomicAdd(&rank_sh[q - q_lo], above);     // (LDS)
        }
    }
    __syncthreads();
    if (t < PLAN_QUERIES && q_lo + t < nq) order[rank_sh[t]] = q_lo + t;
    if (blockIdx.x != 0) return;
    // expected postings of an item = weight * span documents / n_docs; heavy: more than the resident chunks hold
    const unsigned long long span_docs = (unsigned long long)tpw * BM25_TILE;
    const unsigned long long heavy_above = (unsigned long long)(BM25_RES * 64) * (unsigned long long)ix.n_docs;
    int mine_heavy = 0;
    for (int q = t; q < nq; q += PLAN_THREADS) mine_heavy += weight[q] * span_docs > heavy_above;
    if (mine_heavy) atomicAdd(&n_heavy, mine_heavy);             // (LDS)
    __syncthreads();
    if (t == 0) order[nq] = n_heavy;
}

// A wave looks its query's terms up once and then walks `tpw` consecutive tiles with that plan in registers.  More tiles
// per wave amortise the lookups (chains of dependent loads) but leave fewer work items: large batches take 8, a single
// query one tile per wave (its ~1000 waves are all the parallelism it has).
void msr_bm25_split(int n_tiles, int nq, int* tpw_out, int* n_spans_out) {
    int tpw = BM25_TPW;
    while (tpw > 1 && (int64_t)nq * ((n_tiles + tpw - 1) / tpw) < 8192) tpw >>= 1;
    *tpw_out = tpw;
    *n_spans_out = (n_tiles + tpw - 1) / tpw;
}

hipError_t msr_bm25_scores(const Bm25Index& ix, const int32_t* q_term_off, const int32_t* q_terms,
                           const int32_t* q_qtf, int q_first, int nq, double min_score, double* cand_score,
                           int32_t* cand_doc, int32_t* seg_n, int* n_seg, int64_t* seg_stride, uint64_t* win, int32_t* order,
                           hipStream_t stream, const MsrSetView* set) {
    *n_seg = 0; *seg_stride = 0;
    if (nq <= 0 || ix.n_docs <= 0) return hipSuccess;
    if (nq > PLAN_MAX || !win || !order) return hipErrorInvalidValue;
    int tpw = 1, n_spans = 0;
    msr_bm25_split(ix.n_tiles, nq, &tpw, &n_spans);
    const int64_t items = (int64_t)nq * n_spans;
    if (items >= (1ll << 31)) return hipErrorInvalidValue;
    *n_seg = n_spans;
    *seg_stride = (int64_t)tpw * BM25_TILE;
    bm25_plan_kernel<<<(unsigned)((nq + PLAN_QUERIES - 1) / PLAN_QUERIES), PLAN_THREADS, 0, stream>>>(ix, q_term_off, q_terms, q_qtf, q_first, nq, min_score, tpw, win, order);
    const unsigned blocks = (unsigned)((items + BM25_WAVES - 1) / BM25_WAVES);
    if (set)
        bm25_taat_kernel<<<blocks, BM25_THREADS, 0, stream>>>(ix, q_term_off, q_terms, q_qtf, q_first, nq, min_score, tpw, n_spans,
                                                              cand_score, cand_doc, seg_n, order, g_bm25_dbg, *set);
    else
        bm25_taat_kernel<<<blocks, BM25_THREADS, 0, stream>>>(ix, q_term_off, q_terms, q_qtf, q_first, nq, min_score, tpw, n_spans,
                                                              cand_score, cand_doc, seg_n, order, g_bm25_dbg);
    return hipGetLastError();
}

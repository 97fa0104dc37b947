// K10 -- hybrid candidates (gfx950): BM25 scores of NAMED documents (a point lookup, not a stream) and the join of a lexical
// and a dense candidate list on the device.
//
// msr_bm25_score_docs.  The dense stage names a few hundred documents per query that the BM25 stage did not return; the
// rerank chain min-max normalises the "old similarity" over the whole candidate list (reranker_api.py:356-362), so each of
// them needs its TRUE BM25 score: the float64 sum the reference forms for that document (bm25_indexer.py:466-478), the
// contributions (idf * tf_component) * qtf of the query's unique valid terms the document contains, added in the query's
// first-occurrence order from 0.0.  K1 (msr_bm25.hip) gets those sums by streaming posting lists; for a handful of documents
// that is the wrong shape -- the city term alone has a list of 85 % of the corpus.  Here a wave owns PT_SLOTS (query,
// document) slots of one query; lane j = the query's j-th unique term (<= 64, as in K1's plan).  A lane reads its term's
// plan once (offsets, idf, qtf, table rows) and then finds, for every slot, its term's tf_component for the slot's document:
//   * the term has a dense tf_component table (long negative-idf list): ONE load, 0.0 = the document lacks the term;
//   * the term has a skip-table row (list of >= MSR_BM25_HEAVY_DF postings): two loads give the slice of the document's
//     1024-document tile, then a binary search of that slice (<= 10 probes);
//   * any other list (< 2048 postings): a binary search of the whole list (<= 11 probes);
// and one more 12-byte load of the posting found.  The searches of a batch of PT_U slots run side by side (independent
// loads in flight: the kernel is a chain of dependent loads, nothing else).  The values are the ones K1 streams -- the
// {doc, tf_component} copy of the postings and the tables built from it at bind -- so a contribution is K1's, bit for bit.
// The sum then runs over the lanes that found a posting in lane order 0, 1, 2 .. (a readlane loop: every lane forms the same
// sum; a tree or DPP reduction would change the order of the additions).  This file is compiled with -ffp-contract=off.
// No atomics, no LDS, no state: everything read was built by msr_bind_postings, so a re-bind is followed automatically.
//
// msr_union_candidates.  One workgroup per query: the lexical list unchanged, then the dense list's documents that are not
// in it (and not earlier in the dense list), in dense rank order, with the scores of the point kernel.  Both lists hold <=
// 1024 documents and sit in LDS; membership is a linear walk (every thread reads the same LDS word: a broadcast), <= 1024
// steps per thread and list -- at the serving shape (900 + 100) a few microseconds, which a sort or a hash would not beat.
#include "msr_common.h"
#include "msr_internal.h"

namespace {

constexpr int PT_SLOTS = 8;            // slots per wave (the plan -- ~8 dependent loads per lane -- is read once for them)
constexpr int PT_U = 4;                // slots whose searches run side by side
constexpr int PT_MAX_TERMS = 64;       // MSR_MAX_QUERY_TERMS: one lane per term

__device__ __forceinline__ double pt_comp(const Bm25Post& x) { return __hiloint2double((int)x.comp_hi, (int)x.comp_lo); }
__device__ __forceinline__ double pt_lane_f64(double v, int j) {          // v of lane j (j wave-uniform)
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)b, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)b >> 32), j);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

enum : int { P_DEAD = 0, P_TABLE = 1, P_HEAVY = 2, P_RANGE = 3 };

__global__ __launch_bounds__(64) void bm25_point_kernel(Bm25Index ix, const int32_t* __restrict__ q_term_off,
                                                        const int32_t* __restrict__ q_terms,
                                                        const int32_t* __restrict__ q_qtf, int nq,
                                                        const int32_t* __restrict__ doc, const int32_t* __restrict__ doc_n,
                                                        int max_docs, int groups, double* __restrict__ out_score,
                                                        int32_t* __restrict__ out_touched) {
    const int lane = threadIdx.x;
    const int q = (int)blockIdx.x / groups, g = (int)blockIdx.x - q * groups;     // (wave-uniform)
    if (q >= nq) return;
    int n_valid = doc_n ? doc_n[q] : max_docs;
    n_valid = n_valid < 0 ? 0 : (n_valid > max_docs ? max_docs : n_valid);
    const int slot0 = g * PT_SLOTS;
    const int64_t row = (int64_t)q * max_docs;
    // ---- the plan: lane j = term j of the query ----
    int klass = P_DEAD;
    int64_t s = 0, e = 0;                      // the term's posting list
    const double* table = nullptr;             // P_TABLE: its row of dense tf_components
    const uint32_t* skip = nullptr;            // P_HEAVY: its row of the skip table
    double idf = 0.0, qtf = 0.0;
    if (slot0 < n_valid) {                     // (a group of padding slots reads no plan)
        const int t0 = q_term_off[q];
        int nt = q_term_off[q + 1] - t0;
        if (nt > PT_MAX_TERMS) nt = PT_MAX_TERMS;                                 // the host never sends more
        if (lane < nt) {
            const int32_t t = q_terms[t0 + lane];
            if (t >= 0 && t < ix.n_terms) {
                s = ix.term_off[t];
                e = ix.term_off[t + 1];
                if (e > s) {                                                      // (:430: a term without postings is skipped)
                    idf = (double)ix.idf[t];
                    qtf = (double)q_qtf[t0 + lane];
                    const int dh = ix.dense_id ? ix.dense_id[t] : -1;
                    const int h = ix.heavy_id ? ix.heavy_id[t] : -1;
                    if (dh >= 0) {
                        klass = P_TABLE;
                        table = ix.dense_comp + (int64_t)dh * ix.dense_stride;
                    } else if (h >= 0) {
                        klass = P_HEAVY;
                        skip = ix.tile_off + (int64_t)h * (ix.n_tiles + 1);
                    } else {
                        klass = P_RANGE;
                    }
                }
            }
        }
    }
    const int64_t null_post = ix.n_postings;                                      // the sentinel {doc -1, 0.0}
#pragma unroll 1
    for (int b0 = 0; b0 < PT_SLOTS; b0 += PT_U) {
        int32_t d[PT_U];
        bool live[PT_U];                       // the slot names a document of the index (wave-uniform)
        int64_t lo[PT_U], hi[PT_U], end[PT_U];
        double comp[PT_U];
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            const int slot = slot0 + b0 + u;
            d[u] = slot < n_valid ? doc[row + slot] : -1;
            live[u] = d[u] >= 0 && (int64_t)d[u] < ix.n_docs;
            lo[u] = hi[u] = end[u] = 0;
            comp[u] = 0.0;
        }
        // the slice to search (P_HEAVY: from the skip table) and the table loads
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            if (!live[u]) continue;                                               // (wave-uniform)
            if (klass == P_TABLE) {
                comp[u] = table[d[u]];
            } else if (klass == P_HEAVY) {
                const int tile = d[u] / MSR_BM25_TILE;
                lo[u] = s + skip[tile];
                hi[u] = end[u] = s + skip[tile + 1];
            } else if (klass == P_RANGE) {
                lo[u] = s;
                hi[u] = end[u] = e;
            }
        }
        // lower bound of d in [lo, hi): the probes of the PT_U slots are independent loads
        for (;;) {
            bool more = false;
#pragma unroll
            for (int u = 0; u < PT_U; ++u) more |= lo[u] < hi[u];
            if (!__any(more)) break;
            int32_t pd[PT_U];
            int64_t mid[PT_U];
#pragma unroll
            for (int u = 0; u < PT_U; ++u) {
                mid[u] = (lo[u] + hi[u]) >> 1;
                pd[u] = ix.post[lo[u] < hi[u] ? mid[u] : null_post].doc;
            }
#pragma unroll
            for (int u = 0; u < PT_U; ++u) {
                if (lo[u] < hi[u]) {
                    if (pd[u] < d[u]) lo[u] = mid[u] + 1; else hi[u] = mid[u];
                }
            }
        }
        // the posting found (or the sentinel)
        {
            Bm25Post p[PT_U];
#pragma unroll
            for (int u = 0; u < PT_U; ++u) p[u] = ix.post[lo[u] < end[u] ? lo[u] : null_post];
#pragma unroll
            for (int u = 0; u < PT_U; ++u)
                if (klass >= P_HEAVY && p[u].doc == d[u]) comp[u] = pt_comp(p[u]);     // (d >= 0 here: the sentinel never matches)
        }
        // the sum, in the query's term order (bm25_indexer.py:466-478)
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            const int slot = slot0 + b0 + u;
            if (slot >= max_docs) continue;                                       // (wave-uniform)
            const bool has = live[u] && comp[u] != 0.0;                           // (a tf_component is never 0: tf >= 1)
            const double c = (idf * comp[u]) * qtf;                               // term_score = idf * tf_component * qtf (:478)
            unsigned long long m = __ballot(has);
            const int touched = m != 0ull;
            double acc = 0.0;                                                     // bm25_score = 0.0 (:466)
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                acc = acc + pt_lane_f64(c, j);                                    // bm25_score += term_score
            }
            if (lane == 0) {
                out_score[row + slot] = acc;
                out_touched[row + slot] = touched;
            }
        }
    }
}

constexpr int UN_THREADS = 256;
constexpr int UN_MAX = 1024;           // documents per input list (MSR_MAX_K)

__global__ __launch_bounds__(UN_THREADS) void union_kernel(const int32_t* __restrict__ lex_doc, const double* __restrict__ lex_score,
                                                           const int32_t* __restrict__ lex_n, int k_lex,
                                                           const int32_t* __restrict__ dense_doc,
                                                           const double* __restrict__ dense_bm25,
                                                           const int32_t* __restrict__ dense_n, int k_dense,
                                                           int32_t* __restrict__ out_doc, double* __restrict__ out_score,
                                                           int32_t* __restrict__ out_src, int32_t* __restrict__ out_n,
                                                           int max_cand) {
    __shared__ int32_t L[UN_MAX], D[UN_MAX];
    __shared__ int32_t wave_cnt[UN_THREADS / 64];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nl = k_lex > 0 ? lex_n[q] : 0, nd = k_dense > 0 ? dense_n[q] : 0;
    nl = nl < 0 ? 0 : (nl > k_lex ? k_lex : nl);
    nd = nd < 0 ? 0 : (nd > k_dense ? k_dense : nd);
    const int64_t lrow = (int64_t)q * k_lex, drow = (int64_t)q * k_dense, orow = (int64_t)q * max_cand;
    for (int i = tid; i < nl; i += UN_THREADS) L[i] = lex_doc[lrow + i];
    for (int j = tid; j < nd; j += UN_THREADS) D[j] = dense_doc[drow + j];
    __syncthreads();
    // the lexical list as it is; source 3 if the dense list names the document too
    for (int i = tid; i < nl; i += UN_THREADS) {
        const int32_t x = L[i];
        bool both = false;
        if (x >= 0)
            for (int j = 0; j < nd; ++j) both |= D[j] == x;
        out_doc[orow + i] = x;
        out_score[orow + i] = lex_score[lrow + i];
        out_src[orow + i] = both ? 3 : 1;
    }
    // the dense list's new documents behind it, in dense rank order
    int n_out = nl;                                                               // (workgroup-uniform)
    for (int base = 0; base < nd; base += UN_THREADS) {
        const int j = base + tid;
        bool keep = false;
        int32_t x = -1;
        if (j < nd) {
            x = D[j];
            keep = x >= 0;
            if (keep) {
                bool seen = false;
                for (int i = 0; i < nl; ++i) seen |= L[i] == x;
                for (int i = 0; i < j; ++i) seen |= D[i] == x;                     // a repeat: the first place counts
                keep = !seen;
            }
        }
        const unsigned long long km = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(km);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < UN_THREADS / 64; ++w) {
            if (w < wave) before += wave_cnt[w];
            total += wave_cnt[w];
        }
        if (keep) {
            const int m = n_out + before +
                          (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
            out_doc[orow + m] = x;                                               // m < nl + nd <= k_lex + k_dense <= max_cand
            out_score[orow + m] = dense_bm25[drow + j];
            out_src[orow + m] = 2;
        }
        n_out += total;
        __syncthreads();
    }
    for (int m = n_out + tid; m < max_cand; m += UN_THREADS) {                     // the padding of every list of the chain
        out_doc[orow + m] = -1;
        out_score[orow + m] = -__builtin_inf();
        out_src[orow + m] = 0;
    }
    if (tid == 0) out_n[q] = n_out;
}

}  // namespace

hipError_t msr_bm25_point(const Bm25Index& ix, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf, int nq,
                          const int32_t* doc, const int32_t* doc_n, int max_docs, double* out_score, int32_t* out_touched,
                          hipStream_t stream) {
    if (nq <= 0 || max_docs <= 0) return hipSuccess;
    const int groups = (max_docs + PT_SLOTS - 1) / PT_SLOTS;
    if ((int64_t)nq * groups >= (1ll << 31)) return hipErrorInvalidValue;
    bm25_point_kernel<<<(unsigned)((int64_t)nq * groups), 64, 0, stream>>>(ix, q_term_off, q_terms, q_qtf, nq, doc, doc_n, max_docs,
                                                                          groups, out_score, out_touched);
    return hipGetLastError();
}

hipError_t msr_union_lists(int nq, const int32_t* lex_doc, const double* lex_score, const int32_t* lex_n, int k_lex,
                           const int32_t* dense_doc, const double* dense_bm25, const int32_t* dense_n, int k_dense,
                           int32_t* out_doc, double* out_score, int32_t* out_src, int32_t* out_n, int max_cand,
                           hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (k_lex < 0 || k_lex > UN_MAX || k_dense < 0 || k_dense > UN_MAX || (int64_t)k_lex + k_dense > max_cand)
        return hipErrorInvalidValue;
    union_kernel<<<(unsigned)nq, UN_THREADS, 0, stream>>>(lex_doc, lex_score, lex_n, k_lex, dense_doc, dense_bm25, dense_n, k_dense,
                                                         out_doc, out_score, out_src, out_n, max_cand);
    return hipGetLastError();
}

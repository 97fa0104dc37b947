// K6 -- rerank / fuse of the stage-1 candidates (gfx950).  Compiled with -ffp-contract=off.
//
// Replaces the arithmetic of the /rerank endpoint (reranker/reranker_api.py):
//   candidate fetch   URL dedup (MIN(id) per URL-without-query-string), first <=10 chunks   :27-63
//   cosine            sklearn cosine_similarity, float32                                     :273-287
//   min-max           over ALL chunk rows of the request, python floats (float64)            :289-296, 360-361
//   blend             new*(1-smoothing) + old*smoothing                                      :362
//   positional        boost/decay of each document's best chunk                              :299-334
//   pool + order      per-document first maximum, descending                                 :370-372
// Two kernels: (A) one wave per (query, candidate) gathers the candidate's chunk rows and computes the
// cosines (HBM-bound gather of <= 10 x 3 KiB rows) plus three integers per candidate (rows, URL group,
// first row); (B) one workgroup per query runs the float64 chain on <= 1024 candidates entirely in LDS,
// reading ONLY the arrays (A) produced.  That split is what lets a doc-sharded index rerank a global
// candidate list: each shard runs (A) for the documents it owns, the halves of a query travel to the rank that fuses that
// query (one all-to-all, msretr/distributed.py) and are joined there (or_parts_kernel: all other shards contributed
// zeros), and that rank runs (B) for its share of the queries.
#include "msr_common.h"
#include "msr_internal.h"
#include "msr_sort.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int RR_MAXC = 10;           // scratch slots per candidate (MSR_RERANK_MAX_CHUNKS)
constexpr int RR_THREADS = 1024;
constexpr int RR_MAXM = 1024;

// One wave per query and block of 8 candidate slots: lanes 0 .. 7 sort the slots into "mine" (the document lies in this
// shard) and "not mine" (zeros: the owner's words arrive through the join of the shards' halves), then the wave takes the
// rows of all the slots that are mine as ONE list (<= 80 rows) and runs one row pipeline over it, RC_DEPTH rows in flight.
// (Before, the slots were taken one after the other with, by the source, two rows in flight; the compiled loop had at most
// one: lane 0's out[..] = s * inv_norm[c] is a load, an s_waitcnt vmcnt(0) and a store behind the next row's loads, and
// vmcnt retires in order, so the wait for the norm drained the row just asked for; the document offsets were one more
// round trip per slot.  Now offsets and norms are loaded once per block, nothing in the row loop depends on a load but
// the rows themselves, and a slot's cosines are stored by one instruction behind its last row.)
// (One wave per slot, as before, launches N times the waves a rank of an N-way
// sharded run has work for -- 2 M waves per 2048-query step at N = 8, most of which only wrote zeros: 2.2 ms instead of 0.7;
// workgroups of several waves sharing a block lose 12 % on the unsharded corpus, where every slot is work: a workgroup
// keeps its place on the CU until its slowest wave is done.)
// SLOTS = 1 (calls of a few queries, no records): one wave per candidate slot -- a single query has 1000 slots, i.e. 125 waves
// of 8 slots each on a chip with room for thousands; its gather took 43 us of one after the other.
constexpr int RC_SLOTS = 8;
#ifndef MSR_RC_DEPTH
#define MSR_RC_DEPTH 4
#endif
// rows in flight per wave: 2 / 3 / 4 = 56 / 68 / 79 VGPRs = 8 / 7 / 6 waves per SIMD; 4 measured fastest and steadiest
// (profiles/rerank_stage_pipeline.md)
constexpr int RC_DEPTH = MSR_RC_DEPTH;
static_assert(RC_DEPTH >= 2 && RC_DEPTH <= 4, "the tail's waits are written out for 2 .. 4 rows");

typedef const __attribute__((address_space(1))) char* rr_gptr;    // (global, not flat)
// loads the compiler neither moves nor counts: the caller waits (rr_wait) and pins the destination before its first use
template <int OFF>
__device__ __forceinline__ void rr_load16(f32x4& r, rr_gptr p) {
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
}
__device__ __forceinline__ void rr_load4(float& r, rr_gptr p) {
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
}
template <int N>
__device__ __forceinline__ void rr_wait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

template <bool TILED, int SLOTS = RC_SLOTS>
__global__ __launch_bounds__(64) void rerank_cos_kernel(DenseIndex ix, const int32_t* __restrict__ url_group,
                                                         const float* __restrict__ qn,
                                                         const int32_t* __restrict__ cand_doc,
                                                         const int32_t* __restrict__ cand_n, int max_cand,
                                                         int doc_base, int row_base, int max_chunks,
                                                         float* __restrict__ cos_out, int32_t* __restrict__ meta,
                                                         int q_per_block, int64_t block_stride, RerankRecords rec) {
    // cand_doc holds GLOBAL document indices; this shard owns [doc_base, doc_base + n_docs).
    // Output layout: query q's rows start (q / q_per_block) * block_stride words + (q % q_per_block) rows into cos_out / meta
    // (one contiguous array: q_per_block >= the number of queries; the blocks of an all-to-all send buffer: see msretr.h).
    // RECORDS (rec.out != null): nothing is written for the slots this shard does not own; an owned slot becomes a 16-word
    // record [slot, rows, url group + 2, first row, cos x 10, query, 0] at the place rerank_plan_kernel counted out for it.
    const int q = blockIdx.y, m0 = blockIdx.x * SLOTS, lane = threadIdx.x;
    const bool records = rec.out != nullptr;
    cos_out += (int64_t)(q / q_per_block) * block_stride + (int64_t)(q % q_per_block) * max_cand * RR_MAXC;
    meta += (int64_t)(q / q_per_block) * block_stride + (int64_t)(q % q_per_block) * max_cand * 3;
    int d_mine = -1;
    {
        const int m = m0 + lane;
        const bool slot = lane < SLOTS && m < max_cand;
        if (slot && m < cand_n[q]) d_mine = cand_doc[(int64_t)q * max_cand + m] - doc_base;
        const bool own = d_mine >= 0 && d_mine < ix.n_docs;
        if (!own) d_mine = -1;
        if (slot && !own && !records) {                  // not a candidate, or owned by another shard
            float* out = cos_out + (int64_t)m * RR_MAXC;
            int32_t* mt = meta + (int64_t)m * 3;
#pragma unroll
            for (int i = 0; i < RR_MAXC; ++i) out[i] = 0.f;
            mt[0] = 0; mt[1] = 0; mt[2] = 0;
        }
    }
    const unsigned long long mine_all = __ballot(d_mine >= 0);
    if (mine_all == 0) return;
    const f32x4* q4 = (const f32x4*)(qn + (size_t)q * MSR_DIM);
    f32x4 qa = q4[lane], qb = q4[lane + 64], qc = q4[lane + 128];

    // ---- every slot of the block at once: lane sl < SLOTS owns slot m0 + sl ------------------------------------------------
    // One round trip for the 2 x SLOTS document offsets, meta written by the slots' lanes; rows = the slot's row count
    // clamped to max_chunks (0: not mine, no chunk, or a record past rec.capacity, which is dropped whole as before).
    int64_t rec_first = 0;
    if (records) rec_first = (int64_t)rec.q_base[q] + rec.blk_off[(int64_t)q * gridDim.x + blockIdx.x];
    auto record_of = [&](int sl) -> int64_t { return rec_first + __builtin_popcountll(mine_all & ((1ull << sl) - 1)); };
    auto cos_of = [&](int sl) -> float* {
        return records ? (float*)(rec.out + record_of(sl) * MSR_RERANK_RECORD_WORDS + 4) : cos_out + (int64_t)(m0 + sl) * RR_MAXC;
    };
    // Loads first, stores after.  The URL group is asked for beside the offsets, without a branch (in a branch of its own,
    // or behind a store, it is one more round trip).  The query was asked for before the offsets, so it has landed with them:
    // pinned between the loads and the stores, the compiler's wait for it costs nothing -- behind the stores it would be a
    // vmcnt(0) that waits for them, and behind the loads of inv_norm one that drains those.
    int ds = 0, rows = 0, group = 0;                         // (doc_off is 32-bit: row numbers fit an int)
    bool live = d_mine >= 0;
    int64_t at = 0;
    if (records && live) {
        at = record_of(lane);
        live = at >= 0 && at < rec.capacity;
    }
    if (live) {
        const int32_t* gp = url_group ? url_group + d_mine : ix.doc_off + d_mine;
        const int gword = *gp;
        ds = ix.doc_off[d_mine];
        rows = ix.doc_off[d_mine + 1] - ds;
        group = url_group ? gword : d_mine + doc_base;
        if (rows > max_chunks) rows = max_chunks;
    }
    asm volatile("" : "+v"(qa), "+v"(qb), "+v"(qc), "+v"(ds), "+v"(rows), "+v"(group));
    if (live) {
        int32_t* mt = meta + (int64_t)(m0 + lane) * 3;
        if (records) {
            int32_t* r = rec.out + at * MSR_RERANK_RECORD_WORDS;
            mt = r + 1;
            r[0] = m0 + lane; r[14] = rec.q_first + q; r[15] = 0;
        }
        mt[0] = rows;                                        // chunk rows that take part (<= max_chunks)
        // URL group + 2, so that after the join of the shards' halves 0 = nobody owns it, 1 = owned, not in urlsDB
        mt[1] = group + 2;
        mt[2] = ds + row_base;                               // global row of the document's first chunk
        if (rows <= 0) {                                     // no row: all ten places are zero (a slot with rows writes its ten
            float* out = cos_of(lane);                       // places, zeros included, behind its last row)
#pragma unroll
            for (int i = 0; i < RR_MAXC; ++i) out[i] = 0.f;
        }
    }
    if (rows < 0) rows = 0;
    // the block's flat row list: slot sl's rows are numbers [incl(sl) - rows(sl), incl(sl)), R <= 10 SLOTS rows in all
    int incl = rows;
#pragma unroll
    for (int o = 1; o < SLOTS; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const int R = __builtin_amdgcn_readlane(incl, SLOTS - 1);
    if (R == 0) return;
    // inv_norm of row number `lane` (and lane + 64) of the list goes into that lane.  The loads are inline asm like the rows':
    // a load the compiler counts would be waited for with vmcnt(0) at its first use, behind the first rows of the pipeline.
    // Lanes past the list load the list's last row's (an address that is a candidate's row, whatever the lane).
    auto list_row = [&](int r) -> int64_t {                  // (per lane) global row of list entry min(r, R - 1)
        r = r < R ? r : R - 1;
        int sl = 0;
#pragma unroll
        for (int j = 0; j + 1 < SLOTS; ++j) sl += r >= __builtin_amdgcn_readlane(incl, j) ? 1 : 0;
        return (int64_t)__shfl(ds, sl) + (r - (__shfl(incl, sl) - __shfl(rows, sl)));
    };
    float inv_a, inv_b = 0.f;
    rr_load4(inv_a, (rr_gptr)(ix.inv_norm + list_row(lane)));
    if (SLOTS > 6) rr_load4(inv_b, (rr_gptr)(ix.inv_norm + list_row(lane + 64)));

    // ---- one row pipeline over the list, across the slots' boundaries: RC_DEPTH rows in flight per wave ---------------------
    // Driven by hand as the row ring of msr_gemm_f32.hip: inline-asm loads the compiler neither counts nor moves, a counted
    // s_waitcnt before every use.  Vector-memory operations retire in order, so with `ahead` rows issued behind row r,
    // vmcnt(3 ahead) says row r has landed (and inv_norm, which is older than every row); a candidate's cosine store, issued
    // behind some of those rows, only makes the wait ask for a little more.  Row r + RC_DEPTH is asked for as soon as row r's
    // 12 products per lane are taken (they read the slot; the butterfly, the scaling and the store follow the new loads).
    // Only the list's last RC_DEPTH - 1 rows wait with fewer rows behind them, the last one with vmcnt(0).
    // The ring hazard of DESIGN K2+K3: the compiler takes an asm load's destination as written at once, so no copy of a slot
    // may live across its reload -- the products are forced out (the empty asm on dot) before the slot is loaded again.
    struct Walk { int sl, j, n; unsigned left; };            // (wave-uniform) a position in the list: slot, row within it, its rows
    auto start = [&](Walk& w) {
        w.left = (unsigned)__ballot(rows > 0);
        w.sl = __builtin_ctz(w.left); w.left &= w.left - 1; w.j = 0; w.n = __builtin_amdgcn_readlane(rows, w.sl);
    };
    auto advance = [&](Walk& w) {
        if (++w.j == w.n && w.left != 0) { w.sl = __builtin_ctz(w.left); w.left &= w.left - 1; w.j = 0; w.n = __builtin_amdgcn_readlane(rows, w.sl); }
    };
    Walk wi, wr;                                             // the next row to ask for; the next row to reduce
    start(wi);
    wr = wi;
    const rr_gptr emb = (rr_gptr)ix.emb;
    // float4 number v of a row of the interleaved image (dims 4v .. 4v + 3) lives at block v >> 2, place 16 (v & 3) + i of the
    // 16-row group: lane + 64 k is 16384 k bytes behind lane's
    const int64_t lane_off = TILED ? (int64_t)((lane >> 2) * 64 + (lane & 3) * 16) * 16 : (int64_t)lane * 16;
    auto issue = [&](f32x4 (&s)[3]) {
        const int64_t c = (int64_t)__builtin_amdgcn_readlane(ds, wi.sl) + wi.j;
        if (TILED) {
            const rr_gptr p = emb + (c >> 4) * (int64_t)(16 * MSR_DIM * 4) + (c & 15) * 16 + lane_off;
            rr_load16<0>(s[0], p); rr_load16<0>(s[1], p + 16384); rr_load16<0>(s[2], p + 32768);
        } else {
            const rr_gptr p = emb + c * (int64_t)(MSR_DIM * 4) + lane_off;
            rr_load16<0>(s[0], p); rr_load16<1024>(s[1], p); rr_load16<2048>(s[2], p);
        }
        advance(wi);
    };
    f32x4 ring[RC_DEPTH][3];
#pragma unroll
    for (int k = 0; k < RC_DEPTH; ++k)
        if (k < R) issue(ring[k]);
    float park = 0.f;                                        // lane j: the cosine of row j of the candidate being reduced
    for (int r0 = 0; r0 < R; r0 += RC_DEPTH) {
#pragma unroll
        for (int k = 0; k < RC_DEPTH; ++k) {
            const int r = r0 + k;
            if (r >= R) break;                               // (wave-uniform)
            const int ahead = R - 1 - r;
            if (ahead >= RC_DEPTH - 1) rr_wait<3 * (RC_DEPTH - 1)>();
            else if (ahead == 2) rr_wait<6>();
            else if (ahead == 1) rr_wait<3>();
            else rr_wait<0>();
            f32x4(&s)[3] = ring[k];
            asm volatile("" : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(inv_a), "+v"(inv_b));
            float dot = s[0].x * qa.x + s[0].y * qa.y + s[0].z * qa.z + s[0].w * qa.w;
            dot += s[1].x * qb.x + s[1].y * qb.y + s[1].z * qb.z + s[1].w * qb.w;
            dot += s[2].x * qc.x + s[2].y * qc.y + s[2].z * qc.z + s[2].w * qc.w;
            asm volatile("" : "+v"(dot));
            if (r + RC_DEPTH < R) issue(s);
            for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
            const float inv = __int_as_float((SLOTS > 6 && r >= 64) ? __builtin_amdgcn_readlane(__float_as_int(inv_b), r - 64)
                                                                     : __builtin_amdgcn_readlane(__float_as_int(inv_a), r));
            if (lane == wr.j) park = dot * inv;
            if (wr.j + 1 == wr.n) {                          // the candidate's last row: its ten places with one store
                float* out = cos_of(wr.sl);
                if (lane < RR_MAXC) out[lane] = park;
                park = 0.f;
            }
            advance(wr);
        }
    }
}

// (B) one workgroup per query, thread i = candidate slot i.  Everything a slot needs from memory -- document, (rows, group,
// first row), BM25 score and its ten cosines as five 8-byte loads (a slot's cosines start at a multiple of 40 bytes) -- is
// asked for once, before anything is used, and stays in registers for both the min-max and the chain; the chain's rows
// v[0 .. 9] are indexed by constants only (the row loops are unrolled and predicated), so nothing lives in scratch.
constexpr int RF_TABLE = 2048;        // URL-group table: twice the slots, linear probing
__global__ __launch_bounds__(RR_THREADS) void rerank_fuse_kernel(
    const int32_t* __restrict__ cand_doc, const double* __restrict__ cand_bm25,
    const int32_t* __restrict__ cand_n, int max_cand, RerankParams prm, const float* __restrict__ cos_in,
    const int32_t* __restrict__ meta, int32_t* __restrict__ out_doc, double* __restrict__ out_score,
    double* __restrict__ out_orig, int32_t* __restrict__ out_chunk, int32_t* __restrict__ out_n,
    int32_t* __restrict__ out_rows) {
    __shared__ uint64_t khi[RR_MAXM];
    __shared__ uint32_t klo[RR_MAXM];
    __shared__ uint32_t val[RR_MAXM];
    __shared__ double sc[RR_MAXM];
    __shared__ double og[RR_MAXM];
    __shared__ int32_t ch[RR_MAXM];
    __shared__ uint32_t tkey[RF_TABLE];                          // group word (>= 2), 0 = free
    __shared__ unsigned long long tmin[RF_TABLE];                // the group's smallest (document, slot)
    __shared__ double red_b[2][RR_THREADS / 64];
    __shared__ float red_c[2][RR_THREADS / 64];
    __shared__ int red_n[2][RR_THREADS / 64];

    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = cand_n[q];
    if (n > max_cand) n = max_cand;
    if (n > RR_MAXM) n = RR_MAXM;
    int P = 64;
    while (P < n) P <<= 1;

    // 0. the slot's words
    int d = -1, nr = 0, gw = 0, first = 0;
    double bm = 0.0;
    float c[RR_MAXC];
#pragma unroll
    for (int j = 0; j < RR_MAXC; ++j) c[j] = 0.f;
    if (tid < n) {
        const int64_t m = (int64_t)q * max_cand + tid;
        const float2* cs = (const float2*)(cos_in + m * RR_MAXC);
        float2 c2[RR_MAXC / 2];
#pragma unroll
        for (int j = 0; j < RR_MAXC / 2; ++j) c2[j] = cs[j];
        d = cand_doc[m];
        nr = meta[3 * m]; gw = meta[3 * m + 1]; first = meta[3 * m + 2];
        bm = cand_bm25[m];
#pragma unroll
        for (int j = 0; j < RR_MAXC / 2; ++j) { c[2 * j] = c2[j].x; c[2 * j + 1] = c2[j].y; }
    }
    for (int i = tid; i < RF_TABLE; i += RR_THREADS) { tkey[i] = 0; tmin[i] = ~0ull; }
    __syncthreads();

    // 1. keep = the smallest (document, slot) of its URL group (MIN(id) per URL, :38-47; among repeated slots of that
    //    document the first slot, msretr.h) that has at least one chunk row.  This is the rule the sort by (group, document,
    //    slot) implemented -- "first entry of its group" IS the group's minimum -- found with one 64-bit LDS minimum per slot
    //    in a table keyed by the group instead of a 55-stage network.  The final order does not depend on the order the kept
    //    slots are found in: kept documents are distinct (one per group, and a document has one group), so the keys
    //    (score, ~document) of the sort below are unique and val carries the slot.
    const bool valid = d >= 0 && gw >= 2;
    const unsigned long long mine = ((unsigned long long)(uint32_t)d << 32) | (uint32_t)tid;
    int h = 0;
    if (valid) {
        h = (int)(((uint32_t)gw * 2654435761u) >> 21);           // top 11 bits: RF_TABLE places
        for (;;) {
            const uint32_t old = atomicCAS(&tkey[h], 0u, (uint32_t)gw);
            if (old == 0u || old == (uint32_t)gw) break;
            h = (h + 1) & (RF_TABLE - 1);                        // (<= 1024 groups in 2048 places: a free place exists)
        }
        atomicMin(&tmin[h], mine);
    }
    __syncthreads();
    const bool keep = valid && nr > 0 && tmin[h] == mine;

    // 2. min-max over the kept slots' rows and BM25 scores, the counts: per wave by shuffles / ballot, then 16 partials
    //    per value in LDS -- two barriers for all of it.  (Minima and maxima of the f32 cosines are taken in f32: the
    //    conversion to double is exact and monotone.)
    float cmin_f = __builtin_inff(), cmax_f = -__builtin_inff();
    double bmin = __builtin_inf(), bmax = -__builtin_inf();
    if (keep) {
#pragma unroll
        for (int j = 0; j < RR_MAXC; ++j)
            if (j < nr) { cmin_f = c[j] < cmin_f ? c[j] : cmin_f; cmax_f = c[j] > cmax_f ? c[j] : cmax_f; }
        bmin = bm; bmax = bm;
    }
    int rows_w = keep ? nr : 0;
    for (int o = 32; o > 0; o >>= 1) {
        const float u0 = __shfl_xor(cmin_f, o), u1 = __shfl_xor(cmax_f, o);
        const double u2 = __shfl_xor(bmin, o), u3 = __shfl_xor(bmax, o);
        cmin_f = u0 < cmin_f ? u0 : cmin_f; cmax_f = u1 > cmax_f ? u1 : cmax_f;
        bmin = u2 < bmin ? u2 : bmin; bmax = u3 > bmax ? u3 : bmax;
        rows_w += __shfl_xor(rows_w, o);
    }
    const unsigned long long kept_w = __ballot(keep);
    if (lane == 0) {
        red_c[0][wave] = cmin_f; red_c[1][wave] = cmax_f; red_b[0][wave] = bmin; red_b[1][wave] = bmax;
        red_n[0][wave] = rows_w; red_n[1][wave] = __builtin_popcountll(kept_w);
    }
    __syncthreads();
    int n_rows = 0, n_keep = 0;
    for (int i = 0; i < RR_THREADS / 64; ++i) {
        const float u0 = red_c[0][i], u1 = red_c[1][i];
        const double u2 = red_b[0][i], u3 = red_b[1][i];
        cmin_f = u0 < cmin_f ? u0 : cmin_f; cmax_f = u1 > cmax_f ? u1 : cmax_f;
        bmin = u2 < bmin ? u2 : bmin; bmax = u3 > bmax ? u3 : bmax;
        n_rows += red_n[0][i]; n_keep += red_n[1][i];
    }
    const double cmin = (double)cmin_f, cmax = (double)cmax_f;

    // 3. per kept document: normalise, blend, positional weighting, first maximum
    const double one_m_s = 1.0 - prm.smoothing;
    if (tid < P) {                                               // P <= RR_THREADS: one entry per thread
        uint64_t shi = 0; uint32_t slo = 0;
        if (keep) {
            const double old = (bmax == bmin) ? 0.0 : (bm - bmin) / (bmax - bmin);
            double v[RR_MAXC];
            int best = 0;
            double vb = 0.0;                                     // v[best]
#pragma unroll
            for (int j = 0; j < RR_MAXC; ++j) {
                v[j] = 0.0;
                if (j < nr) {
                    const double nw = (cmax == cmin) ? 0.0 : ((double)c[j] - cmin) / (cmax - cmin);
                    v[j] = nw * one_m_s + old * prm.smoothing;
                    if (j == 0) vb = v[0];
                    else if (v[j] > vb) { best = j; vb = v[j]; }
                }
            }
            if (nr > 1) {
                const double ratio = (double)best / (double)(nr - 1);
                const double adj = prm.max_boost - (prm.max_boost + prm.max_decay) * ratio;
                double a = vb + adj;
                a = a < 1.0 ? a : 1.0;                           // min(1.0, adjusted)
                a = a > 0.0 ? a : 0.0;                           // max(0.0, ...)
                const int shifted = best;
                best = 0;
                vb = shifted == 0 ? a : v[0];
#pragma unroll
                for (int j = 1; j < RR_MAXC; ++j) {
                    const double vj = shifted == j ? a : v[j];
                    if (j < nr && vj > vb) { best = j; vb = vj; }
                }
            }
            sc[tid] = vb; og[tid] = old; ch[tid] = first + best;
            shi = msr_ord64(vb); slo = ~(uint32_t)d;
        }
        khi[tid] = shi; klo[tid] = slo; val[tid] = (uint32_t)tid;
    }
    __syncthreads();
    // 4. order by (score desc, doc asc)
    msr_sort::bitonic_sort<RR_THREADS, true>(khi, klo, val, P, false);
    for (int i = tid; i < max_cand; i += RR_THREADS) {
        const int64_t o = (int64_t)q * max_cand + i;
        if (i < n_keep) {
            const int src = (int)val[i];
            out_doc[o] = (int32_t)~klo[i]; out_score[o] = sc[src]; out_orig[o] = og[src]; out_chunk[o] = ch[src];
        } else {
            out_doc[o] = -1; out_score[o] = -__builtin_inf(); out_orig[o] = 0.0; out_chunk[o] = -1;
        }
    }
    if (tid == 0) { out_n[q] = n_keep; out_rows[q] = n_rows; }
}


// ---- domain diversification of the fused lists (reranker_api.py:178-236), one workgroup per query ----------------------
// Input: the fused list of a query as rerank_fuse_kernel leaves it -- (new_similarity desc, document asc) -- and one word
// per document: its DOMAIN id (urlparse(url).netloc.lower(), :170-176, numbered by the host at bind) or -1 for a document
// the reference's response models reject (NULL title / url / text, :376-397; dropped BEFORE the diversification).
// hybrid_diversification on a list in that order reduces to (derivation in DESIGN.md section 3, K6b):
//   * a domain is "high" iff its FIRST entry scores >= threshold (the list is sorted, the first entry is the domain's best);
//     every entry of a domain is in the same tier, so apply_domain_cap(.., 1) on either tier keeps exactly the first entry
//     of each domain: kept-high entries (score >= threshold) precede kept-medium ones in list order;
//   * final = kept-high + kept-medium[: top_k - #kept-high]   (Python slice semantics, a NEGATIVE bound included);
//   * if that is short of top_k: the dropped entries, stably sorted by score with the high tier's drops first on ties, fill
//     it up with their scores shifted by delta = first_dropped - last_kept + 1e-4, clamped at 0 -- all float64, the
//     reference's operations in the reference's order (the file is compiled with -ffp-contract=off);
//   * the closing sorted() is then the identity (kept scores descend, shifted scores descend from last_kept - 1e-4).
// diversify == 0 (config.yaml similarity.diversification false): the first top_k accepted entries.
constexpr int DV_THREADS = 1024;

__device__ __forceinline__ int dv_excl_scan(bool flag, int* wsum, int* total) {
    // exclusive prefix count of `flag` over the workgroup (thread order); *total = the count.  Two barriers.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int within = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                     // (wsum may still be read from an earlier scan)
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < DV_THREADS / 64; ++i) {
        const int c = wsum[i];
        if (i < wv) base += c;
        tot += c;
    }
    *total = tot;
    return base + within;
}

__global__ __launch_bounds__(DV_THREADS) void diversify_kernel(
    const int32_t* __restrict__ f_doc, const double* __restrict__ f_score, const double* __restrict__ f_orig,
    const int32_t* __restrict__ f_chunk, const int32_t* __restrict__ f_n, int max_cand,
    const int32_t* __restrict__ doc_domain, int64_t n_domain_docs, int top_k, double threshold, int diversify,
    int32_t* __restrict__ out_doc, double* __restrict__ out_score, double* __restrict__ out_orig,
    int32_t* __restrict__ out_chunk, int32_t* __restrict__ out_n) {
    __shared__ int32_t Ldom[RR_MAXM];
    __shared__ double Ls[RR_MAXM];
    __shared__ int16_t Lsrc[RR_MAXM];
    __shared__ uint8_t Lhi[RR_MAXM], Ldrop[RR_MAXM];
    __shared__ int wsum[DV_THREADS / 64];
    __shared__ double s_last, s_a0;
    const int q = blockIdx.x, tid = threadIdx.x;
    int n = f_n[q];
    n = n < 0 ? 0 : (n > max_cand ? max_cand : n);
    n = n > RR_MAXM ? RR_MAXM : n;
    const int64_t row = (int64_t)q * max_cand;
    // 1. accepted entries, in list order
    int dm = -1;
    double sc = 0.0;
    if (tid < n) {
        const int d = f_doc[row + tid];
        sc = f_score[row + tid];
        if (d >= 0) dm = doc_domain ? ((int64_t)d < n_domain_docs ? doc_domain[d] : -1) : d;     // (no table: every document its own domain)
    }
    int nv = 0;
    const int v = dv_excl_scan(dm >= 0, wsum, &nv);
    if (dm >= 0) { Ldom[v] = dm; Ls[v] = sc; Lsrc[v] = (int16_t)tid; }
    __syncthreads();
    auto emit = [&](int pos, int src, double score) {
        out_doc[row + pos] = f_doc[row + src]; out_score[row + pos] = score;
        out_orig[row + pos] = f_orig[row + src]; out_chunk[row + pos] = f_chunk[row + src];
    };
    int n_out = 0;
    if (!diversify) {
        n_out = nv < top_k ? nv : top_k;
        if (tid < n_out) emit(tid, Lsrc[tid], Ls[tid]);
    } else {
        // 2. first entry of each domain; tier of the domain
        bool kept = false, hi = false;
        if (tid < nv) {
            const int mine = Ldom[tid];
            int f = 0;
            while (Ldom[f] != mine) ++f;                 // (terminates at f == tid at the latest)
            kept = f == tid;
            hi = Ls[f] >= threshold;
            Lhi[tid] = hi ? 1 : 0; Ldrop[tid] = kept ? 0 : 1;
        }
        int n_kept = 0, n_hi = 0;
        const int kr = dv_excl_scan(kept, wsum, &n_kept);
        (void)dv_excl_scan(kept && hi, wsum, &n_hi);
        const int n_med = n_kept - n_hi, remaining = top_k - n_hi;
        const int take_med = remaining >= 0 ? (n_med < remaining ? n_med : remaining) : (n_med + remaining > 0 ? n_med + remaining : 0);
        const int n_final = n_hi + take_med;
        const bool in_final = kept && kr < n_final;       // (kept-high entries have kr < n_hi, kept-medium ones kr - n_hi < take_med)
        if (in_final) {
            emit(kr, Lsrc[tid], Ls[tid]);
            if (kr == n_final - 1) s_last = Ls[tid];
        }
        n_out = n_final;
        const int need = top_k - n_final, n_drop = nv - n_kept;
        if (need > 0 && n_drop > 0) {                     // (workgroup-uniform)
            // 3. the dropped entries in the order of sorted(dropped_high + dropped_medium, key=score, reverse=True)
            int rr = 0;
            const bool dropped = tid < nv && !kept;
            if (dropped) {
                const double ms = Ls[tid];
                for (int j = 0; j < nv; ++j) {
                    if (!Ldrop[j] || j == tid) continue;
                    const double js = Ls[j];
                    const bool before = js > ms || (js == ms && (Lhi[j] > (uint8_t)hi || (Lhi[j] == (uint8_t)hi && j < tid)));
                    rr += before ? 1 : 0;
                }
                if (rr == 0) s_a0 = Ls[tid];
            }
            __syncthreads();
            const int n_add = need < n_drop ? need : n_drop;
            if (dropped && rr < n_add) {
                const double delta = (s_a0 - s_last) + 1e-4;
                const double x = Ls[tid] - delta;
                emit(n_final + rr, Lsrc[tid], x > 0.0 ? x : 0.0);
            }
            n_out = n_final + n_add;
        }
    }
    for (int i = n_out + tid; i < max_cand; i += DV_THREADS) {
        out_doc[row + i] = -1; out_score[row + i] = -__builtin_inf(); out_orig[row + i] = 0.0; out_chunk[row + i] = -1;
    }
    if (tid == 0) out_n[q] = n_out;
}

// ---- the sharded rerank's compact exchange ------------------------------------------------------------------------------
// A rank of an N-way run owns ~1/N of a query's candidates: the dense halves of msr_rerank_gather_blocks are 13 words per
// SLOT, mostly zeros.  Compact: a 16-word record per OWNED slot, variable counts -- which every rank can work out for every
// (source, query) without talking to anyone, because the merged candidate lists are replicated and the shards are document
// ranges.  rerank_plan_kernel counts, rerank_offsets_kernel turns the counts into the places of the records in the send and
// receive buffers and into the N x N matrix of records per (source, destination) the host sizes the all-to-all with.
constexpr int RP_THREADS = 256;
__global__ __launch_bounds__(RP_THREADS) void rerank_plan_kernel(const int32_t* __restrict__ cand_doc,
                                                                  const int32_t* __restrict__ cand_n, int max_cand,
                                                                  const int32_t* __restrict__ bounds, int n_shards, int my,
                                                                  int nq, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ blk_off) {
    __shared__ int s_cnt[64];
    __shared__ int s_blk[RR_MAXM / RC_SLOTS + 1];
    const int q = blockIdx.x, t = threadIdx.x;
    const int n_blk = (max_cand + RC_SLOTS - 1) / RC_SLOTS;
    if (t < 64) s_cnt[t] = 0;
    __syncthreads();
    int n = cand_n[q];
    if (n > max_cand) n = max_cand;
    const int lo_my = bounds[my], hi_my = bounds[my + 1];
    for (int m0 = 0; m0 < n_blk * RC_SLOTS; m0 += RP_THREADS) {           // (whole waves: the ballot below)
        const int m = m0 + t;
        int owner = -1;
        const int d = m < n ? cand_doc[(int64_t)q * max_cand + m] : -1;
        if (d >= bounds[0] && d < bounds[n_shards]) {
            int a = 0, b = n_shards;                                       // bounds[a] <= d < bounds[b]
            while (b - a > 1) {
                const int c = (a + b) >> 1;
                if (d >= bounds[c]) a = c; else b = c;
            }
            owner = a;
        }
        if (owner >= 0) atomicAdd(&s_cnt[owner], 1);
        const unsigned long long mine = __ballot(d >= lo_my && d < hi_my);
        if ((t & (RC_SLOTS - 1)) == 0 && m < n_blk * RC_SLOTS)
            s_blk[m / RC_SLOTS] = __builtin_popcountll((mine >> (t & 63)) & ((1ull << RC_SLOTS) - 1));
    }
    __syncthreads();
    if (t < n_shards) counts[(int64_t)t * nq + q] = s_cnt[t];
    if (t == 0) {                                                          // <= 128 blocks: a serial prefix in LDS
        int acc = 0;
        for (int b = 0; b < n_blk; ++b) { const int c = s_blk[b]; s_blk[b] = acc; acc += c; }
    }
    __syncthreads();
    for (int b = t; b < n_blk; b += RP_THREADS) blk_off[(int64_t)q * n_blk + b] = s_blk[b];
}

constexpr int RO_THREADS = 1024;
// exclusive prefix of in[0 .. n) + base -> out, by one workgroup
__device__ void block_excl_scan(const int32_t* __restrict__ in, int n, int base, int32_t* __restrict__ out, int* sh) {
    const int t = threadIdx.x, per = (n + RO_THREADS - 1) / RO_THREADS;
    const int a = t * per < n ? t * per : n, b = a + per < n ? a + per : n;
    int sum = 0;
    for (int i = a; i < b; ++i) sum += in[i];
    sh[t] = sum;
    __syncthreads();
    for (int o = 1; o < RO_THREADS; o <<= 1) {
        const int v = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    int acc = base + sh[t] - sum;
    for (int i = a; i < b; ++i) { out[i] = acc; acc += in[i]; }
    __syncthreads();
}
// sum of in[0 .. n) by ONE wave (every lane gets it)
__device__ __forceinline__ int wave_sum(const int32_t* __restrict__ in, int n) {
    int sum = 0;
    for (int i = threadIdx.x & 63; i < n; i += 64) sum += in[i];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    return sum;
}
// block s < n_shards: the places of source s' records for MY queries in the receive buffer; block n_shards: the places of my
// records in the send buffer; block n_shards + 1: pair[s][o] = records source s has for the queries of rank o (a wave per
// pair, no barrier).
__global__ __launch_bounds__(RO_THREADS) void rerank_offsets_kernel(const int32_t* __restrict__ counts, int n_shards, int my,
                                                                     int nq, int qps, int32_t* __restrict__ send_base,
                                                                     int32_t* __restrict__ recv_off,
                                                                     int32_t* __restrict__ pair) {
    __shared__ int sh[RO_THREADS];
    __shared__ int s_base[64];
    const int b = blockIdx.x, w = threadIdx.x >> 6;
    const int lo = my * qps < nq ? my * qps : nq, hi = lo + qps < nq ? lo + qps : nq;
    if (b < n_shards) {
        for (int s = w; s < b; s += RO_THREADS / 64) {                     // what the sources before b send me
            const int v = wave_sum(counts + (int64_t)s * nq + lo, hi - lo);
            if ((threadIdx.x & 63) == 0) s_base[s] = v;
        }
        __syncthreads();
        int base = 0;
        for (int s = 0; s < b; ++s) base += s_base[s];
        block_excl_scan(counts + (int64_t)b * nq + lo, hi - lo, base, recv_off + (int64_t)b * qps, sh);
    } else if (b == n_shards) {
        block_excl_scan(counts + (int64_t)my * nq, nq, 0, send_base, sh);
    } else {
        for (int p = w; p < n_shards * n_shards; p += RO_THREADS / 64) {
            const int s = p / n_shards, o = p - s * n_shards;
            const int a0 = o * qps < nq ? o * qps : nq, a1 = a0 + qps < nq ? a0 + qps : nq;
            const int v = wave_sum(counts + (int64_t)s * nq + a0, a1 - a0);
            if ((threadIdx.x & 63) == 0) pair[p] = v;
        }
    }
}

// The receiving side: the records of (source s, my query j) go to their slots of the dense arrays the fuse kernel reads
// (zeroed beforehand: a slot nobody owns stays "no document").  One workgroup per (query, source).
__global__ __launch_bounds__(256) void rerank_scatter_kernel(const int32_t* __restrict__ records, int64_t capacity,
                                                              const int32_t* __restrict__ counts,
                                                              const int32_t* __restrict__ recv_off, int nq, int qps, int q_first,
                                                              int max_cand, float* __restrict__ cos_out,
                                                              int32_t* __restrict__ meta_out) {
    const int j = blockIdx.x, s = blockIdx.y;
    int cnt = counts[(int64_t)s * nq + q_first + j];
    const int64_t first = recv_off[(int64_t)s * qps + j];
    if (first < 0 || first >= capacity) return;
    if (first + cnt > capacity) cnt = (int)(capacity - first);
    const int32_t* rec = records + first * MSR_RERANK_RECORD_WORDS;
    for (int i = threadIdx.x; i < cnt * 13; i += 256) {
        const int r = i / 13, w = i - 13 * r;
        const int32_t* rr = rec + (int64_t)r * MSR_RERANK_RECORD_WORDS;
        const int slot = rr[0];
        if (slot < 0 || slot >= max_cand) continue;                       // (never, with records this library wrote)
        if (w < 3) meta_out[((int64_t)j * max_cand + slot) * 3 + w] = rr[1 + w];
        else cos_out[((int64_t)j * max_cand + slot) * RR_MAXC + (w - 3)] = __int_as_float(rr[4 + (w - 3)]);
    }
}

}  // namespace

hipError_t msr_rerank_plan_run(int nq, const int32_t* cand_doc, const int32_t* cand_n, int max_cand, const int32_t* bounds,
                               int n_shards, int my, int qps, int32_t* counts, int32_t* send_base, int32_t* blk_off,
                               int32_t* recv_off, int32_t* pair, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (max_cand <= 0 || max_cand > RR_MAXM || n_shards < 1 || n_shards > 64 || my < 0 || my >= n_shards || qps < 1)
        return hipErrorInvalidValue;
    rerank_plan_kernel<<<nq, RP_THREADS, 0, stream>>>(cand_doc, cand_n, max_cand, bounds, n_shards, my, nq, counts, blk_off);
    rerank_offsets_kernel<<<n_shards + 2, RO_THREADS, 0, stream>>>(counts, n_shards, my, nq, qps, send_base, recv_off, pair);
    return hipGetLastError();
}

hipError_t msr_rerank_scatter_run(const int32_t* records, int64_t capacity, const int32_t* counts, const int32_t* recv_off, int n_shards, int nq,
                                  int qps, int q_first, int n_mine, int max_cand, float* cos_out, int32_t* meta_out,
                                  hipStream_t stream) {
    if (n_mine <= 0) return hipSuccess;
    if (max_cand <= 0 || max_cand > RR_MAXM || n_shards < 1 || n_shards > 64) return hipErrorInvalidValue;
    hipError_t err = hipMemsetAsync(cos_out, 0, (size_t)n_mine * max_cand * RR_MAXC * 4, stream);
    if (err != hipSuccess) return err;
    err = hipMemsetAsync(meta_out, 0, (size_t)n_mine * max_cand * 3 * 4, stream);
    if (err != hipSuccess) return err;
    rerank_scatter_kernel<<<dim3((unsigned)n_mine, (unsigned)n_shards), 256, 0, stream>>>(records, capacity, counts, recv_off, nq, qps,
                                                                                           q_first, max_cand, cos_out, meta_out);
    return hipGetLastError();
}

hipError_t msr_diversify_run(int nq, const int32_t* f_doc, const double* f_score, const double* f_orig, const int32_t* f_chunk,
                             const int32_t* f_n, int max_cand, const int32_t* doc_domain, int64_t n_domain_docs, int top_k,
                             double threshold, int diversify, int32_t* out_doc, double* out_score, double* out_orig,
                             int32_t* out_chunk, int32_t* out_n, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (max_cand <= 0 || max_cand > RR_MAXM || top_k < 1) return hipErrorInvalidValue;
    diversify_kernel<<<nq, DV_THREADS, 0, stream>>>(f_doc, f_score, f_orig, f_chunk, f_n, max_cand, doc_domain, n_domain_docs,
                                                    top_k, threshold, diversify, out_doc, out_score, out_orig, out_chunk, out_n);
    return hipGetLastError();
}

hipError_t msr_rerank_gather(const DenseIndex& ix, const int32_t* url_group, const float* qn, int nq,
                             const int32_t* cand_doc, const int32_t* cand_n, int max_cand, int doc_base,
                             int row_base, int max_chunks, float* cos_out, int32_t* meta, int q_per_block,
                             int64_t block_stride, const RerankRecords& rec, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (max_cand <= 0 || max_cand > RR_MAXM || max_chunks <= 0 || max_chunks > RR_MAXC || q_per_block < 1) return hipErrorInvalidValue;
    if (rec.out == nullptr && (int64_t)nq * max_cand <= 16384) {      // a few queries: one wave per slot
        dim3 grid1((unsigned)max_cand, (unsigned)nq);
        if (ix.layout == 1)
            rerank_cos_kernel<true, 1><<<grid1, 64, 0, stream>>>(ix, url_group, qn, cand_doc, cand_n, max_cand, doc_base,
                                                                 row_base, max_chunks, cos_out, meta, q_per_block, block_stride, rec);
        else
            rerank_cos_kernel<false, 1><<<grid1, 64, 0, stream>>>(ix, url_group, qn, cand_doc, cand_n, max_cand, doc_base,
                                                                  row_base, max_chunks, cos_out, meta, q_per_block, block_stride, rec);
        return hipGetLastError();
    }
    dim3 grid((unsigned)((max_cand + RC_SLOTS - 1) / RC_SLOTS), (unsigned)nq);
    if (ix.layout == 1)
        rerank_cos_kernel<true><<<grid, 64, 0, stream>>>(ix, url_group, qn, cand_doc, cand_n, max_cand, doc_base,
                                                         row_base, max_chunks, cos_out, meta, q_per_block, block_stride, rec);
    else
        rerank_cos_kernel<false><<<grid, 64, 0, stream>>>(ix, url_group, qn, cand_doc, cand_n, max_cand, doc_base,
                                                          row_base, max_chunks, cos_out, meta, q_per_block, block_stride, rec);
    return hipGetLastError();
}

// out[i] = OR over parts p of in[p][i]: the join of the per-shard halves of msr_rerank_gather.  Exactly one shard wrote a
// non-zero word for a candidate (the owner of its document), every other shard wrote 0, so the OR -- like the integer sum the
// all-reduce form used -- IS that shard's word.  16 bytes per thread and step.
__global__ __launch_bounds__(256) void or_parts_kernel(const uint4* __restrict__ in, int n_parts, int64_t part_stride16,
                                                        int64_t n16, uint4* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        uint4 v = in[i];
        for (int p = 1; p < n_parts; ++p) {
            const uint4 u = in[p * part_stride16 + i];
            v.x |= u.x; v.y |= u.y; v.z |= u.z; v.w |= u.w;
        }
        out[i] = v;
    }
}
__global__ __launch_bounds__(256) void or_parts_tail_kernel(const uint32_t* __restrict__ in, int n_parts, int64_t part_stride,
                                                             int64_t first, int64_t n, uint32_t* __restrict__ out) {
    const int64_t i = first + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t v = in[i];
    for (int p = 1; p < n_parts; ++p) v |= in[p * part_stride + i];
    out[i] = v;
}

hipError_t msr_rerank_fuse_run(int nq, const int32_t* cand_doc, const double* cand_bm25, const int32_t* cand_n,
                               int max_cand, const RerankParams& p, const float* cos_in, const int32_t* meta,
                               int32_t* out_doc, double* out_score, double* out_orig, int32_t* out_chunk,
                               int32_t* out_n, int32_t* out_rows, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (max_cand <= 0 || max_cand > RR_MAXM || p.max_chunks <= 0 || p.max_chunks > RR_MAXC) return hipErrorInvalidValue;
    rerank_fuse_kernel<<<nq, RR_THREADS, 0, stream>>>(cand_doc, cand_bm25, cand_n, max_cand, p, cos_in, meta, out_doc,
                                                      out_score, out_orig, out_chunk, out_n, out_rows);
    return hipGetLastError();
}

// out[0 .. n_words) = OR over the n_parts arrays in + p * part_stride_bytes (32-bit words; every pointer and the stride
// 4-byte aligned, 16-byte aligned ones take the wide path)
hipError_t msr_or_parts(const void* in, int n_parts, int64_t part_stride_bytes, int64_t n_words, void* out, hipStream_t stream) {
    if (n_words <= 0) return hipSuccess;
    const bool wide = (((uintptr_t)in | (uintptr_t)out | (uint64_t)part_stride_bytes) & 15) == 0;
    const int64_t n16 = wide ? n_words / 4 : 0;
    if (n16 > 0) {
        const unsigned grid = (unsigned)((n16 + 255) / 256 < 4096 ? (n16 + 255) / 256 : 4096);
        or_parts_kernel<<<grid, 256, 0, stream>>>((const uint4*)in, n_parts, part_stride_bytes / 16, n16, (uint4*)out);
    }
    const int64_t rest = n_words - 4 * n16;
    if (rest > 0)
        or_parts_tail_kernel<<<(unsigned)((rest + 255) / 256), 256, 0, stream>>>((const uint32_t*)in, n_parts, part_stride_bytes / 4,
                                                                              4 * n16, n_words, (uint32_t*)out);
    return hipGetLastError();
}

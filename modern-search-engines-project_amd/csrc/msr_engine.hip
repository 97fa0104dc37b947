// C ABI of libmsretr (see include/msretr.h): engine object, scratch, argument checks, kernel sequencing.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/msretr.h"
#include "msr_devmem.h"
#include "msr_internal.h"
#include "msr_match_args.h"

struct HipMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
using Group = DevGroup<HipMem>;

struct msr_engine {
    msr_config cfg;
    char err[512];
    // Engine-owned device memory, one group per lifetime; every allocation is in exactly one, msr_owned_bytes() is their sum.
    // The groups remember the addresses of the pointer members below: an engine lives on the heap and never moves.
    Group mem_engine;                  // until msr_destroy: per-query scratch, the grow-only scratch of the similar-documents calls
    Group mem_corpus;                  // until msr_unbind: grow-only scratch sized by the corpus (score_rows, bm_cand_doc)
    Group mem_postings;                // until drop_postings: the next msr_bind_postings, msr_unbind
    Group mem_chunks;                  // until drop_chunks: the next msr_bind_chunks, msr_unbind
    Group mem_bf16;                    // what msr_enable_bf16 builds; goes with the chunks
    // bound index parts (borrowed device pointers)
    Bm25Index bm25{};
    bool have_postings = false;
    const int64_t* tok_off = nullptr;      // msr_bind_tokens (borrowed): the forward index of the bound postings' documents
    const int32_t* tok_ids = nullptr;
    int64_t n_tokens = 0;
    bool have_tokens = false;
    const int64_t* voc_char_off = nullptr; // msr_bind_vocab (borrowed): the bound postings' terms as code points, their weights
    const uint16_t* voc_chars = nullptr;
    const uint32_t* voc_weight = nullptr;
    int64_t voc_n_chars = 0;
    bool have_vocab = false;
    FacetTable facet{};                    // msr_bind_facet (borrowed): the facet table of the bound postings' documents (K17)
    bool have_facet = false;
    const uint32_t* sig = nullptr;         // msr_bind_signatures (borrowed): [sig_n][MSR_SIG_WORDS] min-hash signatures (K18)
    int64_t sig_n = 0;
    DenseIndex dense{};
    bool have_chunks = false;
    const int32_t* url_group = nullptr;
    int64_t url_group_n = 0;
    const int32_t* doc_domain = nullptr;   // msr_bind_doc_domains (borrowed): domain id per document, -1 = rejected from responses
    int64_t doc_domain_n = 0;
    // engine-owned device memory.  mem_chunks:
    int32_t* chunk_doc = nullptr;
    void* emb_presplit = nullptr;     // MSR_SCAN_PRESPLIT: f16 hi/lo image of the rows
    void* row_meta = nullptr;         // packed {document, inverse norm} per row for the K-split kernels
    float* inv_norm_own = nullptr;
    int32_t* span_doc = nullptr;
    int32_t* wspan_doc = nullptr;
    // mem_engine:
    float* qn = nullptr;              // [128][768] normalised queries of the current slice
    float* rr_qn = nullptr;           // [max(max_queries, 128)][768] normalised queries of a rerank gather (one launch per call)
    void* qimg = nullptr;             // query image in fragment order (<= 256 KB)
    SelScratch sel{};
    float* rerank_cos = nullptr;
    int32_t* rerank_meta = nullptr;
    // mem_corpus:
    void* score_rows = nullptr;       // max_queries rows of n_docs float64 (reused as float32 rows)
    size_t score_rows_bytes = 0;
    int32_t* bm_cand_doc = nullptr;    // max_queries rows of n_docs i32: document of each BM25 candidate
    size_t bm_cand_bytes = 0;
    // mem_postings:
    int32_t* bm_heavy_id = nullptr;    // skip table of the BM25 stage (see Bm25Index)
    void* bm_post = nullptr;           // {doc, tf, tf_component} copy of the postings (see Bm25Index)
    int32_t* bm_dense_id = nullptr;    // dense tf_component tables of the long negative-idf lists (see Bm25Index)
    double* bm_dense = nullptr;
    uint32_t* bm_tile_off = nullptr;
    int32_t* bm_cand_n = nullptr;      // [max_queries][tiles] candidates per (query, segment) of the candidate rows
    uint64_t* bm_win = nullptr;        // [max_queries] anchor of the select's window pass (msr_bm25_scores' plan kernel)
    int32_t* bm_order = nullptr;       // [max_queries + 1] item order of the scoring kernel (the same plan kernel)
    uint64_t* voc_sig = nullptr;       // [n_terms] character-set signatures of the bound vocabulary (msr_bind_vocab, K15)
    // mem_engine: candidate scratch of the batched bf16 path (allocated by the first msr_enable_bf16, kept across re-binds)
    int32_t* bt_top_doc = nullptr; float* bt_top_score = nullptr; int32_t* bt_top_n = nullptr;
    int32_t* bt_cand_doc = nullptr; float* bt_cand_score = nullptr; int32_t* bt_cand_chunk = nullptr;
    int32_t* bt_cand_n = nullptr;
    // mem_chunks: row tiles of <= 256 rows cut at document boundaries (both GEMM paths); built when the chunks are bound
    int32_t* tile_row = nullptr;
    int n_tiles = 0;
    bool tiles_ok = false;             // every document fits one tile
    // default scan for 65..128 queries as a tiled GEMM over the f32 rows (msr_gemm_f32.hip).  mem_chunks; its scratch is
    // allocated straight into `gf`: here is only what `gf` holds as const and what the engine itself uses
    GemmF32Index gf{};
    bool gf_ok = false;
    float* gf_inv_pad = nullptr; float* gf_qn = nullptr; void* gf_fb_qimg = nullptr;
    int32_t* gf_gate = nullptr;       // GF_GATE_BYTES
    void* gf_emb_tiled = nullptr;     // fragment-order copy of the f32 rows (256-query streaming pass)
    void* gf_emb_f16 = nullptr;       // row-major f16 image of the rows (launches of several 256-query groups)
    int32_t* tile_trow = nullptr;     // [n_tiles] first row of each tile in those copies
    // batched path as a tiled GEMM (msr_gemm.hip): unit-row bf16 image + tile table + scratch for GM_SLICE queries per pass.
    // mem_bf16; the GEMM's scratch is allocated straight into `gemm`
    void* emb_bf16 = nullptr;          // bf16 copy of the embeddings; non-null = msr_enable_bf16 has built the whole path
    GemmIndex gemm{};
    bool gemm_ok = false;
    float* gm_qn = nullptr;
    uint32_t* bf_err = nullptr;        // bits of the largest rounding-error norm of an image row (see msr_batch_margin)
    float* bf_margin = nullptr;        // [GM_SLICE] candidate margin of each query of the current slice
    float* bf_ones = nullptr;          // inverse norms of the unit-row image (all 1) for the <= 128-query bf16 sweeps
    void* bf_row_meta = nullptr;       // {document, 1.0f} per row for the K-split bf16 sweeps
    DenseIndex dense_bf16{};           // `dense` with the unit-row image, its inverse norms and row meta
    int n_cus = 256;
    int split_pending = 0;             // queries of an msr_dense_topk_begin whose msr_dense_topk_end has not come yet
    int row_copy_state = 0;            // fragment-order copy of the rows: 0 not wanted / not applicable, 1 built, 2 declined by
                                       // msr_config.flags, 3 allocation failed (the row-major instantiation of the kernel runs)
    int row_image_state = 0;           // f16 image of the rows (launches of several query groups): the same four states
    int last_dense_width = 0;          // queries per pass over the matrix of the most recent msr_dense_topk call (msr_dense_path)
    int last_dense_segments = 0;       // emit launches per query group of the most recent streaming call (msr_dense_pass_info)
    // mem_engine: msr_gather_rows / msr_dense_topk_grouped (grown on demand, kept until msr_destroy): a check flag, the per-row
    // lists, the per-row set indices and the merge's overflow records
    int32_t* sim_flag = nullptr;
    void* sim_lists = nullptr; size_t sim_lists_bytes = 0;
    void* sim_over = nullptr; size_t sim_over_bytes = 0;
    int64_t* dirty_counts = nullptr;   // mem_engine: the device counts of msr_debug_scratch_dirty (allocated by its first call)
    // timing
    bool timing = false;
    static constexpr int EV_RING = 256;
    static constexpr int EV_KINDS = 4; // 0 dense scan, 1 BM25 TAAT, 2 GEMM emit pass, 3 GEMM sample pass
    hipEvent_t ev_start[EV_KINDS][EV_RING] = {};
    hipEvent_t ev_stop[EV_KINDS][EV_RING] = {};
    int ev_count[EV_KINDS] = {0, 0, 0, 0};   // launches recorded since msr_set_timing(1)
};

// gf_gate: the gate words of the streaming pass, one per slice of 64 queries of a call (at most 8 groups of 128 queries)
static constexpr size_t GF_GATE_BYTES = 16 * sizeof(int32_t);

static thread_local char g_create_err[512] = "";

static int fail(msr_engine* e, int code, const char* fmt, ...) {
    char* dst = e ? e->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(e, call)                                                                          \
    do {                                                                                          \
        hipError_t _err = (call);                                                                 \
        if (_err != hipSuccess) return fail(e, MSR_ERR_HIP, "%s: %s", #call, hipGetErrorString(_err)); \
    } while (0)

// slot <- `bytes` of device memory owned by `group`; a failure returns MSR_ERR_NOMEM with the slot's name in the error text
#define ALLOC(e, group, slot, bytes)                                                              \
    do {                                                                                          \
        const size_t _n = (bytes);                                                                \
        hipError_t _err = (group).alloc(&(slot), _n);                                             \
        if (_err != hipSuccess) return fail(e, MSR_ERR_NOMEM, "%s (%zu bytes): %s", #slot, _n, hipGetErrorString(_err)); \
    } while (0)

// How a binding goes away, in msr_unbind, in msr_destroy and in each bind where it starts to replace state: the flags and the
// index structs first, then the memory, so that nothing is left pointing at what is freed.
static void drop_vocab(msr_engine* e) {
    e->have_vocab = false;
    e->voc_char_off = nullptr; e->voc_chars = nullptr; e->voc_weight = nullptr; e->voc_n_chars = 0;
    e->mem_postings.free_one(&e->voc_sig);
}
static void drop_facet(msr_engine* e) {
    e->have_facet = false;
    e->facet = FacetTable{};
}
static void drop_postings(msr_engine* e) {
    e->have_postings = e->have_tokens = false;
    drop_facet(e);
    e->sig = nullptr; e->sig_n = 0;
    e->tok_off = nullptr; e->tok_ids = nullptr; e->n_tokens = 0;
    drop_vocab(e);
    e->bm25 = Bm25Index{};
    e->mem_postings.release();
}
static void drop_bf16(msr_engine* e) {
    e->dense.emb_bf16 = nullptr;
    e->dense_bf16 = DenseIndex{};
    e->gemm = GemmIndex{};
    e->gemm_ok = false;
    e->mem_bf16.release();
}
static void drop_chunks(msr_engine* e) {
    e->have_chunks = false;
    e->split_pending = 0;                                    // (a pending begin's scratch goes too)
    e->dense = DenseIndex{};
    e->gf = GemmF32Index{};
    e->gf_ok = e->tiles_ok = false;
    e->n_tiles = 0;
    e->row_copy_state = e->row_image_state = 0;
    drop_bf16(e);
    e->mem_chunks.release();
}

// Grow-only scratch: afterwards *slot holds at least `need` bytes (*have: how many it holds).
template <class T>
static int grow(msr_engine* e, Group& group, T** slot, size_t* have, size_t need, const char* what) {
    if (need <= *have && *slot) return MSR_OK;
    group.free_one(slot);
    *have = 0;
    hipError_t herr = group.alloc(slot, need);
    if (herr != hipSuccess) return fail(e, MSR_ERR_NOMEM, "%s (%zu bytes): %s", what, need, hipGetErrorString(herr));
    *have = need;
    return MSR_OK;
}

extern "C" int msr_abi_version(void) { return MSR_ABI_VERSION; }

extern "C" const char* msr_last_error(const msr_engine* e) { return e ? e->err : g_create_err; }

// error text of the handle-less entry points (msr_encoder.hip): read back with msr_last_error(NULL)
int msr_fail_global(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_create_err, sizeof(g_create_err), fmt, ap);
    va_end(ap);
    return code;
}

// Device state of a new engine: the per-query scratch (mem_engine) and the timing events.
static int create_scratch(msr_engine* e) {
    const msr_config& cfg = e->cfg;
    HIP_TRY(e, hipSetDevice(cfg.device));
    hipDeviceProp_t prop;
    HIP_TRY(e, hipGetDeviceProperties(&prop, cfg.device));
    e->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // select scratch and query buffers cover the widest sweep (128 queries) whatever max_queries says
    const size_t nq = (size_t)std::max(cfg.max_queries, 128);
    ALLOC(e, e->mem_engine, e->qn, 128 * MSR_DIM * sizeof(float));
    ALLOC(e, e->mem_engine, e->qimg, 256 * 1024);
    if (cfg.rerank_max_docs > 0) ALLOC(e, e->mem_engine, e->rr_qn, nq * MSR_DIM * sizeof(float));
    ALLOC(e, e->mem_engine, e->sel.hist, nq * MSR_SEL_BINS * sizeof(uint32_t));
    ALLOC(e, e->mem_engine, e->sel.state, nq * sizeof(SelState));
    ALLOC(e, e->mem_engine, e->sel.cand_hi, nq * MSR_SEL_CAP * sizeof(uint64_t));
    ALLOC(e, e->mem_engine, e->sel.cand_lo, nq * MSR_SEL_CAP * sizeof(uint32_t));
    ALLOC(e, e->mem_engine, e->sel.cand_n, nq * sizeof(int32_t));
    // "zero between calls" from the start: cleared on the null stream and waited for here, so that the engine's first call finds
    // them done on whatever stream it comes -- a non-blocking stream does not wait for the null stream (creation is no hot path)
    HIP_TRY(e, hipMemsetAsync(e->sel.hist, 0, nq * MSR_SEL_BINS * sizeof(uint32_t), nullptr));
    HIP_TRY(e, hipMemsetAsync(e->sel.cand_n, 0, nq * sizeof(int32_t), nullptr));
    HIP_TRY(e, hipStreamSynchronize(nullptr));
    if (cfg.rerank_max_docs > 0) {
        ALLOC(e, e->mem_engine, e->rerank_cos, nq * (size_t)cfg.rerank_max_docs * MSR_RERANK_MAX_CHUNKS * sizeof(float));
        ALLOC(e, e->mem_engine, e->rerank_meta, nq * (size_t)cfg.rerank_max_docs * 3 * sizeof(int32_t));
    }
    for (int w = 0; w < msr_engine::EV_KINDS; ++w)
        for (int j = 0; j < msr_engine::EV_RING; ++j) {
            HIP_TRY(e, hipEventCreate(&e->ev_start[w][j]));
            HIP_TRY(e, hipEventCreate(&e->ev_stop[w][j]));
        }
    return MSR_OK;
}

extern "C" int msr_create(const msr_config* cfg, msr_engine** out) {
    if (!cfg || !out) return fail(nullptr, MSR_ERR_INVALID, "msr_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(msr_config))
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: struct_size %d != %zu", cfg->struct_size, sizeof(msr_config));
    if (cfg->dim != MSR_DIM) return fail(nullptr, MSR_ERR_INVALID, "msr_create: dim must be %d", MSR_DIM);
    if (cfg->max_queries < 1 || cfg->max_queries > 4096)
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: max_queries out of range [1, 4096]");
    if (cfg->max_k < 1 || cfg->max_k > MSR_MAX_K)
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: max_k out of range [1, %d]", MSR_MAX_K);
    if (cfg->rerank_max_docs < 0 || cfg->rerank_max_docs > 1024)
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: rerank_max_docs out of range [0, 1024]");
    if (cfg->scan_layout != 0 && cfg->scan_layout != 1)
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: scan_layout must be 0 or 1");
    if (cfg->scan_variant != MSR_SCAN_AUTO && !dense_variant_known(cfg->scan_variant))
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: scan_variant must be 0, 2, 7, 14 or 15");
    if (cfg->flags & ~(int32_t)(MSR_CFG_NO_ROW_COPY | MSR_CFG_SINGLE_EMIT))
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: unknown flag bits 0x%x", cfg->flags);
    int ndev = 0;
    hipError_t herr = hipGetDeviceCount(&ndev);
    if (herr != hipSuccess || ndev <= 0)
        return fail(nullptr, MSR_ERR_HIP, "msr_create: no HIP device available (%s)",
                    herr == hipSuccess ? "device count is 0" : hipGetErrorString(herr));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, MSR_ERR_INVALID, "msr_create: device %d out of range (have %d)", cfg->device, ndev);
    msr_engine* e = new (std::nothrow) msr_engine();
    if (!e) return fail(nullptr, MSR_ERR_NOMEM, "msr_create: out of host memory");
    e->cfg = *cfg;
    e->err[0] = 0;
    const int rc = create_scratch(e);
    if (rc) {
        fail(nullptr, rc, "msr_create: %s", e->err);
        msr_destroy(e);
        return rc;
    }
    *out = e;
    return MSR_OK;
}

extern "C" int msr_destroy(msr_engine* e) {
    if (!e) return MSR_OK;
    drop_postings(e);
    drop_chunks(e);
    for (int w = 0; w < msr_engine::EV_KINDS; ++w)
        for (int j = 0; j < msr_engine::EV_RING; ++j) {
            if (e->ev_start[w][j]) (void)hipEventDestroy(e->ev_start[w][j]);
            if (e->ev_stop[w][j]) (void)hipEventDestroy(e->ev_stop[w][j]);
        }
    delete e;                                                // (the groups release what is left: mem_engine, mem_corpus)
    return MSR_OK;
}

// (Re)size the per-slice score rows: max_queries rows of n_docs float64.
static int ensure_score_rows(msr_engine* e, int64_t n_docs) {
    // f64 candidate scores of max_queries queries, or f32 score rows (padded to 32 documents) of up to 128 queries
    const size_t pad = (size_t)(n_docs + 31) / 32 * 32;
    const size_t need = std::max((size_t)e->cfg.max_queries * pad * sizeof(double), (size_t)128 * pad * sizeof(float));
    return grow(e, e->mem_corpus, &e->score_rows, &e->score_rows_bytes, need, "score rows");
}

// The engine's tables and scratch for the posting index `cand`, which is checked on the way.  The engine is unbound meanwhile.
static int build_postings(msr_engine* e, Bm25Index cand, hipStream_t st) {
    const int64_t n_terms = cand.n_terms, n_postings = cand.n_postings, n_docs = cand.n_docs;
    int rc = ensure_score_rows(e, n_docs);
    if (rc) return rc;
    // candidate lists of the BM25 stage: worst case every document of every query
    rc = grow(e, e->mem_corpus, &e->bm_cand_doc, &e->bm_cand_bytes, (size_t)e->cfg.max_queries * (size_t)n_docs * sizeof(int32_t),
              "BM25 candidate lists");
    if (rc) return rc;
    ALLOC(e, e->mem_postings, e->bm_win, (size_t)e->cfg.max_queries * sizeof(uint64_t));
    ALLOC(e, e->mem_postings, e->bm_order, ((size_t)e->cfg.max_queries + 1) * sizeof(int32_t));
    ALLOC(e, e->mem_postings, e->bm_cand_n, (size_t)e->cfg.max_queries * msr_bm25_max_segments(n_docs) * sizeof(int32_t));
    // the scoring kernel indexes LDS with (post_doc - tile start): validate the CSR once, on the device
    int32_t h_flag = 0;
    HIP_TRY(e, msr_bm25_validate(cand, e->sel.cand_n, st));           // cand_n[0] as a scratch word (zero between calls)
    HIP_TRY(e, hipMemcpyAsync(&h_flag, e->sel.cand_n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipMemsetAsync(e->sel.cand_n, 0, sizeof(int32_t), st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (h_flag >= 1 && h_flag <= 5) {
        static const char* why[] = {"", "term_off is not a monotone offset array ending at n_postings",
                                    "a posting's document index is outside [0, n_docs)",
                                    "documents are not strictly ascending inside a posting list",
                                    "negative doc_len", "non-positive term frequency"};
        return fail(e, MSR_ERR_INVALID, "msr_bind_postings: malformed index: %s", why[h_flag]);
    }
    if (!(cand.avgdl > 0.0) || !(cand.k1 >= 0.0) || !(cand.b >= 0.0 && cand.b <= 1.0))
        return fail(e, MSR_ERR_INVALID, "msr_bind_postings: avgdl must be > 0, k1 >= 0, 0 <= b <= 1");
    // skip table for the long posting lists (one-time; the offsets come to the host once for this)
    std::vector<int32_t> dense_terms;                         // long lists with negative idf, longest first (tables below)
    if (n_terms > 0) {
        std::vector<int64_t> h_toff((size_t)n_terms + 1);
        std::vector<float> h_idf((size_t)n_terms);
        HIP_TRY(e, hipMemcpyAsync(h_toff.data(), cand.term_off, h_toff.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipMemcpyAsync(h_idf.data(), cand.idf, h_idf.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        std::vector<int32_t> heavy_id((size_t)n_terms, -1), heavy_terms;
        for (int64_t t = 0; t < n_terms; ++t)
            if (h_toff[t + 1] - h_toff[t] >= MSR_BM25_HEAVY_DF && h_toff[t + 1] - h_toff[t] < (1ll << 32)) {
                heavy_id[t] = (int32_t)heavy_terms.size();
                heavy_terms.push_back((int32_t)t);
                if (h_idf[t] < 0.0f) dense_terms.push_back((int32_t)t);
            }
        if (!heavy_terms.empty()) {
            DevTemp<HipMem, int32_t> d_terms;                // (freed at the end of this block on every path; hipFree waits for the device)
            const size_t rows = heavy_terms.size() * (size_t)(cand.n_tiles + 1);
            ALLOC(e, e->mem_postings, e->bm_heavy_id, heavy_id.size() * sizeof(int32_t));
            ALLOC(e, e->mem_postings, e->bm_tile_off, rows * sizeof(uint32_t));
            ALLOC(e, d_terms.group, d_terms.p, heavy_terms.size() * sizeof(int32_t));
            HIP_TRY(e, hipMemcpyAsync(e->bm_heavy_id, heavy_id.data(), heavy_id.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(e, hipMemcpyAsync(d_terms.p, heavy_terms.data(), heavy_terms.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(e, msr_bm25_build_skip(cand, d_terms.p, (int)heavy_terms.size(), e->bm_tile_off, st));
            HIP_TRY(e, hipStreamSynchronize(st));
            cand.heavy_id = e->bm_heavy_id;
            cand.tile_off = e->bm_tile_off;
        }
        // the longest negative-idf lists get a dense table: at most MSR_BM25_MAX_DENSE of them and 4 GiB in all
        std::stable_sort(dense_terms.begin(), dense_terms.end(), [&](int32_t a, int32_t b2) {
            return h_toff[a + 1] - h_toff[a] > h_toff[b2 + 1] - h_toff[b2];
        });
        const size_t row_bytes = ((size_t)cand.n_tiles * MSR_BM25_TILE + 8) * sizeof(double);
        const size_t cap = std::min<size_t>(MSR_BM25_MAX_DENSE, (size_t)(4ull << 30) / row_bytes);
        if (dense_terms.size() > cap) dense_terms.resize(cap);
    }
    // the copy the scoring kernel streams (after the validation above: the copy is of a well-formed index): every posting with
    // its tf_component, from the per-document length norms k1 (1 - b + b dl / avgdl)
    {
        const int64_t n_pad = (int64_t)cand.n_tiles * MSR_BM25_TILE;
        DevTemp<HipMem, double> dnorm;
        ALLOC(e, e->mem_postings, e->bm_post, (size_t)(n_postings + 1) * sizeof(Bm25Post));      // + the sentinel posting
        ALLOC(e, dnorm.group, dnorm.p, (size_t)n_pad * sizeof(double));
        HIP_TRY(e, msr_bm25_dnorm(cand.doc_len, n_docs, n_pad, cand.k1, cand.b, cand.avgdl, dnorm.p, st));
        HIP_TRY(e, msr_bm25_post_comp(cand.post_doc, cand.post_tf, dnorm.p, cand.k1, n_postings, (Bm25Post*)e->bm_post, st));
        HIP_TRY(e, hipStreamSynchronize(st));
    }
    cand.post = (const Bm25Post*)e->bm_post;
    if (!dense_terms.empty()) {
        const int64_t stride = (int64_t)cand.n_tiles * MSR_BM25_TILE + 8;      // the tail of a row stays 0.0 (the kernel's "no value")
        std::vector<int32_t> dense_id((size_t)n_terms, -1);
        for (size_t h = 0; h < dense_terms.size(); ++h) dense_id[dense_terms[h]] = (int32_t)h;
        DevTemp<HipMem, int32_t> d_terms;
        ALLOC(e, e->mem_postings, e->bm_dense_id, dense_id.size() * sizeof(int32_t));
        ALLOC(e, e->mem_postings, e->bm_dense, dense_terms.size() * (size_t)stride * sizeof(double));
        ALLOC(e, d_terms.group, d_terms.p, dense_terms.size() * sizeof(int32_t));
        HIP_TRY(e, hipMemcpyAsync(e->bm_dense_id, dense_id.data(), dense_id.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(e, hipMemcpyAsync(d_terms.p, dense_terms.data(), dense_terms.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(e, hipMemsetAsync(e->bm_dense, 0, dense_terms.size() * (size_t)stride * sizeof(double), st));
        HIP_TRY(e, msr_bm25_build_dense(cand, d_terms.p, (int)dense_terms.size(), e->bm_dense, stride, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        cand.dense_id = e->bm_dense_id;
        cand.dense_comp = e->bm_dense;
        cand.dense_stride = stride;
    }
    e->bm25 = cand;
    return MSR_OK;
}

extern "C" int msr_bind_postings(msr_engine* e, const int64_t* term_off, int64_t n_terms, const int32_t* post_doc,
                                 const int32_t* post_tf, int64_t n_postings, const int32_t* doc_len, int64_t n_docs,
                                 const float* idf, float avgdl, double k1, double b, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!term_off || !doc_len || !idf || n_terms < 0 || n_postings < 0 || n_docs <= 0 || n_docs >= (1ll << 31) ||
        (n_postings > 0 && (!post_doc || !post_tf)))
        return fail(e, MSR_ERR_INVALID, "msr_bind_postings: bad argument");
    if (e->have_chunks && e->dense.n_docs != n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_postings: n_docs %lld differs from bound chunks (%lld)",
                    (long long)n_docs, (long long)e->dense.n_docs);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // from here on the previous binding's tables are being replaced: the engine counts as unbound until this call succeeds
    // (a failed re-bind must not leave msr_bm25_topk reading freed tables)
    drop_postings(e);
    const Bm25Index cand{term_off, post_doc, post_tf, doc_len, idf, n_terms, n_postings, n_docs, (double)avgdl, k1, b,
                         nullptr, nullptr, (int32_t)((n_docs + MSR_BM25_TILE - 1) / MSR_BM25_TILE), nullptr, nullptr, nullptr, 0};
    const int rc = build_postings(e, cand, (hipStream_t)stream);
    if (rc) drop_postings(e);                                // (nothing half-built stays behind)
    e->have_postings = rc == MSR_OK;
    return rc;
}

// ---- msr_bind_chunks in three steps: what doc_off says (host only), the device tables, the streaming pass ------------------
struct ChunkLayout {
    std::vector<int32_t> spans, wspans;             // equal-chunk-count spans cut at document boundaries
    int wide_ok = 1, wide_ok64 = 1;                 // see DenseIndex
    bool tiles_ok = true;                           // every document fits a row tile of <= 256 rows (else: no GEMM paths)
    std::vector<int32_t> tiles;                     // [n_tiles + 1] first row of each tile
    std::vector<int32_t> trow;                      // [n_tiles] first row of each tile in the fragment-order copy of the rows, which
    int64_t n_trows = 0;                            // has n_trows rows (empty, 0: the copy would have 2^31 rows or more)
};

// Checks the document offsets (host copy) and works out everything the bind derives from them.  No device calls.
// (e: whose error text a refusal writes, null for the handle-less debug call; n_cus: workgroups of the K-split kernels.)
static int chunk_layout(msr_engine* e, int n_cus, const std::vector<int32_t>& h_off, int64_t n_chunks, int64_t n_docs,
                        ChunkLayout& L) {
    if (h_off[0] != 0 || (int64_t)h_off[n_docs] != n_chunks)
        return fail(e, MSR_ERR_INVALID, "msr_bind_chunks: doc_off[0]=%d, doc_off[n_docs]=%d, n_chunks=%lld",
                    h_off[0], h_off[n_docs], (long long)n_chunks);
    for (int64_t d = 0; d < n_docs; ++d)
        if (h_off[d + 1] < h_off[d]) return fail(e, MSR_ERR_INVALID, "msr_bind_chunks: doc_off not monotone at %lld", (long long)d);
    // one span per workgroup of the K-split kernels / per wave of the wave-streaming kernel
    auto make_spans = [&](int target, int64_t min_rows) {
        if ((int64_t)target * min_rows > n_chunks) target = (int)std::max<int64_t>(1, n_chunks / min_rows);
        std::vector<int32_t> sp;
        sp.push_back(0);
        for (int s = 1; s < target; ++s) {
            const int64_t want = n_chunks * s / target;
            int64_t d = std::lower_bound(h_off.begin(), h_off.end(), (int32_t)want) - h_off.begin();   // first doc starting at >= want
            if (d > n_docs) d = n_docs;
            if (d > sp.back()) sp.push_back((int32_t)d);
        }
        if (sp.back() != (int32_t)n_docs) sp.push_back((int32_t)n_docs);
        return sp;
    };
    L.spans = make_spans(n_cus, 256);
    L.wspans = make_spans(n_cus * 8, 64);
    // K-split kernels: documents spanned by any two consecutive 16-row groups must fit the LDS ring with a block to spare
    {
        const int64_t n_groups = (n_chunks + 15) / 16;
        int64_t dl = 0, dr = 0;                              // document of the window's first / last row
        for (int64_t u = 0; u < n_groups && (L.wide_ok || L.wide_ok64); ++u) {
            const int64_t first = 16 * u, last = std::min<int64_t>(16 * (u + 2), n_chunks) - 1;
            while (h_off[dl + 1] <= first) ++dl;
            if (dr < dl) dr = dl;
            while (h_off[dr + 1] <= last) ++dr;
            if (dr - dl + 32 > MSR_WIDE_RING) L.wide_ok = 0;
            if (dr - dl + 32 > 64) L.wide_ok64 = 0;
            // ... and one group at most 32 documents: the kernel writes at most two finished blocks per unit
            int64_t dm = dl;
            const int64_t glast = std::min<int64_t>(16 * (u + 1), n_chunks) - 1;
            while (h_off[dm + 1] <= glast) ++dm;
            if (dm - dl > 32) L.wide_ok = L.wide_ok64 = 0;
        }
    }
    // ... and the kernel's retirement must keep up.  It retires at most two blocks of 32 documents per unit, and only blocks
    // that were complete before the unit, so where the documents under the units advance by more than 64 per unit for several
    // units in a row (sustained runs of chunk-less documents; the windows above allow up to 96) the first block not yet retired
    // falls further behind each unit, until a document being folded lies a whole ring ahead of it and shares a slot with a
    // document still waiting to be written.  Walk the kernel's own bookkeeping (next_b, next_end, flush_step in
    // msr_dense_ks.hip) over every span, O(n_docs + n_chunks / 16), and refuse such a corpus: it takes the narrow kernel.
    if (L.wide_ok || L.wide_ok64) {
        int64_t lag = 0;                                     // most documents between next_b and a document being folded
        for (size_t s = 0; s + 1 < L.spans.size(); ++s) {
            const int64_t d0 = L.spans[s], d1 = L.spans[s + 1];
            const int64_t c0 = h_off[d0], c1 = h_off[d1];
            if (c1 <= c0) continue;
            auto block_end = [&](int64_t b) -> int64_t { return h_off[std::min(b + 32, d1)]; };
            int64_t next_b = d0 & ~(int64_t)31;
            while (next_b < d1 && block_end(next_b) <= c0) next_b += 32;            // flush_done(c0)
            int64_t d = d0;                                  // document of the unit's last row
            for (int64_t g = c0 >> 4; g < (c1 + 15) >> 4; ++g) {
                const int64_t last = std::min(16 * g + 16, c1) - 1;
                while (h_off[d + 1] <= last) ++d;
                lag = std::max(lag, d - next_b);
                for (int i = 0; i < 2 && next_b < d1 && block_end(next_b) <= 16 * g; ++i) next_b += 32;   // flush_step(16 g)
            }
        }
        if (lag >= MSR_WIDE_RING) L.wide_ok = 0;
        if (lag >= 64) L.wide_ok64 = 0;
    }
    // row tiles for the GEMM paths: <= 256 rows, cut at document boundaries
    int32_t start = 0;
    L.tiles.push_back(0);
    for (int64_t d = 0; d < n_docs && L.tiles_ok; ++d) {
        const int32_t end = h_off[d + 1];
        if (end - h_off[d] > 256) L.tiles_ok = false;
        if (end - start > 256) { L.tiles.push_back(h_off[d]); start = h_off[d]; }
    }
    if (!L.tiles_ok) return MSR_OK;
    if (L.tiles.back() != (int32_t)n_chunks) L.tiles.push_back((int32_t)n_chunks);
    const size_t n_tiles = L.tiles.size() - 1;
    L.trow.resize(n_tiles);
    for (size_t t = 0; t < n_tiles; ++t) {                   // every tile starts at a multiple of 16 rows
        L.trow[t] = (int32_t)L.n_trows;
        L.n_trows += (L.tiles[t + 1] - L.tiles[t] + 15) / 16 * 16;
    }
    if (L.n_trows + MSR_STREAM256_TILE_ROWS >= ((int64_t)1 << 31)) { L.trow.clear(); L.n_trows = 0; }
    return MSR_OK;
}

// The device tables of the binding: e->dense, and the tile tables of the GEMM paths.
static int bind_chunk_tables(msr_engine* e, const float* emb, int64_t n_chunks, const int32_t* doc_off, int64_t n_docs,
                             const float* inv_norm, const ChunkLayout& L, hipStream_t st) {
    ALLOC(e, e->mem_chunks, e->chunk_doc, (size_t)n_chunks * sizeof(int32_t));
    ALLOC(e, e->mem_chunks, e->span_doc, L.spans.size() * sizeof(int32_t));
    ALLOC(e, e->mem_chunks, e->wspan_doc, L.wspans.size() * sizeof(int32_t));
    HIP_TRY(e, hipMemcpyAsync(e->span_doc, L.spans.data(), L.spans.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(e, hipMemcpyAsync(e->wspan_doc, L.wspans.data(), L.wspans.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(e, msr_fill_chunk_doc(doc_off, n_docs, e->chunk_doc, st));
    if (!inv_norm) {
        ALLOC(e, e->mem_chunks, e->inv_norm_own, (size_t)n_chunks * sizeof(float));
        HIP_TRY(e, msr_row_inv_norm(emb, n_chunks, e->inv_norm_own, st));
        inv_norm = e->inv_norm_own;
    }
    if (L.wide_ok) {
        ALLOC(e, e->mem_chunks, e->row_meta, (size_t)(n_chunks + 16) * 8);
        HIP_TRY(e, msr_pack_row_meta(e->chunk_doc, inv_norm, n_chunks, e->row_meta, st));
    }
    // The default scan multiplies f16-split pieces (error bound in msr_dense.hip); the bound needs row norms near 1
    // (the reference stores unit-norm rows, indexer/indexer.py:165).  Otherwise fall back to the exact f32 MFMA kernel.
    int variant = e->cfg.scan_variant;
    if (variant == MSR_SCAN_AUTO) {
        uint32_t h_rng[2] = {0, 0};
        HIP_TRY(e, msr_inv_norm_range(inv_norm, n_chunks, (uint32_t*)e->sel.cand_n, st));   // 2 scratch words
        HIP_TRY(e, hipMemcpyAsync(h_rng, e->sel.cand_n, sizeof(h_rng), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipMemsetAsync(e->sel.cand_n, 0, 2 * sizeof(int32_t), st));
        HIP_TRY(e, hipStreamSynchronize(st));
        float lo, hi;
        memcpy(&lo, &h_rng[0], 4); memcpy(&hi, &h_rng[1], 4);
        variant = (lo >= 0.5f && hi <= 2.0f) ? MSR_SCAN_F16X2 : MSR_SCAN_EXACT;
        if (variant == MSR_SCAN_F16X2 && e->cfg.scan_layout == 0 && L.wide_ok) variant = MSR_SCAN_KSPLIT;   // up to 64 queries per sweep
    }
    if (variant == MSR_SCAN_PRESPLIT) {                   // A/B variant: K-split scan over a pre-split copy of the rows
        if (e->cfg.scan_layout != 0 || !L.wide_ok) {
            variant = MSR_SCAN_F16X2;                     // preconditions of the K-split kernel not met
        } else {
            ALLOC(e, e->mem_chunks, e->emb_presplit, (size_t)n_chunks * MSR_DIM * sizeof(float));
            HIP_TRY(e, msr_presplit_rows(emb, n_chunks, e->emb_presplit, st));
        }
    }
    DenseIndex d{};                                       // (emb_bf16: msr_enable_bf16; gate, gate_per64: per launch)
    d.emb = emb; d.doc_off = doc_off; d.chunk_doc = e->chunk_doc; d.inv_norm = inv_norm;
    d.n_chunks = n_chunks; d.n_docs = n_docs; d.score_stride = (n_docs + 31) / 32 * 32;
    d.span_doc = e->span_doc; d.n_spans = (int)L.spans.size() - 1;
    d.wspan_doc = e->wspan_doc; d.n_wspans = (int)L.wspans.size() - 1;
    d.layout = e->cfg.scan_layout; d.variant = variant;
    d.qimg = e->qimg; d.emb_presplit = e->emb_presplit; d.row_meta = e->row_meta;
    d.wide_ok = L.wide_ok; d.wide_ok64 = L.wide_ok && L.wide_ok64;
    e->dense = d;
    if (L.tiles_ok) {
        ALLOC(e, e->mem_chunks, e->tile_row, L.tiles.size() * 4);
        HIP_TRY(e, hipMemcpyAsync(e->tile_row, L.tiles.data(), L.tiles.size() * 4, hipMemcpyHostToDevice, st));
        e->n_tiles = (int)L.tiles.size() - 1;
        e->tiles_ok = true;
    }
    if (!L.trow.empty()) {
        ALLOC(e, e->mem_chunks, e->tile_trow, L.trow.size() * 4);
        HIP_TRY(e, hipMemcpyAsync(e->tile_trow, L.trow.data(), L.trow.size() * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(e, hipStreamSynchronize(st));                 // (the copies out of L's vectors have been made)
    return MSR_OK;
}

// Batches of 65..128 queries take ONE streaming pass over the f32 rows (f16 filter + exact f32 finish, msr_gemm_f32.hip) when the
// corpus allows it: the pass' scratch, the two optional copies of the rows, e->gf.
static int bind_stream_pass(msr_engine* e, const ChunkLayout& L, hipStream_t st) {
    if (!dense_stream_bindable(dense_binding(e->dense), e->tiles_ok, e->n_tiles)) return MSR_OK;
    const float* emb = e->dense.emb;
    const float* inv_norm = e->dense.inv_norm;
    const int64_t n_chunks = e->dense.n_chunks;
    const int n_tiles = e->n_tiles, nw = e->n_cus * 8, stride = (n_tiles + 31) / 32 * 32;
    const StreamCaps caps = stream_caps(e->cfg.max_queries);         // (msr_stream_plan.h)
    const size_t QM = (size_t)caps.groups * 128;
    GemmF32Index& g = e->gf;
    g.n_tiles = n_tiles; g.n_cus = e->n_cus; g.caps = caps; g.tmax_stride = stride;
    g.single_emit = (e->cfg.flags & MSR_CFG_SINGLE_EMIT) ? 1 : 0;
    ALLOC(e, e->mem_chunks, e->gf_inv_pad, (size_t)(n_chunks + 512) * 4);
    ALLOC(e, e->mem_chunks, g.qimg, (size_t)caps.groups * 24 * 8192);
    ALLOC(e, e->mem_chunks, e->gf_qn, (QM + 64) * MSR_DIM * 4);
    ALLOC(e, e->mem_chunks, e->gf_fb_qimg, dense_fallback_slices((int)QM) * msr_ksplit_slice_image_bytes());
    ALLOC(e, e->mem_chunks, g.tmax_t, (size_t)n_tiles * 8 * caps.tmax_row * 4);    // [tile][wave][queries of a launch]
    ALLOC(e, e->mem_chunks, g.tmax, QM * stride * 4);
    ALLOC(e, e->mem_chunks, g.thr, QM * 4);
    ALLOC(e, e->mem_chunks, g.thr2, QM * 4);
    ALLOC(e, e->mem_chunks, g.flag, QM * 4);
    ALLOC(e, e->mem_chunks, g.wvbuf, (size_t)nw * caps.wv_cap * 16);
    ALLOC(e, e->mem_chunks, g.wv_count, (size_t)nw * 4);
    ALLOC(e, e->mem_chunks, g.pairs, QM * 4096 * 8);
    ALLOC(e, e->mem_chunks, g.pair_n, QM * 4);
    ALLOC(e, e->mem_chunks, e->gf_gate, GF_GATE_BYTES);
    ALLOC(e, e->mem_chunks, g.err_max, 4);
    ALLOC(e, e->mem_chunks, g.margin, QM * 4);
    ALLOC(e, e->mem_chunks, g.cand_doc, QM * MSR_SEL_CAP * 4);
    ALLOC(e, e->mem_chunks, g.cand_score, QM * MSR_SEL_CAP * 4);
    ALLOC(e, e->mem_chunks, g.cand_chunk, QM * MSR_SEL_CAP * 4);
    ALLOC(e, e->mem_chunks, g.cand_n, QM * 4);
    g.tile_row = e->tile_row;
    g.inv_pad = e->gf_inv_pad;
    HIP_TRY(e, msr_pad_inv_norm(inv_norm, n_chunks, n_chunks + 512, e->gf_inv_pad, st));
    HIP_TRY(e, hipMemsetAsync(g.pair_n, 0, QM * 4, st));
    HIP_TRY(e, hipMemsetAsync(e->gf_gate, 0, GF_GATE_BYTES, st));
    HIP_TRY(e, hipMemsetAsync(g.cand_n, 0, QM * 4, st));
    HIP_TRY(e, msr_f16_row_error(emb, inv_norm, n_chunks, g.err_max, st));   // measured once: the margin of the f16 filter
    // The 256-query kernel streams a copy of the rows in fragment order (whole cache lines per load instruction; +3 % rows
    // of padding: every tile starts at a multiple of 16 rows).  Size of the copy: a workgroup's tile visit ALWAYS loads
    // MSR_STREAM256_TILE_ROWS = 8 waves x 32 rows from the tile's first row on, whatever the tile's own length (rows behind
    // the tile are masked in the epilogue); all K blocks of a visit, and the prefetch of the next visit's first block,
    // address rows of [first row of a tile, first row + MSR_STREAM256_TILE_ROWS) -- the "next" tile of a workgroup's last
    // visit is that same tile again (jn == jt).  So the highest row the kernel touches is max_t tile_trow[t] +
    // MSR_STREAM256_TILE_ROWS - 1 < n_trows + MSR_STREAM256_TILE_ROWS: that many rows of zero padding behind the last
    // tile are exactly enough, for every prefetch depth (checked against the tile table here, not assumed).
    // The row-major matrix stays what every other kernel reads.  Declined by MSR_CFG_NO_ROW_COPY, or when the allocation
    // fails (the copy doubles the matrix): the TILED = false instantiation of the same kernel reads the caller's matrix.
    if (caps.want_copy && e->tile_trow) {
        const size_t copy_rows = (size_t)L.n_trows + MSR_STREAM256_TILE_ROWS;
        if ((int64_t)L.trow.back() + MSR_STREAM256_TILE_ROWS > (int64_t)copy_rows)
            return fail(e, MSR_ERR_INVALID, "msr_bind_chunks: internal: tile table exceeds the fragment-order copy");
        if (e->cfg.flags & MSR_CFG_NO_ROW_COPY) {
            e->row_copy_state = 2;
        } else if (e->mem_chunks.alloc(&e->gf_emb_tiled, copy_rows * MSR_DIM * 4) != hipSuccess) {
            (void)hipGetLastError();                      // clear the sticky error: the engine works without the copy
            e->row_copy_state = 3;
        } else {
            HIP_TRY(e, hipMemsetAsync((char*)e->gf_emb_tiled + (size_t)L.n_trows * MSR_DIM * 4, 0,
                                      (size_t)MSR_STREAM256_TILE_ROWS * MSR_DIM * 4, st));
            HIP_TRY(e, msr_tile_rows(emb, e->tile_row, e->tile_trow, n_tiles, e->gf_emb_tiled, st));
            e->row_copy_state = 1;
        }
    }
    // Launches of SEVERAL 256-query groups (engines for >= 512 queries per call: the batched steps, a rank of a sharded
    // run) are bound by the matrix pipes and the vector issue beside them; every group converts the same f32 rows to f16
    // again.  They read an f16 image of the rows instead -- the very values the pass converts in registers (round to
    // nearest, not normalised): same products, same candidates, same results; 1536 B per row.  Declined with the other
    // copy (MSR_CFG_NO_ROW_COPY) or when the allocation fails: those launches then convert as before.
    if (caps.want_image && (e->cfg.flags & MSR_CFG_NO_ROW_COPY)) {
        e->row_image_state = 2;
    } else if (caps.want_image) {
        const size_t img_rows = (size_t)n_chunks + 512;
        if (e->mem_chunks.alloc(&e->gf_emb_f16, img_rows * MSR_DIM * 2) != hipSuccess) {
            (void)hipGetLastError();
            e->row_image_state = 3;
        } else {
            HIP_TRY(e, msr_f16_rows(emb, n_chunks, (int64_t)img_rows, e->gf_emb_f16, st));
            e->row_image_state = 1;
        }
    }
    g.emb_tiled = e->gf_emb_tiled;
    g.tile_trow = e->gf_emb_tiled ? e->tile_trow : nullptr;
    g.emb_f16 = e->gf_emb_f16;
    e->gf_ok = true;
    return MSR_OK;
}

extern "C" int msr_bind_chunks(msr_engine* e, const float* emb, int64_t n_chunks, const int32_t* doc_off,
                               int64_t n_docs, const float* inv_norm, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!emb || !doc_off || n_chunks <= 0 || n_chunks >= (1ll << 31) || n_docs <= 0 || n_docs >= (1ll << 31))
        return fail(e, MSR_ERR_INVALID, "msr_bind_chunks: bad argument");
    if (e->have_postings && e->bm25.n_docs != n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_chunks: n_docs %lld differs from bound postings (%lld)",
                    (long long)n_docs, (long long)e->bm25.n_docs);
    if (e->cfg.scan_layout == 1 && !inv_norm)
        return fail(e, MSR_ERR_INVALID, "msr_bind_chunks: inv_norm is required with the interleaved layout");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // spans need the document offsets on the host (one-time, at bind)
    std::vector<int32_t> h_off((size_t)n_docs + 1);
    HIP_TRY(e, hipMemcpyAsync(h_off.data(), doc_off, (size_t)(n_docs + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    ChunkLayout L;
    int rc = chunk_layout(e, e->n_cus, h_off, n_chunks, n_docs, L);
    if (rc) return rc;                                       // (a malformed doc_off: the previous binding keeps serving)
    // from here on the previous binding is being replaced -- its tables, the bf16 image, a pending msr_dense_topk_begin: the
    // engine counts as unbound until this call succeeds
    drop_chunks(e);
    rc = ensure_score_rows(e, n_docs);
    if (!rc) rc = bind_chunk_tables(e, emb, n_chunks, doc_off, n_docs, inv_norm, L, st);
    if (!rc) rc = bind_stream_pass(e, L, st);
    if (rc) drop_chunks(e);                                  // (nothing half-built stays behind)
    e->have_chunks = rc == MSR_OK;
    return rc;
}

extern "C" int msr_debug_chunk_layout(const int32_t* doc_off, int64_t n_docs, int32_t out[4]) {
    if (!doc_off || !out || n_docs < 0 || n_docs >= ((int64_t)1 << 31))
        return fail(nullptr, MSR_ERR_INVALID, "msr_debug_chunk_layout: bad argument");
    const int n_cus = out[3] > 0 ? out[3] : 256;
    const std::vector<int32_t> h_off(doc_off, doc_off + n_docs + 1);
    ChunkLayout L;
    const int rc = chunk_layout(nullptr, n_cus, h_off, h_off[n_docs], n_docs, L);
    if (rc) return rc;
    out[0] = L.wide_ok; out[1] = L.wide_ok && L.wide_ok64; out[2] = L.tiles_ok; out[3] = (int32_t)L.spans.size() - 1;
    return MSR_OK;
}

extern "C" int msr_unbind(msr_engine* e) {
    if (!e) return MSR_ERR_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    drop_postings(e);
    drop_chunks(e);
    e->url_group = nullptr; e->url_group_n = 0;
    e->doc_domain = nullptr; e->doc_domain_n = 0;
    e->last_dense_width = 0;
    e->last_dense_segments = 0;
    // scratch sized by the corpus (the per-query scratch of msr_create stays)
    e->mem_corpus.release();
    e->score_rows_bytes = e->bm_cand_bytes = 0;
    return MSR_OK;
}

extern "C" int msr_bind_doc_meta(msr_engine* e, const int32_t* url_group, int64_t n_docs, void* stream) {
    (void)stream;
    if (!e) return MSR_ERR_INVALID;
    if (url_group && e->have_chunks && n_docs != e->dense.n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_doc_meta: n_docs mismatch");
    e->url_group = url_group;
    e->url_group_n = n_docs;
    return MSR_OK;
}

extern "C" int msr_bind_doc_domains(msr_engine* e, const int32_t* domain, int64_t n_docs, void* stream) {
    (void)stream;
    if (!e) return MSR_ERR_INVALID;
    if (n_docs < 0 || (domain && n_docs == 0)) return fail(e, MSR_ERR_INVALID, "msr_bind_doc_domains: bad argument");
    e->doc_domain = domain;
    e->doc_domain_n = domain ? n_docs : 0;
    return MSR_OK;
}

extern "C" int msr_diversify(msr_engine* e, int32_t n_queries, const int32_t* fused_doc, const double* fused_score,
                             const double* fused_orig, const int32_t* fused_chunk, const int32_t* fused_n, int32_t max_cand,
                             int32_t top_k, double relevance_threshold, int32_t diversify, int32_t* out_doc, double* out_score,
                             double* out_orig, int32_t* out_chunk, int32_t* out_n, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!fused_doc || !fused_score || !fused_orig || !fused_chunk || !fused_n || !out_doc || !out_score || !out_orig || !out_chunk ||
        !out_n)
        return fail(e, MSR_ERR_INVALID, "msr_diversify: null argument");
    if (n_queries < 0 || max_cand < 1 || max_cand > 1024 || top_k < 1)
        return fail(e, MSR_ERR_INVALID, "msr_diversify: bad argument (max_cand=%d, top_k=%d)", max_cand, top_k);
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_diversify_run(n_queries, fused_doc, fused_score, fused_orig, fused_chunk, fused_n, max_cand, e->doc_domain,
                                 e->doc_domain_n, top_k, relevance_threshold, diversify, out_doc, out_score, out_orig, out_chunk,
                                 out_n, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_interleave_rows(msr_engine* e, const float* src, int64_t n_rows, float* dst, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!src || !dst || n_rows <= 0 || src == dst) return fail(e, MSR_ERR_INVALID, "msr_interleave_rows: bad argument");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_interleave(src, n_rows, dst, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_scan_arith(const msr_engine* e) {
    if (!e || !e->have_chunks) return -1;
    return dense_variant_f16x2(e->dense.variant) ? 1 : 0;
}

extern "C" int msr_scan_width(const msr_engine* e) {
    if (!e || !e->have_chunks) return -1;
    const DenseBinding b = dense_binding(e->dense);
    // streaming pass over the f32 rows for batches of more than 64 queries: 128 queries per pass, 256 for batches of more
    // than 128 (when the engine was created for that many queries per call)
    if (dense_stream_bound(b, e->gf_ok)) return e->gf.caps.width;
    return dense_slice(b, 0);
}

extern "C" int msr_dense_path(const msr_engine* e) { return e ? e->last_dense_width : -1; }

// Diagnostic (never on the hot path): waits for the device and reads the per-wave emission counters of the last streaming call.
extern "C" int msr_dense_pass_info(msr_engine* e, int32_t* segments, int64_t* entries) {
    if (!e) return MSR_ERR_INVALID;
    if (!segments || !entries) return fail(e, MSR_ERR_INVALID, "msr_dense_pass_info: null argument");
    *segments = e->last_dense_segments;
    *entries = 0;
    if (!e->have_chunks || !e->gf_ok || e->last_dense_segments == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipDeviceSynchronize());
    std::vector<int32_t> cnt((size_t)e->gf.n_cus * 8);
    HIP_TRY(e, hipMemcpy(cnt.data(), e->gf.wv_count, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t sum = 0;
    for (int32_t c : cnt) sum += c;
    *entries = sum;
    return MSR_OK;
}

extern "C" int64_t msr_owned_bytes(const msr_engine* e) {
    if (!e) return -1;
    return (int64_t)(e->mem_engine.bytes() + e->mem_corpus.bytes() + e->mem_postings.bytes() + e->mem_chunks.bytes() +
                     e->mem_bf16.bytes());
}

extern "C" int msr_row_copy_state(const msr_engine* e) { return e ? e->row_copy_state : -1; }
extern "C" int msr_row_image_state(const msr_engine* e) { return e ? e->row_image_state : -1; }

extern "C" int msr_batch_width(const msr_engine* e) {
    if (!e || !e->have_chunks || !e->emb_bf16) return -1;
    return dense_bf16_slice(dense_binding(e->dense), 0);
}

extern "C" int msr_set_timing(msr_engine* e, int32_t enabled) {
    if (!e) return MSR_ERR_INVALID;
    e->timing = enabled != 0;
    for (int w = 0; w < msr_engine::EV_KINDS; ++w) e->ev_count[w] = 0;
    return MSR_OK;
}

extern "C" int msr_kernel_time_ms(msr_engine* e, int32_t which, float* out_ms, int32_t* out_launches) {
    if (!e || which < 0 || which >= msr_engine::EV_KINDS || !out_ms) return e ? fail(e, MSR_ERR_INVALID, "msr_kernel_time_ms: bad argument") : MSR_ERR_INVALID;
    const int n = std::min(e->ev_count[which], (int)msr_engine::EV_RING);
    if (n <= 0) return fail(e, MSR_ERR_INVALID, "msr_kernel_time_ms: no timed launch recorded");
    float total = 0.f;
    for (int j = 0; j < n; ++j) {
        float ms = 0.f;
        HIP_TRY(e, hipEventSynchronize(e->ev_stop[which][j]));
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_start[which][j], e->ev_stop[which][j]));
        total += ms;
    }
    *out_ms = total;
    if (out_launches) *out_launches = n;
    return MSR_OK;
}

// Document sets of a *_within call: refused as the header says, before anything is launched (outputs untouched).
static int within_args_ok(msr_engine* e, const char* fn, int64_t n_docs, const uint32_t* set_bits, int32_t n_sets,
                          int64_t set_stride, const int32_t* q_set) {
    if (n_sets < 0) return fail(e, MSR_ERR_INVALID, "%s: bad argument (n_sets=%d)", fn, n_sets);
    if (n_sets == 0) return MSR_OK;
    if (!set_bits || !q_set) return fail(e, MSR_ERR_INVALID, "%s: bad argument (set_bits or q_set is NULL with n_sets=%d)", fn, n_sets);
    if (set_stride < (n_docs + 31) / 32)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (set_stride=%lld < ceil(n_docs / 32) = %lld)", fn, (long long)set_stride,
                    (long long)((n_docs + 31) / 32));
    return MSR_OK;
}

// What every dense top-k entry point refuses first, in this order: nothing bound (need_bf16: no bf16 image either), an open
// msr_dense_topk_begin (they share the score rows and the select scratch), and -- args_ok false -- its arguments, which the
// three calls over plain query rows test alike (dense_topk_args).
static bool dense_topk_args(const msr_engine* e, int32_t n_queries, int32_t k, int32_t max_chunks_per_doc, const float* q,
                            const int32_t* out_doc, const float* out_score, const int32_t* out_n) {
    return n_queries >= 0 && k >= 1 && k <= e->cfg.max_k && max_chunks_per_doc >= 0 && q && out_doc && out_score && out_n;
}
static int dense_entry_ok(msr_engine* e, const char* fn, bool need_bf16, bool args_ok, int32_t k) {
    if (need_bf16 && (!e->have_chunks || !e->emb_bf16)) return fail(e, MSR_ERR_NOT_BOUND, "%s: call msr_enable_bf16 first", fn);
    if (!e->have_chunks) return fail(e, MSR_ERR_NOT_BOUND, "%s: chunks not bound", fn);
    if (e->split_pending)
        return fail(e, MSR_ERR_INVALID, "%s: an msr_dense_topk_begin is pending (its scratch is in use): call msr_dense_topk_end first", fn);
    if (!args_ok) return fail(e, MSR_ERR_INVALID, "%s: bad argument (k=%d, max_k=%d)", fn, k, e->cfg.max_k);
    return MSR_OK;
}

static int bm25_topk_impl(msr_engine* e, const char* fn, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                          int32_t n_queries, int32_t k, double min_score, int32_t* out_doc, double* out_score, int32_t* out_n,
                          void* stream, const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* q_set) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "%s: postings not bound", fn);
    if (n_queries < 0 || k < 1 || k > e->cfg.max_k || !q_term_off || !out_doc || !out_score || !out_n)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (k=%d, max_k=%d)", fn, k, e->cfg.max_k);
    {
        const int rc = within_args_ok(e, fn, e->bm25.n_docs, set_bits, n_sets, set_stride, q_set);
        if (rc) return rc;
    }
    if (n_queries == 0) return MSR_OK;
    // n_sets > 0: the restricted scoring kernel (q_set indexed by the call's query number); the select is the same
    const MsrSetView set_view{set_bits, set_stride, q_set, n_sets};
    const MsrSetView* set = n_sets > 0 ? &set_view : nullptr;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const int slice = e->cfg.max_queries;
    const int64_t N = e->bm25.n_docs;
    for (int q0 = 0; q0 < n_queries; q0 += slice) {
        const int nq = std::min(slice, n_queries - q0);
        int32_t* o_doc = out_doc + (int64_t)q0 * k;
        double* o_score = out_score + (int64_t)q0 * k;
        // every launch gets its own event pair (ring of EV_RING; later launches are not recorded)
        const bool timed = e->timing && e->ev_count[1] < msr_engine::EV_RING;
        int n_seg = 0;
        int64_t seg_stride = 0;
        if (timed) HIP_TRY(e, hipEventRecord(e->ev_start[1][e->ev_count[1]], st));
        // (the plan kernel in front of the scoring kernel -- item order and window anchors -- runs inside the timing pair)
        HIP_TRY(e, msr_bm25_scores(e->bm25, q_term_off, q_terms, q_qtf, q0, nq, min_score, (double*)e->score_rows, e->bm_cand_doc,
                                   e->bm_cand_n, &n_seg, &seg_stride, e->bm_win, e->bm_order, st, set));
        if (timed) {
            HIP_TRY(e, hipEventRecord(e->ev_stop[1][e->ev_count[1]], st));
            e->ev_count[1]++;
        }
        // scores >= min_score >= 0 lie in a window of 16 octaves below a bound known from the query alone: one histogram
        // pass instead of two (a negative min_score keeps the general two)
        const uint64_t* win = min_score >= 0.0 ? e->bm_win : nullptr;
        HIP_TRY(e, msr_select_topk_list((const double*)e->score_rows, e->bm_cand_doc, e->bm_cand_n, n_seg, seg_stride, N, nq, k,
                                        e->sel, o_doc, o_score, out_n + q0, st, win));
    }
    return MSR_OK;
}

extern "C" int msr_bm25_topk(msr_engine* e, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                             int32_t n_queries, int32_t k, double min_score, int32_t* out_doc, double* out_score,
                             int32_t* out_n, void* stream) {
    return bm25_topk_impl(e, "msr_bm25_topk", q_term_off, q_terms, q_qtf, n_queries, k, min_score, out_doc, out_score, out_n,
                          stream, nullptr, 0, 0, nullptr);
}

extern "C" int msr_bm25_topk_within(msr_engine* e, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                                    int32_t n_queries, int32_t k, double min_score, const uint32_t* set_bits, int32_t n_sets,
                                    int64_t set_stride, const int32_t* q_set, int32_t* out_doc, double* out_score,
                                    int32_t* out_n, void* stream) {
    return bm25_topk_impl(e, "msr_bm25_topk_within", q_term_off, q_terms, q_qtf, n_queries, k, min_score, out_doc, out_score,
                          out_n, stream, set_bits, n_sets, set_stride, q_set);
}

// K12 - K14 read the forward index: refused until msr_bind_tokens has bound one to the bound postings.
static int tokens_bound(msr_engine* e, const char* fn) {
    if (e->have_postings && e->have_tokens) return MSR_OK;
    return fail(e, MSR_ERR_NOT_BOUND, "%s: tokens not bound (msr_bind_tokens: the index has no forward index)", fn);
}

// The refusals that the calls writing bitset rows share (K11 - K13, msr_combine_sets): n_rows rows out, described by arrays of
// the call's own (rows_ok: out_bits and they are non-NULL; rows_what names them), and n_in rows in -- base, candidate or input
// rows (in_ok: their pointers are non-NULL).  Checked as the header says, before anything is launched (outputs untouched).
static int set_rows_args_ok(msr_engine* e, const char* fn, int32_t n_rows, bool rows_ok, const char* rows_what, int64_t out_stride,
                            const char* n_in_name, int32_t n_in, bool in_ok, const char* in_what, const char* in_stride_name,
                            int64_t in_stride) {
    const int64_t W = (e->bm25.n_docs + 31) / 32;
    if (n_rows < 0 || n_in < 0) return fail(e, MSR_ERR_INVALID, "%s: bad argument (n_rows=%d, %s=%d)", fn, n_rows, n_in_name, n_in);
    if (n_rows > 0 && !rows_ok)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (%s is NULL with n_rows=%d)", fn, rows_what, n_rows);
    if (out_stride < W)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (out_stride=%lld < ceil(n_docs / 32) = %lld)", fn, (long long)out_stride,
                    (long long)W);
    if (n_in > 0 && !in_ok)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (%s is NULL with %s=%d)", fn, in_what, n_in_name, n_in);
    if (n_in > 0 && in_stride < W)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (%s=%lld < ceil(n_docs / 32) = %lld)", fn, in_stride_name,
                    (long long)in_stride, (long long)W);
    return MSR_OK;
}

extern "C" int msr_term_sets(msr_engine* e, int32_t n_rows, const int32_t* must_off, const int32_t* must_terms,
                             const int32_t* not_off, const int32_t* not_terms, const uint32_t* base_bits, int32_t n_base,
                             int64_t base_stride, const int32_t* row_base, uint32_t* out_bits, int64_t out_stride, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_term_sets: postings not bound");
    const int rc = set_rows_args_ok(e, "msr_term_sets", n_rows, out_bits && must_off && not_off, "out_bits, must_off or not_off",
                                    out_stride, "n_base", n_base, base_bits && row_base, "base_bits or row_base", "base_stride",
                                    base_stride);
    if (rc) return rc;
    if (n_rows == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_term_sets_run(e->bm25, n_rows, must_off, must_terms, not_off, not_terms, base_bits, n_base, base_stride,
                                 row_base, out_bits, out_stride, (hipStream_t)stream));
    return MSR_OK;
}

// ---- K19: match modes (msr_match.hip; include/msretr_match.h) ------------------------------------------------------------------
extern "C" int msr_match_sets(msr_engine* e, int32_t n_rows, const int32_t* row_group_off, const int32_t* group_term_off,
                              const int32_t* group_terms, const int32_t* row_need, const uint32_t* base_bits, int32_t n_base,
                              int64_t base_stride, const int32_t* row_base, uint32_t* out_bits, int64_t out_stride, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_match_sets: postings not bound");
    char why[192];
    const int rc = msr_match_args_check(e->bm25.n_docs, n_rows, out_bits && row_group_off && group_term_off && row_need, out_stride,
                                        n_base, base_bits && row_base, base_stride, why, sizeof why);
    if (rc) return fail(e, rc, "%s", why);
    if (n_rows == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_match_sets_run(e->bm25, n_rows, row_group_off, group_term_off, group_terms, row_need, base_bits, n_base,
                                  base_stride, row_base, out_bits, out_stride, (hipStream_t)stream));
    return MSR_OK;
}

// ---- K17: facet counts (msr_facet.hip) ----------------------------------------------------------------------------------------
extern "C" int msr_bind_facet(msr_engine* e, const uint16_t* local, const int32_t* span_off, const int32_t* span_values,
                              const int32_t* value_off, const int32_t* value_pos, int64_t n_docs, int32_t n_values, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_bind_facet: postings not bound");
    if (!local && !span_off && !span_values && !value_off && !value_pos) {       // all NULL: unbind
        drop_facet(e);
        return MSR_OK;
    }
    // a refused table leaves the previous binding as it is: nothing of the engine changes before the check has passed
    if (!span_off || !value_off || n_values < 0 || (n_docs > 0 && !local))
        return fail(e, MSR_ERR_INVALID, "msr_bind_facet: bad argument");
    if (n_docs != e->bm25.n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_facet: n_docs %lld differs from bound postings (%lld)", (long long)n_docs,
                    (long long)e->bm25.n_docs);
    if ((uintptr_t)local % 16)
        return fail(e, MSR_ERR_INVALID, "msr_bind_facet: local is not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (!e->sim_flag) ALLOC(e, e->mem_engine, e->sim_flag, 64);
    const int64_t n_spans = (n_docs + MSR_TERMSET_SPAN_DOCS - 1) / MSR_TERMSET_SPAN_DOCS;
    int32_t ends[2] = {0, 0};                                // T = span_off[n_spans] sizes span_values and value_pos
    HIP_TRY(e, hipMemcpyAsync(&ends[0], span_off + n_spans, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipMemcpyAsync(&ends[1], value_off + n_values, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (ends[0] < 0 || ends[0] > n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_facet: malformed table: span_off ends at %d, outside [0, n_docs]", ends[0]);
    if (ends[1] != ends[0])
        return fail(e, MSR_ERR_INVALID, "msr_bind_facet: malformed table: value_off[n_values] = %d, span_off[n_spans] = %d",
                    ends[1], ends[0]);
    if (ends[0] > 0 && (!span_values || !value_pos)) return fail(e, MSR_ERR_INVALID, "msr_bind_facet: bad argument");
    const FacetTable f{local, span_off, span_values, value_off, value_pos, n_values, ends[0]};
    // two kernels: the first reads the offsets and local[] by its own index only; the second follows the offsets and returns
    // at once unless the first found them sound, so a malformed table cannot send a read out of bounds
    int32_t flag = 0;
    HIP_TRY(e, hipMemsetAsync(e->sim_flag, 0, sizeof(int32_t), st));
    HIP_TRY(e, msr_facet_validate(f, n_docs, e->sim_flag, st));
    HIP_TRY(e, hipMemcpyAsync(&flag, e->sim_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (flag) {
        static const char* why[] = {"", "span_off does not start at 0, descends, or a span holds more entries than documents",
                                    "a local id at or past its span's entry count", "value_off does not start at 0 or descends",
                                    "span_values out of range or not strictly ascending within a span",
                                    "value_pos out of range, not strictly ascending within a value, or naming another value"};
        return fail(e, MSR_ERR_INVALID, "msr_bind_facet: malformed table: %s", why[std::min(std::max(flag, 0), 5)]);
    }
    e->facet = f;
    e->have_facet = true;
    return MSR_OK;
}

extern "C" int64_t msr_facet_scratch_bytes(const msr_engine* e, int32_t n_rows) {
    if (!e || n_rows < 0) return MSR_ERR_INVALID;
    if (!e->have_postings || !e->have_facet) return MSR_ERR_NOT_BOUND;
    return (int64_t)n_rows * msr_facet_row_bytes(e->facet, e->bm25.n_docs);
}

extern "C" int msr_facet_counts(msr_engine* e, int32_t n_rows, const int32_t* any_off, const int32_t* any_terms,
                                const uint32_t* base_bits, int32_t n_base, int64_t base_stride, const int32_t* row_base,
                                int32_t limit, int32_t* out_hits, int32_t* out_n_values_hit, int32_t* out_top_value,
                                int32_t* out_top_count, int32_t* out_counts, int64_t count_stride, void* scratch,
                                int64_t scratch_bytes, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_facet_counts: postings not bound");
    if (!e->have_facet) return fail(e, MSR_ERR_NOT_BOUND, "msr_facet_counts: facet table not bound (msr_bind_facet)");
    const int64_t W = (e->bm25.n_docs + 31) / 32;
    if (n_rows < 0 || n_base < 0)
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: bad argument (n_rows=%d, n_base=%d)", n_rows, n_base);
    if (limit < 0 || limit > MSR_FACET_MAX_LIMIT)
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: limit %d outside [0, MSR_FACET_MAX_LIMIT = %d]", limit, MSR_FACET_MAX_LIMIT);
    if (n_rows > 0 && (!any_off || !out_hits || !out_n_values_hit))
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: bad argument (any_off, out_hits or out_n_values_hit is NULL with n_rows=%d)",
                    n_rows);
    if (n_rows > 0 && limit > 0 && (!out_top_value || !out_top_count))
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: bad argument (out_top_value or out_top_count is NULL with limit=%d)", limit);
    if (out_counts && count_stride < e->facet.n_values)
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: bad argument (count_stride=%lld < n_values = %d)", (long long)count_stride,
                    e->facet.n_values);
    if (n_base > 0 && (!base_bits || !row_base))
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: bad argument (base_bits or row_base is NULL with n_base=%d)", n_base);
    if (n_base > 0 && base_stride < W)
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: bad argument (base_stride=%lld < ceil(n_docs / 32) = %lld)",
                    (long long)base_stride, (long long)W);
    const int64_t need = (int64_t)n_rows * msr_facet_row_bytes(e->facet, e->bm25.n_docs);
    if (scratch_bytes < need || (need > 0 && (!scratch || (uintptr_t)scratch % 16)))
        return fail(e, MSR_ERR_INVALID, "msr_facet_counts: scratch of %lld bytes, %lld needed (msr_facet_scratch_bytes; 16-byte aligned)",
                    (long long)scratch_bytes, (long long)need);
    if (n_rows == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_facet_counts_run(e->bm25, e->facet, n_rows, any_off, any_terms, base_bits, n_base, base_stride, row_base, limit,
                                    out_hits, out_n_values_hit, out_top_value, out_top_count, out_counts, count_stride, scratch,
                                    (hipStream_t)stream));
    return MSR_OK;
}

// ---- K18: near-duplicate collapse (msr_dedup.hip) -----------------------------------------------------------------------------
extern "C" int msr_doc_signatures(msr_engine* e, int64_t d0, int64_t d1, int32_t shingle, uint32_t* out_sig, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings || !e->have_tokens)
        return fail(e, MSR_ERR_NOT_BOUND, "msr_doc_signatures: tokens not bound (msr_bind_tokens: the index has no forward index)");
    if (d0 < 0 || d1 < d0 || d1 > e->bm25.n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_doc_signatures: bad range [%lld, %lld) of %lld documents", (long long)d0, (long long)d1,
                    (long long)e->bm25.n_docs);
    if (shingle < 1 || shingle > MSR_SIG_MAX_SHINGLE)
        return fail(e, MSR_ERR_INVALID, "msr_doc_signatures: shingle %d outside [1, MSR_SIG_MAX_SHINGLE = %d]", shingle,
                    MSR_SIG_MAX_SHINGLE);
    if (d1 > d0 && !out_sig) return fail(e, MSR_ERR_INVALID, "msr_doc_signatures: bad argument (out_sig is NULL)");
    if (d0 == d1) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_doc_signatures_run(e->tok_off, e->tok_ids, d0, d1, shingle, out_sig, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_bind_signatures(msr_engine* e, const uint32_t* sig, int64_t n_docs, void* stream) {
    (void)stream;
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_bind_signatures: postings not bound");
    if (!sig) {
        e->sig = nullptr; e->sig_n = 0;
        return MSR_OK;
    }
    if (n_docs != e->bm25.n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_signatures: n_docs %lld differs from bound postings (%lld)", (long long)n_docs,
                    (long long)e->bm25.n_docs);
    e->sig = sig;
    e->sig_n = n_docs;
    return MSR_OK;
}

extern "C" int64_t msr_collapse_scratch_bytes(int32_t n_queries, int32_t max_cand) {
    if (n_queries < 0 || max_cand < 1 || max_cand > MSR_COLLAPSE_MAX_CAND) return MSR_ERR_INVALID;
    return msr_collapse_bytes(n_queries, max_cand);
}

extern "C" int msr_collapse_duplicates(msr_engine* e, int32_t n_queries, const int32_t* fused_doc, const double* fused_score,
                                       const double* fused_orig, const int32_t* fused_chunk, const int32_t* fused_n,
                                       int32_t max_cand, int32_t min_matches, int32_t* out_doc, double* out_score,
                                       double* out_orig, int32_t* out_chunk, int32_t* out_n, int32_t* out_drop_doc,
                                       int32_t* out_drop_leader, int32_t* out_drop_matches, int32_t* out_drop_n, void* scratch,
                                       int64_t scratch_bytes, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->sig) return fail(e, MSR_ERR_NOT_BOUND, "msr_collapse_duplicates: signatures not bound (msr_bind_signatures)");
    if (min_matches < 1 || min_matches > MSR_SIG_WORDS)
        return fail(e, MSR_ERR_INVALID, "msr_collapse_duplicates: min_matches %d outside [1, MSR_SIG_WORDS = %d]", min_matches,
                    MSR_SIG_WORDS);
    if (max_cand < 1 || max_cand > MSR_COLLAPSE_MAX_CAND)
        return fail(e, MSR_ERR_INVALID, "msr_collapse_duplicates: max_cand %d outside [1, MSR_COLLAPSE_MAX_CAND = %d]", max_cand,
                    MSR_COLLAPSE_MAX_CAND);
    if (n_queries < 0) return fail(e, MSR_ERR_INVALID, "msr_collapse_duplicates: bad argument (n_queries=%d)", n_queries);
    if (n_queries > 0 && (!fused_doc || !fused_score || !fused_orig || !fused_chunk || !fused_n || !out_doc || !out_score ||
                          !out_orig || !out_chunk || !out_n || !out_drop_doc || !out_drop_leader || !out_drop_matches || !out_drop_n))
        return fail(e, MSR_ERR_INVALID, "msr_collapse_duplicates: null argument");
    const int64_t need = msr_collapse_bytes(n_queries, max_cand);
    if (scratch_bytes < need || (need > 0 && (!scratch || (uintptr_t)scratch % 16)))
        return fail(e, MSR_ERR_INVALID,
                    "msr_collapse_duplicates: scratch of %lld bytes, %lld needed (msr_collapse_scratch_bytes; 16-byte aligned)",
                    (long long)scratch_bytes, (long long)need);
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_collapse_run(e->sig, e->sig_n, e->doc_domain, e->doc_domain_n, n_queries, fused_doc, fused_score, fused_orig,
                                fused_chunk, fused_n, max_cand, min_matches, out_doc, out_score, out_orig, out_chunk, out_n,
                                out_drop_doc, out_drop_leader, out_drop_matches, out_drop_n, scratch, (hipStream_t)stream));
    return MSR_OK;
}

// ---- K12: phrase search (msr_phrase.hip) --------------------------------------------------------------------------------------
extern "C" int msr_bind_tokens(msr_engine* e, const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_tokens,
                               void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_bind_tokens: postings not bound");
    e->have_tokens = false; e->tok_off = nullptr; e->tok_ids = nullptr; e->n_tokens = 0;
    if (!tok_off || n_tokens < 0 || (n_tokens > 0 && !tok_ids)) return fail(e, MSR_ERR_INVALID, "msr_bind_tokens: bad argument");
    if (n_docs != e->bm25.n_docs)
        return fail(e, MSR_ERR_INVALID, "msr_bind_tokens: n_docs %lld differs from bound postings (%lld)", (long long)n_docs,
                    (long long)e->bm25.n_docs);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (!e->sim_flag) ALLOC(e, e->mem_engine, e->sim_flag, 64);
    // one kernel checks the offsets and the ids; it reads tok_off[0 .. n_docs] and tok_ids[0 .. n_tokens), which the caller
    // vouches for, and never follows an offset into tok_ids, so malformed offsets cannot send a read out of bounds
    int32_t flag = 0;
    HIP_TRY(e, hipMemsetAsync(e->sim_flag, 0, sizeof(int32_t), st));
    HIP_TRY(e, msr_tokens_validate(tok_off, tok_ids, n_docs, n_tokens, e->bm25.n_terms, e->sim_flag, st));
    HIP_TRY(e, hipMemcpyAsync(&flag, e->sim_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (flag) {
        static const char* why[] = {"", "tok_off does not run from 0 to n_tokens", "tok_off descends",
                                    "a token id is outside [0, n_terms)"};
        return fail(e, MSR_ERR_INVALID, "msr_bind_tokens: malformed forward index: %s", why[std::min(std::max(flag, 0), 3)]);
    }
    e->tok_off = tok_off; e->tok_ids = tok_ids; e->n_tokens = n_tokens;
    e->have_tokens = true;
    return MSR_OK;
}

extern "C" int msr_phrase_sets(msr_engine* e, int32_t n_rows, const int32_t* phrase_off, const int32_t* phrase_terms,
                               const uint32_t* cand_bits, int32_t n_cand, int64_t cand_stride, const int32_t* row_cand,
                               uint32_t* out_bits, int64_t out_stride, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    int rc = tokens_bound(e, "msr_phrase_sets");
    if (rc) return rc;
    rc = set_rows_args_ok(e, "msr_phrase_sets", n_rows, out_bits && phrase_off, "out_bits or phrase_off", out_stride, "n_cand", n_cand,
                          cand_bits && row_cand, "cand_bits or row_cand", "cand_stride", cand_stride);
    if (rc) return rc;
    if (n_rows == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_phrase_sets_run(e->tok_off, e->tok_ids, e->bm25.n_docs, e->bm25.n_terms, n_rows, phrase_off, phrase_terms,
                                   cand_bits, n_cand, cand_stride, row_cand, out_bits, out_stride, (hipStream_t)stream));
    return MSR_OK;
}

// ---- K13: proximity search (msr_proximity.hip) ----------------------------------------------------------------------------------
extern "C" int msr_proximity_sets(msr_engine* e, int32_t n_rows, const int32_t* phrase_off, const int32_t* phrase_terms,
                                  const int32_t* row_span, const int32_t* row_ordered, const uint32_t* cand_bits, int32_t n_cand,
                                  int64_t cand_stride, const int32_t* row_cand, uint32_t* out_bits, int64_t out_stride,
                                  void* stream) {
    if (!e) return MSR_ERR_INVALID;
    int rc = tokens_bound(e, "msr_proximity_sets");
    if (rc) return rc;
    rc = set_rows_args_ok(e, "msr_proximity_sets", n_rows, out_bits && phrase_off && row_span && row_ordered,
                          "out_bits, phrase_off, row_span or row_ordered", out_stride, "n_cand", n_cand, cand_bits && row_cand,
                          "cand_bits or row_cand", "cand_stride", cand_stride);
    if (rc) return rc;
    if (n_rows == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_proximity_sets_run(e->tok_off, e->tok_ids, e->bm25.n_docs, e->bm25.n_terms, n_rows, phrase_off, phrase_terms,
                                      row_span, row_ordered, cand_bits, n_cand, cand_stride, row_cand, out_bits, out_stride,
                                      (hipStream_t)stream));
    return MSR_OK;
}

// ---- K14: query-biased snippets (msr_snippet.hip) -------------------------------------------------------------------------------
extern "C" int msr_best_windows(msr_engine* e, int32_t n_pairs, const int32_t* pair_doc, const int32_t* pair_row, int32_t n_rows,
                                const int32_t* row_off, const int32_t* row_terms, const int32_t* row_weights,
                                const int32_t* row_span, int32_t* out_start, int32_t* out_cover, int32_t* out_hits,
                                uint64_t* out_mask, uint32_t* out_terms, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    const int rc = tokens_bound(e, "msr_best_windows");
    if (rc) return rc;
    if (n_pairs < 0 || n_rows < 0)
        return fail(e, MSR_ERR_INVALID, "msr_best_windows: bad argument (n_pairs=%d, n_rows=%d)", n_pairs, n_rows);
    if (n_pairs == 0) return MSR_OK;
    if (n_rows == 0) return fail(e, MSR_ERR_INVALID, "msr_best_windows: bad argument (n_rows=0 with n_pairs=%d)", n_pairs);
    if (!pair_doc || !pair_row || !row_off || !row_terms || !row_weights || !row_span)
        return fail(e, MSR_ERR_INVALID, "msr_best_windows: bad argument (pair_doc, pair_row, row_off, row_terms, row_weights or "
                    "row_span is NULL with n_pairs=%d)", n_pairs);
    if (!out_start || !out_cover || !out_hits || !out_mask || !out_terms)
        return fail(e, MSR_ERR_INVALID, "msr_best_windows: bad argument (an output pointer is NULL with n_pairs=%d)", n_pairs);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_best_windows_run(e->tok_off, e->tok_ids, e->bm25.n_docs, e->bm25.n_terms, n_pairs, pair_doc, pair_row, n_rows,
                                    row_off, row_terms, row_weights, row_span, out_start, out_cover, out_hits, out_mask, out_terms,
                                    (hipStream_t)stream));
    return MSR_OK;
}

// ---- K15: typo-tolerant lookup (msr_fuzzy.hip) ---------------------------------------------------------------------------------
extern "C" int msr_bind_vocab(msr_engine* e, const int64_t* char_off, const uint16_t* chars, const uint32_t* weight,
                              int64_t n_terms, int64_t n_chars, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_bind_vocab: postings not bound");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    drop_vocab(e);
    if (!char_off || !weight || n_chars < 0 || (n_chars > 0 && !chars)) return fail(e, MSR_ERR_INVALID, "msr_bind_vocab: bad argument");
    if (n_terms != e->bm25.n_terms)
        return fail(e, MSR_ERR_INVALID, "msr_bind_vocab: n_terms %lld differs from bound postings (%lld)", (long long)n_terms,
                    (long long)e->bm25.n_terms);
    hipStream_t st = (hipStream_t)stream;
    if (!e->sim_flag) ALLOC(e, e->mem_engine, e->sim_flag, 64);
    // one kernel checks the offsets and the weights; it reads char_off[0 .. n_terms] and weight[0 .. n_terms), which the
    // caller vouches for, and never follows an offset; the signatures are built from offsets that have passed
    int32_t flag = 0;
    HIP_TRY(e, hipMemsetAsync(e->sim_flag, 0, sizeof(int32_t), st));
    HIP_TRY(e, msr_vocab_validate(char_off, weight, n_terms, n_chars, e->sim_flag, st));
    HIP_TRY(e, hipMemcpyAsync(&flag, e->sim_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (flag) {
        static const char* why[] = {"", "char_off does not run from 0 to n_chars", "char_off descends",
                                    "a weight is 2^31 or more"};
        return fail(e, MSR_ERR_INVALID, "msr_bind_vocab: malformed vocabulary: %s", why[std::min(std::max(flag, 0), 3)]);
    }
    ALLOC(e, e->mem_postings, e->voc_sig, (size_t)std::max<int64_t>(n_terms, 1) * sizeof(uint64_t));
    hipError_t err = msr_vocab_signatures(char_off, chars, n_terms, e->voc_sig, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) {
        e->mem_postings.free_one(&e->voc_sig);
        return fail(e, MSR_ERR_HIP, "msr_bind_vocab: %s", hipGetErrorString(err));
    }
    e->voc_char_off = char_off; e->voc_chars = chars; e->voc_weight = weight; e->voc_n_chars = n_chars;
    e->have_vocab = true;
    return MSR_OK;
}

extern "C" int64_t msr_fuzzy_scratch_bytes(int64_t n_terms, int32_t n_words, int32_t limit) {
    if (n_terms < 0 || n_terms >= (1ll << 31) || n_words < 0 || n_words > MSR_FUZZY_MAX_WORDS || limit < 1 ||
        limit > MSR_FUZZY_MAX_LIMIT)
        return -1;
    return (int64_t)n_words * msr_fuzzy_spans(n_terms) * ((int64_t)limit * 8 + 4);
}

extern "C" int msr_fuzzy_terms(msr_engine* e, int32_t n_words, const int32_t* word_off, const uint16_t* word_chars,
                               const int32_t* word_max, int32_t limit, int32_t* out_term, int32_t* out_dist, int32_t* out_n,
                               int32_t* out_total, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings || !e->have_vocab)
        return fail(e, MSR_ERR_NOT_BOUND, "msr_fuzzy_terms: vocabulary not bound (msr_bind_vocab: the index has no term strings)");
    if (n_words < 0 || n_words > MSR_FUZZY_MAX_WORDS || limit < 1 || limit > MSR_FUZZY_MAX_LIMIT)
        return fail(e, MSR_ERR_INVALID, "msr_fuzzy_terms: bad argument (n_words=%d, at most %d; limit=%d, 1 .. %d)", n_words,
                    MSR_FUZZY_MAX_WORDS, limit, MSR_FUZZY_MAX_LIMIT);
    if (n_words == 0) return MSR_OK;
    if (!word_off || !word_chars || !word_max || !out_term || !out_dist || !out_n || !out_total || !scratch)
        return fail(e, MSR_ERR_INVALID, "msr_fuzzy_terms: bad argument (a NULL pointer with n_words=%d)", n_words);
    const int64_t need = msr_fuzzy_scratch_bytes(e->bm25.n_terms, n_words, limit);
    if (need < 0 || scratch_bytes < need || ((uintptr_t)scratch & 7))
        return fail(e, MSR_ERR_INVALID, "msr_fuzzy_terms: bad argument (scratch_bytes=%lld, needed %lld, 8-byte aligned)",
                    (long long)scratch_bytes, (long long)need);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_fuzzy_terms_run(e->voc_char_off, e->voc_chars, e->voc_weight, e->voc_sig, e->bm25.n_terms, n_words, word_off,
                                   word_chars, word_max, limit, out_term, out_dist, out_n, out_total, scratch,
                                   (hipStream_t)stream));
    return MSR_OK;
}

// ---- K16: prefix and wildcard lookup (msr_wildcard.hip) -------------------------------------------------------------------------
extern "C" int64_t msr_wildcard_scratch_bytes(int64_t n_terms, int32_t n_patterns, int32_t limit) {
    if (n_terms < 0 || n_terms >= (1ll << 31) || n_patterns < 0 || n_patterns > MSR_WILD_MAX_PATTERNS || limit < 1 ||
        limit > MSR_WILD_MAX_LIMIT)
        return -1;
    return (int64_t)n_patterns * msr_fuzzy_spans(n_terms) * ((int64_t)limit * 8 + 4);
}

extern "C" int msr_wildcard_terms(msr_engine* e, int32_t n_patterns, const int32_t* pat_off, const uint16_t* pat_chars,
                                  int32_t limit, int32_t* out_term, int32_t* out_n, int32_t* out_total, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings || !e->have_vocab)
        return fail(e, MSR_ERR_NOT_BOUND, "msr_wildcard_terms: vocabulary not bound (msr_bind_vocab: the index has no term strings)");
    if (n_patterns < 0 || n_patterns > MSR_WILD_MAX_PATTERNS || limit < 1 || limit > MSR_WILD_MAX_LIMIT)
        return fail(e, MSR_ERR_INVALID, "msr_wildcard_terms: bad argument (n_patterns=%d, at most %d; limit=%d, 1 .. %d)",
                    n_patterns, MSR_WILD_MAX_PATTERNS, limit, MSR_WILD_MAX_LIMIT);
    if (n_patterns == 0) return MSR_OK;
    if (!pat_off || !pat_chars || !out_term || !out_n || !out_total || !scratch)
        return fail(e, MSR_ERR_INVALID, "msr_wildcard_terms: bad argument (a NULL pointer with n_patterns=%d)", n_patterns);
    const int64_t need = msr_wildcard_scratch_bytes(e->bm25.n_terms, n_patterns, limit);
    if (need < 0 || scratch_bytes < need || ((uintptr_t)scratch & 7))
        return fail(e, MSR_ERR_INVALID, "msr_wildcard_terms: bad argument (scratch_bytes=%lld, needed %lld, 8-byte aligned)",
                    (long long)scratch_bytes, (long long)need);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_wildcard_terms_run(e->voc_char_off, e->voc_chars, e->voc_weight, e->voc_sig, e->bm25.n_terms, n_patterns,
                                      pat_off, pat_chars, limit, out_term, out_n, out_total, scratch, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_combine_sets(msr_engine* e, int32_t n_rows, const int32_t* and_off, const int32_t* and_rows,
                                const int32_t* not_off, const int32_t* not_rows, const uint32_t* in_bits, int32_t n_in,
                                int64_t in_stride, uint32_t* out_bits, int64_t out_stride, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_combine_sets: postings not bound");
    const int rc = set_rows_args_ok(e, "msr_combine_sets", n_rows, out_bits && and_off && not_off, "out_bits, and_off or not_off",
                                    out_stride, "n_in", n_in, in_bits != nullptr, "in_bits", "in_stride", in_stride);
    if (rc) return rc;
    if (n_rows == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_combine_sets_run(e->bm25.n_docs, n_rows, and_off, and_rows, not_off, not_rows, in_bits, n_in, in_stride,
                                    out_bits, out_stride, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_debug_bm25_split(msr_engine* e, int32_t n_queries, int32_t* tiles_per_item, int32_t* n_segments) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_debug_bm25_split: postings not bound");
    if (n_queries < 1 || n_queries > e->cfg.max_queries || !tiles_per_item || !n_segments)
        return fail(e, MSR_ERR_INVALID, "msr_debug_bm25_split: bad argument (n_queries=%d, max_queries=%d)", n_queries,
                    e->cfg.max_queries);
    int tpw = 1, n_spans = 0;
    msr_bm25_split(e->bm25.n_tiles, n_queries, &tpw, &n_spans);
    *tiles_per_item = tpw;
    *n_segments = n_spans;
    return MSR_OK;
}

// Test-only: the engine's own select (e->sel and the internal entry points of msr_topk.hip, nothing else) over a caller's raw
// score rows, and the SelState of every query as the streaming passes left it (msretr.h).
extern "C" int msr_debug_select(msr_engine* e, int32_t mode, const void* scores, int64_t n, int64_t stride, int32_t n_queries,
                                int32_t k, const int32_t* idx, const int32_t* counts, int32_t n_seg, int64_t seg_stride,
                                const uint64_t* win_base, const uint32_t* set_bits, int32_t n_sets, int64_t set_stride,
                                const int32_t* q_set, const int32_t* gate, int32_t gate_per64, int32_t* out_doc, void* out_score,
                                int32_t* out_n, msr_select_state* out_state, void* stream) {
    static_assert(sizeof(msr_select_state) == sizeof(SelState), "msr_select_state mirrors SelState");
    if (!e) return MSR_ERR_INVALID;
    if (mode < MSR_SELECT_F32 || mode > MSR_SELECT_F64_LIST)
        return fail(e, MSR_ERR_INVALID, "msr_debug_select: bad argument (mode=%d)", mode);
    if (n_queries < 1 || n_queries > e->cfg.max_queries || k < 1 || k > e->cfg.max_k)
        return fail(e, MSR_ERR_INVALID, "msr_debug_select: bad argument (n_queries=%d, max_queries=%d, k=%d, max_k=%d)", n_queries,
                    e->cfg.max_queries, k, e->cfg.max_k);
    if (!scores || !out_doc || !out_score || !out_n || n < 0 || n >= (1ll << 31) || stride < n)
        return fail(e, MSR_ERR_INVALID, "msr_debug_select: bad argument (NULL scores or output, or n=%lld, stride=%lld)",
                    (long long)n, (long long)stride);
    if (mode == MSR_SELECT_F64_LIST && (!idx || !counts || n_seg < 1 || seg_stride < 0 || (int64_t)n_seg * seg_stride > stride))
        return fail(e, MSR_ERR_INVALID, "msr_debug_select: bad argument (list: idx or counts NULL, n_seg=%d < 1, or n_seg * "
                    "seg_stride=%lld > stride=%lld)", n_seg, (long long)seg_stride, (long long)stride);
    if (mode == MSR_SELECT_F32_WITHIN &&
        (n_sets < 1 || !set_bits || !q_set || set_stride < (n + 31) / 32))
        return fail(e, MSR_ERR_INVALID, "msr_debug_select: bad argument (within: n_sets=%d < 1, set_bits or q_set NULL, or "
                    "set_stride=%lld < ceil(n / 32))", n_sets, (long long)set_stride);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    SelScratch sel = e->sel;
    sel.gate = gate;
    sel.gate_per64 = gate && gate_per64 ? 1 : 0;
    switch (mode) {
    case MSR_SELECT_F32:
        HIP_TRY(e, msr_select_topk(32, scores, n, stride, n_queries, k, sel, out_doc, out_score, out_n, st));
        break;
    case MSR_SELECT_F64:
        HIP_TRY(e, msr_select_topk(64, scores, n, stride, n_queries, k, sel, out_doc, out_score, out_n, st));
        break;
    case MSR_SELECT_F32_WITHIN: {
        const MsrSetView set{set_bits, set_stride, q_set, n_sets};
        HIP_TRY(e, msr_select_topk_within((const float*)scores, n, stride, n_queries, k, sel, set, out_doc, (float*)out_score,
                                          out_n, st));
        break;
    }
    default:
        HIP_TRY(e, msr_select_topk_list((const double*)scores, idx, counts, n_seg, seg_stride, stride, n_queries, k, sel, out_doc,
                                        (double*)out_score, out_n, st, win_base));
    }
    if (out_state)
        HIP_TRY(e, hipMemcpyAsync(out_state, e->sel.state, (size_t)n_queries * sizeof(SelState), hipMemcpyDeviceToDevice, st));
    return MSR_OK;
}

// K10: BM25 scores of named documents (everything read was built by msr_bind_postings; no engine scratch)
extern "C" int msr_bm25_score_docs(msr_engine* e, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                                   int32_t n_queries, const int32_t* doc, const int32_t* doc_n, int32_t max_docs,
                                   double* out_score, int32_t* out_touched, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_postings) return fail(e, MSR_ERR_NOT_BOUND, "msr_bm25_score_docs: postings not bound");
    if (n_queries < 0 || max_docs < 0 || !q_term_off || (n_queries > 0 && max_docs > 0 && (!doc || !out_score || !out_touched)))
        return fail(e, MSR_ERR_INVALID, "msr_bm25_score_docs: bad argument (n_queries=%d, max_docs=%d)", n_queries, max_docs);
    if (n_queries == 0 || max_docs == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_bm25_point(e->bm25, q_term_off, q_terms, q_qtf, n_queries, doc, doc_n, max_docs, out_score, out_touched,
                              (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_union_candidates(msr_engine* e, int32_t n_queries, const int32_t* lex_doc, const double* lex_score,
                                    const int32_t* lex_n, int32_t k_lex, const int32_t* dense_doc, const double* dense_bm25,
                                    const int32_t* dense_n, int32_t k_dense, int32_t* out_doc, double* out_score, int32_t* out_src,
                                    int32_t* out_n, int32_t max_cand, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (n_queries < 0 || k_lex < 0 || k_lex > MSR_MAX_K || k_dense < 0 || k_dense > MSR_MAX_K || max_cand < 1 ||
        (int64_t)k_lex + k_dense > max_cand)
        return fail(e, MSR_ERR_INVALID, "msr_union_candidates: bad argument (k_lex=%d, k_dense=%d: each in [0, %d], their sum <= "
                    "max_cand=%d)", k_lex, k_dense, MSR_MAX_K, max_cand);
    if (!out_doc || !out_score || !out_src || !out_n || (k_lex > 0 && (!lex_doc || !lex_score || !lex_n)) ||
        (k_dense > 0 && (!dense_doc || !dense_bm25 || !dense_n)))
        return fail(e, MSR_ERR_INVALID, "msr_union_candidates: bad argument (NULL list)");
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_union_lists(n_queries, lex_doc, lex_score, lex_n, k_lex, dense_doc, dense_bm25, dense_n, k_dense, out_doc,
                               out_score, out_src, out_n, max_cand, (hipStream_t)stream));
    return MSR_OK;
}

// A query whose entries overflowed in the streaming pass (huge tie groups, a zero vector) raised the gate word of its 64-query
// slice: that slice once more on the sweeps, which handle any input.  One scan per slice, gated on its word, into its own score
// rows; then ONE select and ONE best-chunk pass over all rows of the call, in which a query takes part only if its slice's word
// is up.  When no gate is up (the normal case) all these launches return at once.  Queries: e->gf_qn (normalised, nq of them).
static int dense_gated_fallback(msr_engine* e, int nq, int k, int32_t* out_doc, float* out_score, int32_t* out_chunk,
                                int32_t* out_n, hipStream_t st) {
    const int64_t N = e->dense.n_docs;
    DenseIndex ix = e->dense;
    ix.gate = e->gf_gate;
    HIP_TRY(e, msr_dense_scan_slices(ix, e->gf_qn, nq, (float*)e->score_rows, e->gf_fb_qimg, st));
    SelScratch sel = e->sel;
    sel.gate = e->gf_gate; sel.gate_per64 = 1;
    HIP_TRY(e, msr_select_topk(32, e->score_rows, N, e->dense.score_stride, nq, k, sel, out_doc, out_score, out_n, st));
    ix.gate = e->gf_gate; ix.gate_per64 = 1;
    if (out_chunk) HIP_TRY(e, msr_best_chunk(ix, e->gf_qn, nq, k, 0, out_doc, out_n, out_chunk, st));
    return MSR_OK;
}

// Event pairs of a timed two-pass launch: {start, stop} of the sample pass (kind 3), then of the pass of `kind`.  nullptr: not
// timed (every launch gets its own pair out of a ring of EV_RING; later launches are not recorded).  pass_events_used() after
// the launch.
static hipEvent_t* pass_events(msr_engine* e, int kind, hipEvent_t ev[4]) {
    if (!e->timing || e->ev_count[kind] >= msr_engine::EV_RING || e->ev_count[3] >= msr_engine::EV_RING) return nullptr;
    ev[0] = e->ev_start[3][e->ev_count[3]]; ev[1] = e->ev_stop[3][e->ev_count[3]];
    ev[2] = e->ev_start[kind][e->ev_count[kind]]; ev[3] = e->ev_stop[kind][e->ev_count[kind]];
    return ev;
}
static void pass_events_used(msr_engine* e, int kind, const hipEvent_t* ev) {
    if (ev) { e->ev_count[kind]++; e->ev_count[3]++; }
}

extern "C" int msr_dense_split_max(const msr_engine* e, int32_t k) {
    if (!e || !e->have_chunks || k < 1 || k > e->cfg.max_k ||
        !dense_stream_ok(dense_binding(e->dense), 0, e->gf_ok, e->gf.n_tiles, k))
        return 0;
    return e->gf.caps.call_cap;                              // (msr_stream_plan.h)
}

extern "C" int msr_dense_topk_begin(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t k_part, float* out_part,
                                    void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_chunks) return fail(e, MSR_ERR_NOT_BOUND, "msr_dense_topk_begin: chunks not bound");
    if (e->split_pending) return fail(e, MSR_ERR_INVALID, "msr_dense_topk_begin: the previous begin has not been ended");
    const int cap = msr_dense_split_max(e, k);
    if (!q || !out_part || k_part < 1 || k_part > k || n_queries <= 64 || n_queries > cap)
        return fail(e, MSR_ERR_INVALID, "msr_dense_topk_begin: needs 64 < n_queries <= msr_dense_split_max() = %d, 1 <= k_part <= k (got %d, %d, %d)",
                    cap, n_queries, k_part, k);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_prep_queries(q, n_queries, e->gf_qn, dense_fallback_pad(n_queries), st));
    HIP_TRY(e, hipMemsetAsync(e->gf_gate, 0, GF_GATE_BYTES, st));
    hipEvent_t ev_buf[4];
    hipEvent_t* ev = pass_events(e, 0, ev_buf);
    int width = 0;
    int segs = 0;
    HIP_TRY(e, msr_gemm_f32_pass(e->gf, e->dense, e->gf_qn, n_queries, k, k_part, out_part, ev, &width, &segs, st));
    e->last_dense_width = width;
    e->last_dense_segments = segs;
    pass_events_used(e, 0, ev);
    e->split_pending = n_queries;
    return MSR_OK;
}

extern "C" int msr_dense_topk_end(msr_engine* e, int32_t n_queries, int32_t k, const float* bound, int32_t* out_doc,
                                  float* out_score, int32_t* out_chunk, int32_t* out_n, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_chunks) return fail(e, MSR_ERR_NOT_BOUND, "msr_dense_topk_end: chunks not bound");
    if (!e->gf_ok || e->split_pending != n_queries || n_queries <= 0)
        return fail(e, MSR_ERR_INVALID, "msr_dense_topk_end: no matching msr_dense_topk_begin (pending %d, got %d)", e->split_pending, n_queries);
    if (!out_doc || !out_score || !out_n || k < 1 || k > e->cfg.max_k) return fail(e, MSR_ERR_INVALID, "msr_dense_topk_end: bad argument");
    e->split_pending = 0;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_gemm_f32_finish(e->gf, e->dense, e->gf_qn, n_queries, k, bound, out_doc, out_score, out_chunk, out_n, e->gf_gate, st));
    return dense_gated_fallback(e, n_queries, k, out_doc, out_score, out_chunk, out_n, st);
}

// The sweeps of msr_dense_topk for queries [q0, q0 + cnt): one pass over the matrix per dense_slice() queries (msr_dense_scan:
// K-split or narrow kernel), the select of each slice, its best-chunk rows.  `gate` non-null = fallback launches that only do
// work when *gate != 0.  `set` non-null (msr_dense_topk_within; set->q_set indexed by the call's query number): the restricted
// select -- the sweep kernels and the best-chunk pass are the same, so a restricted call sweeps with the kernel an unrestricted
// call of <= 64 queries would run (its bit-for-bit contract).
static int dense_sweeps(msr_engine* e, const float* q, int q0, int cnt, int k, int max_chunks_per_doc, const int32_t* gate,
                        int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_n, hipStream_t st,
                        const MsrSetView* set) {
    const int64_t N = e->dense.n_docs;
    const DenseBinding b = dense_binding(e->dense);
    const int slice = dense_slice(b, max_chunks_per_doc);
    DenseIndex ix = e->dense;
    SelScratch sel = e->sel;
    for (int s0 = q0; s0 < q0 + cnt; s0 += slice) {
        const int nq = std::min(slice, q0 + cnt - s0);
        // gated fallback: one gate word per slice of 64 queries (the streaming path raises the gates of the slices that
        // hold an overflowed query)
        ix.gate = sel.gate = gate ? gate + (s0 - q0) / MSR_DENSE_FALLBACK_SLICE : nullptr;
        // zero rows up to the query blocks of the instance that runs
        const int nq_pad = 16 * dense_plan(b, nq, max_chunks_per_doc).qb;
        const bool timed = !gate && e->timing && e->ev_count[0] < msr_engine::EV_RING;
        HIP_TRY(e, msr_prep_queries(q + (int64_t)s0 * MSR_DIM, nq, e->qn, nq_pad, st));
        if (timed) HIP_TRY(e, hipEventRecord(e->ev_start[0][e->ev_count[0]], st));
        HIP_TRY(e, msr_dense_scan(ix, e->qn, nq, max_chunks_per_doc, (float*)e->score_rows, st));
        if (timed) {
            HIP_TRY(e, hipEventRecord(e->ev_stop[0][e->ev_count[0]], st));
            e->ev_count[0]++;
        }
        if (set) {
            MsrSetView sv = *set;
            sv.q_set += s0;                                      // (the select numbers the slice's queries from 0)
            HIP_TRY(e, msr_select_topk_within((const float*)e->score_rows, N, e->dense.score_stride, nq, k, sel, sv,
                                              out_doc + (int64_t)s0 * k, out_score + (int64_t)s0 * k, out_n + s0, st));
        } else {
            HIP_TRY(e, msr_select_topk(32, e->score_rows, N, e->dense.score_stride, nq, k, sel, out_doc + (int64_t)s0 * k,
                                       out_score + (int64_t)s0 * k, out_n + s0, st));
        }
        if (out_chunk)
            HIP_TRY(e, msr_best_chunk(ix, e->qn, nq, k, max_chunks_per_doc, out_doc + (int64_t)s0 * k,
                                      out_n + s0, out_chunk + (int64_t)s0 * k, st));
    }
    return MSR_OK;
}

extern "C" int msr_dense_topk(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t max_chunks_per_doc,
                              int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_n, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    const bool args_ok = dense_topk_args(e, n_queries, k, max_chunks_per_doc, q, out_doc, out_score, out_n);
    if (const int rc = dense_entry_ok(e, "msr_dense_topk", false, args_ok, k)) return rc;
    if (n_queries == 0) return MSR_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // one sweep of E serves up to 32 queries (wave-streaming kernel) or 64 (K-split kernel); batches of more than 64
    // queries run as a GEMM over the f32 rows, 128 queries per pass (msr_gemm_f32.hip), when the corpus allows it
    const DenseBinding b = dense_binding(e->dense);
    const int slice = dense_slice(b, max_chunks_per_doc);
    const bool gemm = dense_stream_ok(b, max_chunks_per_doc, e->gf_ok, e->gf.n_tiles, k);      // (implies the 64-query slice)
    e->last_dense_width = gemm && n_queries > slice ? 0 : slice;               // (the streaming path reports its own width below)
    e->last_dense_segments = 0;
    int q0 = 0;
    while (q0 < n_queries) {
        const int left = n_queries - q0;
        if (gemm && left > slice) {
            const int nq = std::min(e->gf.caps.call_cap, left);
            // (normalised once for the pass AND for the gated sweeps behind it: zero rows up to the last slice's 64)
            HIP_TRY(e, msr_prep_queries(q + (int64_t)q0 * MSR_DIM, nq, e->gf_qn, dense_fallback_pad(nq), st));
            HIP_TRY(e, hipMemsetAsync(e->gf_gate, 0, GF_GATE_BYTES, st));
            hipEvent_t ev_buf[4];
            hipEvent_t* ev = pass_events(e, 0, ev_buf);
            int width = 0, segs = 0;
            HIP_TRY(e, msr_gemm_f32_topk(e->gf, e->dense, e->gf_qn, nq, k, out_doc + (int64_t)q0 * k,
                                         out_score + (int64_t)q0 * k, out_chunk ? out_chunk + (int64_t)q0 * k : nullptr,
                                         out_n + q0, e->gf_gate, ev, &width, &segs, st));
            e->last_dense_width = std::max(e->last_dense_width, width);
            e->last_dense_segments = segs;
            pass_events_used(e, 0, ev);
            {
                int rcf = dense_gated_fallback(e, nq, k, out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k,
                                               out_chunk ? out_chunk + (int64_t)q0 * k : nullptr, out_n + q0, st);
                if (rcf) return rcf;
            }
            q0 += nq;
        } else {
            const int nq = std::min(slice, left);
            int rc = dense_sweeps(e, q, q0, nq, k, max_chunks_per_doc, nullptr, out_doc, out_score, out_chunk, out_n, st, nullptr);
            if (rc) return rc;
            q0 += nq;
        }
    }
    return MSR_OK;
}

extern "C" int msr_dense_topk_within(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t max_chunks_per_doc,
                                     const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* q_set,
                                     int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_n, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    {
        const bool args_ok = dense_topk_args(e, n_queries, k, max_chunks_per_doc, q, out_doc, out_score, out_n);
        int rc = dense_entry_ok(e, "msr_dense_topk_within", false, args_ok, k);
        if (!rc) rc = within_args_ok(e, "msr_dense_topk_within", e->dense.n_docs, set_bits, n_sets, set_stride, q_set);
        if (rc) return rc;
    }
    if (n_sets == 0)                                             // the unrestricted call
        return msr_dense_topk(e, q, n_queries, k, max_chunks_per_doc, out_doc, out_score, out_chunk, out_n, stream);
    if (n_queries == 0) return MSR_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // every query on the sweeps (the kernels an unrestricted call of <= 64 queries runs), the restriction in the select
    e->last_dense_width = dense_slice(dense_binding(e->dense), max_chunks_per_doc);
    e->last_dense_segments = 0;
    const MsrSetView set{set_bits, set_stride, q_set, n_sets};
    return dense_sweeps(e, q, 0, n_queries, k, max_chunks_per_doc, nullptr, out_doc, out_score, out_chunk, out_n, st, &set);
}

// ---- K9: similar documents (msr_similar.hip) ---------------------------------------------------------------------------------
// 1 if some v[0..n) lies outside [0, hi) (device check, one synchronisation of the stream), 0 if none, < 0 on failure
static int sim_out_of_range(msr_engine* e, const int32_t* v, int64_t n, int64_t hi, hipStream_t st) {
    if (!e->sim_flag) ALLOC(e, e->mem_engine, e->sim_flag, 64);
    int32_t flag = 0;
    HIP_TRY(e, hipMemsetAsync(e->sim_flag, 0, sizeof(int32_t), st));
    HIP_TRY(e, msr_check_range(v, n, hi, e->sim_flag, st));
    HIP_TRY(e, hipMemcpyAsync(&flag, e->sim_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    return flag ? 1 : 0;
}

extern "C" int msr_gather_rows(msr_engine* e, const int32_t* rows, int32_t n, float* out, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_chunks) return fail(e, MSR_ERR_NOT_BOUND, "msr_gather_rows: chunks not bound");
    if (n < 0 || (n > 0 && (!rows || !out))) return fail(e, MSR_ERR_INVALID, "msr_gather_rows: bad argument (n=%d)", n);
    if (n == 0) return MSR_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const int bad = sim_out_of_range(e, rows, n, e->dense.n_chunks, st);
    if (bad < 0) return bad;
    if (bad) return fail(e, MSR_ERR_INVALID, "msr_gather_rows: a row lies outside [0, n_chunks = %lld)", (long long)e->dense.n_chunks);
    HIP_TRY(e, msr_gather_rows_run(e->dense, rows, n, out, st));
    return MSR_OK;
}

extern "C" int msr_dense_topk_grouped(msr_engine* e, const float* q, int32_t n_rows, const int32_t* group_off, int32_t n_groups,
                                      const int32_t* excl_off, const int32_t* excl_doc, int32_t k, float min_score,
                                      const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* g_set,
                                      int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_src_row,
                                      int32_t* out_n, void* stream) {
    static const char* fn = "msr_dense_topk_grouped";
    if (!e) return MSR_ERR_INVALID;
    if (const int rc = dense_entry_ok(e, fn, false, true, k)) return rc;     // (the arguments: worded for this call below)
    if (n_rows < 0 || n_groups < 0 || k < 1 || k > e->cfg.max_k || min_score != min_score || !group_off || !excl_off ||
        (n_rows > 0 && !q) || (n_groups > 0 && (!out_doc || !out_score || !out_chunk || !out_src_row || !out_n)))
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (n_rows=%d, n_groups=%d, k=%d, max_k=%d)", fn, n_rows, n_groups, k,
                    e->cfg.max_k);
    {
        const int rc = within_args_ok(e, fn, e->dense.n_docs, set_bits, n_sets, set_stride, g_set);
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // the offsets on the host: their checks, and the list depth k + max |excl_g| every row is asked for
    std::vector<int32_t> h_goff((size_t)n_groups + 1), h_eoff((size_t)n_groups + 1);
    HIP_TRY(e, hipMemcpyAsync(h_goff.data(), group_off, h_goff.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipMemcpyAsync(h_eoff.data(), excl_off, h_eoff.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (h_goff[0] != 0 || h_goff[n_groups] != n_rows)
        return fail(e, MSR_ERR_INVALID, "%s: group_off must run from 0 to n_rows = %d (got %d .. %d)", fn, n_rows, h_goff[0],
                    h_goff[n_groups]);
    if (h_eoff[0] != 0) return fail(e, MSR_ERR_INVALID, "%s: excl_off[0] = %d, must be 0", fn, h_eoff[0]);
    int max_excl = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (h_goff[g + 1] < h_goff[g]) return fail(e, MSR_ERR_INVALID, "%s: group_off not monotone at group %d", fn, g);
        if (h_eoff[g + 1] < h_eoff[g]) return fail(e, MSR_ERR_INVALID, "%s: excl_off not monotone at group %d", fn, g);
        max_excl = std::max(max_excl, h_eoff[g + 1] - h_eoff[g]);
    }
    if ((int64_t)k + max_excl > e->cfg.max_k)
        return fail(e, MSR_ERR_INVALID, "%s: k + max |excl_g| = %lld exceeds max_k = %d", fn, (long long)k + max_excl, e->cfg.max_k);
    const int64_t n_excl = h_eoff[n_groups];
    if (n_excl > 0) {
        if (!excl_doc) return fail(e, MSR_ERR_INVALID, "%s: excl_doc is NULL with %lld exclusions", fn, (long long)n_excl);
        const int bad = sim_out_of_range(e, excl_doc, n_excl, e->dense.n_docs, st);
        if (bad < 0) return bad;
        if (bad) return fail(e, MSR_ERR_INVALID, "%s: an excluded document lies outside [0, n_docs = %lld)", fn, (long long)e->dense.n_docs);
    }
    if (n_groups == 0) return MSR_OK;
    // scratch: the per-row lists (doc, score, chunk [n_rows][kk], n [n_rows]), the per-row set indices, the overflow records
    const int kk = k + max_excl;
    const size_t L = (size_t)n_rows * kk;
    const size_t lists_bytes = (L * 3 + 2 * (size_t)n_rows + 64) * 4;
    int rc = grow(e, e->mem_engine, &e->sim_lists, &e->sim_lists_bytes, lists_bytes, "grouped lists");
    if (rc) return rc;
    rc = grow(e, e->mem_engine, &e->sim_over, &e->sim_over_bytes, 2 * L * 16 + 64, "grouped merge records");
    if (rc) return rc;
    int32_t* l_doc = (int32_t*)e->sim_lists;
    float* l_score = (float*)(l_doc + L);
    int32_t* l_chunk = (int32_t*)(l_score + L);
    int32_t* l_n = l_chunk + L;
    int32_t* row_set = l_n + n_rows;
    if (n_sets > 0) HIP_TRY(e, msr_group_row_sets(group_off, n_groups, g_set, row_set, st));
    // the per-row lists: one msr_dense_topk(_within) call per max_queries rows (one call when n_rows <= max_queries)
    for (int r0 = 0; r0 < n_rows; r0 += e->cfg.max_queries) {
        const int cnt = std::min(e->cfg.max_queries, n_rows - r0);
        const int64_t o = (int64_t)r0 * kk;
        rc = msr_dense_topk_within(e, q + (int64_t)r0 * MSR_DIM, cnt, kk, 0, set_bits, n_sets, set_stride,
                                   n_sets > 0 ? row_set + r0 : nullptr, l_doc + o, l_score + o, l_chunk + o, l_n + r0, stream);
        if (rc) return rc;
    }
    GroupedMergeArgs a{};
    a.l_doc = l_doc; a.l_score = l_score; a.l_chunk = l_chunk; a.l_n = l_n; a.kk = kk;
    a.group_off = group_off; a.excl_off = excl_off; a.excl_doc = excl_doc; a.k = k; a.min_score = min_score;
    a.out_doc = out_doc; a.out_score = out_score; a.out_chunk = out_chunk; a.out_src = out_src_row; a.out_n = out_n;
    a.g_hi = (uint64_t*)e->sim_over;
    a.g_lo = (uint32_t*)(a.g_hi + 2 * L);
    a.g_val = a.g_lo + 2 * L;
    HIP_TRY(e, msr_grouped_merge(a, n_groups, st));
    return MSR_OK;
}

static int rerank_args_ok(msr_engine* e, const char* fn, int32_t n_queries, int32_t max_cand, int32_t max_chunks) {
    if (n_queries < 0 || max_cand < 1 || max_cand > e->cfg.rerank_max_docs)
        return fail(e, MSR_ERR_INVALID, "%s: bad argument (max_cand=%d, rerank_max_docs=%d)", fn, max_cand,
                    e->cfg.rerank_max_docs);
    if (max_chunks < 1 || max_chunks > MSR_RERANK_MAX_CHUNKS)
        return fail(e, MSR_ERR_INVALID, "%s: max_chunks out of range [1, %d]", fn, MSR_RERANK_MAX_CHUNKS);
    return MSR_OK;
}

static constexpr int BT_SLICE = 128;                        // most queries per bf16 K-split sweep
static constexpr int GM_SLICE = 1024;                       // queries per pass of the GEMM path (4 query tiles of 256)
static constexpr int GM_WV_CAP = 16384;                     // emitted entries per wave (x 8 waves x #CU x 16 B = 512 MB at 256 CUs)

// The bf16 image of the bound rows, the sweeps' tables and, when the corpus has the row tiles for it, the GEMM path.
static int build_bf16(msr_engine* e, hipStream_t st) {
    const int64_t C = e->dense.n_chunks;
    // The image holds the rows NORMALISED and then rounded to bf16 (so a score needs no per-row scale and the error bound
    // of msr_batch.hip is about unit vectors), padded with 512 zero rows: the GEMM reads 256 rows from any tile start.
    const int64_t n_pad = C + 512;
    ALLOC(e, e->mem_bf16, e->emb_bf16, (size_t)n_pad * MSR_DIM * 2);
    const size_t QS = GM_SLICE;                             // the candidate scratch serves both the sweeps and the GEMM path
    // (the candidate scratch is the engine's, not the binding's: the first call allocates it, re-binds keep it)
    if (!e->bt_top_doc) ALLOC(e, e->mem_engine, e->bt_top_doc, (size_t)BT_SLICE * MSR_MAX_K * 4);
    if (!e->bt_top_score) ALLOC(e, e->mem_engine, e->bt_top_score, (size_t)BT_SLICE * MSR_MAX_K * 4);
    if (!e->bt_top_n) ALLOC(e, e->mem_engine, e->bt_top_n, (size_t)BT_SLICE * 4);
    if (!e->bt_cand_doc) ALLOC(e, e->mem_engine, e->bt_cand_doc, QS * MSR_SEL_CAP * 4);
    if (!e->bt_cand_score) ALLOC(e, e->mem_engine, e->bt_cand_score, QS * MSR_SEL_CAP * 4);
    if (!e->bt_cand_chunk) ALLOC(e, e->mem_engine, e->bt_cand_chunk, QS * MSR_SEL_CAP * 4);
    if (!e->bt_cand_n) ALLOC(e, e->mem_engine, e->bt_cand_n, QS * 4);
    ALLOC(e, e->mem_bf16, e->bf_ones, (size_t)C * 4);
    ALLOC(e, e->mem_bf16, e->bf_err, 4);
    ALLOC(e, e->mem_bf16, e->bf_margin, QS * 4);
    HIP_TRY(e, hipMemsetAsync(e->bt_cand_n, 0, QS * 4, st));
    HIP_TRY(e, msr_unit_bf16_rows(e->dense.emb, e->dense.inv_norm, C, n_pad, e->emb_bf16, e->bf_err, st));
    HIP_TRY(e, msr_fill_f32(e->bf_ones, C, 1.0f, st));
    e->dense.emb_bf16 = e->emb_bf16;
    e->dense_bf16 = e->dense;
    e->dense_bf16.inv_norm = e->bf_ones;
    if (e->dense.wide_ok) {
        ALLOC(e, e->mem_bf16, e->bf_row_meta, (size_t)(C + 16) * 8);
        HIP_TRY(e, msr_pack_row_meta(e->chunk_doc, e->bf_ones, C, e->bf_row_meta, st));
        e->dense_bf16.row_meta = e->bf_row_meta;
    }
    // ---- GEMM path: needs the row tiles built at bind time (every document inside one 256-row tile) ----
    const int n_tiles = e->n_tiles;
    const int grid = e->n_cus / 8 * 8;
    if (e->tiles_ok && n_tiles >= 64 && grid >= 32) {
        const int stride = (n_tiles + 31) / 32 * 32;
        GemmIndex& g = e->gemm;
        g.emb_n = e->emb_bf16; g.tile_row = e->tile_row; g.n_tiles = n_tiles; g.n_cus = e->n_cus; g.max_queries = GM_SLICE;
        g.tmax_stride = stride; g.wv_cap = GM_WV_CAP;
        ALLOC(e, e->mem_bf16, g.qmat, (size_t)GM_SLICE * MSR_DIM * 2);
        ALLOC(e, e->mem_bf16, e->gm_qn, (size_t)GM_SLICE * MSR_DIM * 4);
        ALLOC(e, e->mem_bf16, g.tmax, (size_t)GM_SLICE * stride * 4);
        ALLOC(e, e->mem_bf16, g.tmax_t, (size_t)n_tiles * 2 * GM_SLICE * 4);     // [tile][query] (x 2: the diagnostic build's round-2 kernel stores two rows per tile)
        ALLOC(e, e->mem_bf16, g.thr, (size_t)GM_SLICE * 4);
        ALLOC(e, e->mem_bf16, g.thr2, (size_t)GM_SLICE * 4);
        ALLOC(e, e->mem_bf16, g.flag, (size_t)GM_SLICE * 4);
        ALLOC(e, e->mem_bf16, g.wgbuf, (size_t)grid * 8 * GM_WV_CAP * 16);
        ALLOC(e, e->mem_bf16, g.wv_count, (size_t)grid * 8 * 4);
        ALLOC(e, e->mem_bf16, g.pairs, (size_t)GM_SLICE * msr_gemm_pair_cap() * 8);
        ALLOC(e, e->mem_bf16, g.pair_n, (size_t)GM_SLICE * 4);
        HIP_TRY(e, hipMemsetAsync(g.pair_n, 0, (size_t)GM_SLICE * 4, st));
        e->gemm_ok = true;
    }
    return MSR_OK;
}

extern "C" int msr_enable_bf16(msr_engine* e, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_chunks) return fail(e, MSR_ERR_NOT_BOUND, "msr_enable_bf16: chunks not bound");
    if (e->cfg.scan_layout != 0) return fail(e, MSR_ERR_INVALID, "msr_enable_bf16: needs the row-major layout");
    if (e->emb_bf16) return MSR_OK;                          // (built whole: a failed build leaves nothing behind)
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const int rc = build_bf16(e, (hipStream_t)stream);
    if (rc) drop_bf16(e);                                    // a retry starts clean
    return rc;
}

extern "C" int msr_tune(msr_engine* e, int32_t key, int32_t value) {
    if (!e) return MSR_ERR_INVALID;
#ifdef MSR_DIAG
    if (key == 100) { msr_gemm_set_dbg(value); return MSR_OK; }      // timing experiments of the diagnostic build
    if (key == 101) { msr_gemm_f32_set_dbg(value); return MSR_OK; }
    if (key == 102) { msr_bm25_set_dbg(value); return MSR_OK; }
#endif
    return fail(e, MSR_ERR_INVALID, "msr_tune: unknown key %d / value %d", key, value);
}

extern "C" int msr_batch_gemm_ok(const msr_engine* e) { return e && e->have_chunks && e->emb_bf16 && e->gemm_ok ? 1 : 0; }

// Test-only: the counter of msr_debug_scratch_dirty.  Grid-stride dword loads of the counted words, a wave reduction, an LDS
// reduction over the workgroup's waves and ONE 64-bit integer add per workgroup into *out (cleared by the launcher): integer
// sums, so the result does not depend on the order of the adds.  The counted buffer is only read.
static constexpr int CNZ_THREADS = 256;
static constexpr int CNZ_MAX_BLOCKS = 1024;
__global__ __launch_bounds__(CNZ_THREADS) void count_nonzero_kernel(const uint32_t* __restrict__ w, int64_t n,
                                                                     unsigned long long* __restrict__ out) {
    __shared__ unsigned int s_part[CNZ_THREADS / 64];
    unsigned int c = 0;                                      // (a thread sees at most n / (grid x 256) + 1 < 2^32 words)
    const int64_t step = (int64_t)gridDim.x * CNZ_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CNZ_THREADS + threadIdx.x; i < n; i += step) c += w[i] != 0u;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int i = 0; i < CNZ_THREADS / 64; ++i) sum += s_part[i];
        if (sum) atomicAdd(out, sum);
    }
}

static hipError_t count_nonzero(const void* dev, int64_t n_words, int64_t* out, hipStream_t st) {
    hipError_t err = hipMemsetAsync(out, 0, sizeof(int64_t), st);
    if (err != hipSuccess || n_words == 0) return err;
    const int64_t blocks = std::min<int64_t>(CNZ_MAX_BLOCKS, (n_words + CNZ_THREADS - 1) / CNZ_THREADS);
    count_nonzero_kernel<<<(unsigned)blocks, CNZ_THREADS, 0, st>>>((const uint32_t*)dev, n_words, (unsigned long long*)out);
    return hipGetLastError();
}

extern "C" int msr_debug_count_nonzero(const void* dev, int64_t n_words, int64_t* out, void* stream) {
    if (n_words < 0 || !out || (n_words > 0 && (!dev || ((uintptr_t)dev & 3))))
        return msr_fail_global(MSR_ERR_INVALID, "msr_debug_count_nonzero: bad argument (n_words=%lld, NULL out, or dev NULL / not "
                               "4-byte aligned)", (long long)n_words);
    hipError_t err = count_nonzero(dev, n_words, out, (hipStream_t)stream);
    if (err != hipSuccess) return msr_fail_global(MSR_ERR_HIP, "msr_debug_count_nonzero: %s", hipGetErrorString(err));
    return MSR_OK;
}

// Test-only: non-zero words of every buffer documented "zero between calls", over its whole allocation (msretr.h).  The extents
// are the ones of the ALLOC lines: create_scratch (sel), bind_stream_pass (gf), build_bf16 (gemm, bt_cand_n).
extern "C" int msr_debug_scratch_dirty(msr_engine* e, int64_t* out, int32_t n_out, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!out || n_out < MSR_DIRTY_SLOTS)
        return fail(e, MSR_ERR_INVALID, "msr_debug_scratch_dirty: bad argument (NULL out or n_out=%d < %d)", n_out, MSR_DIRTY_SLOTS);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (!e->dirty_counts) ALLOC(e, e->mem_engine, e->dirty_counts, MSR_DIRTY_SLOTS * sizeof(int64_t));
    const int64_t nq = std::max(e->cfg.max_queries, 128);
    const int64_t gf_q = (int64_t)e->gf.caps.groups * 128;
    struct { const void* p; int64_t words; } buf[MSR_DIRTY_SLOTS] = {};
    buf[MSR_DIRTY_SEL_HIST] = {e->sel.hist, nq * MSR_SEL_BINS};
    buf[MSR_DIRTY_SEL_CAND_N] = {e->sel.cand_n, nq};
    buf[MSR_DIRTY_GEMM_PAIR_N] = {e->gemm.pair_n, GM_SLICE};
    buf[MSR_DIRTY_F32_PAIR_N] = {e->gf.pair_n, gf_q};
    buf[MSR_DIRTY_F32_CAND_N] = {e->gf.cand_n, gf_q};
    buf[MSR_DIRTY_BT_CAND_N] = {e->bt_cand_n, GM_SLICE};
    for (int s = 0; s < MSR_DIRTY_SLOTS; ++s)
        if (buf[s].p) HIP_TRY(e, count_nonzero(buf[s].p, buf[s].words, e->dirty_counts + s, st));
    int64_t host[MSR_DIRTY_SLOTS];
    HIP_TRY(e, hipMemcpyAsync(host, e->dirty_counts, sizeof(host), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    for (int s = 0; s < MSR_DIRTY_SLOTS; ++s) out[s] = buf[s].p ? host[s] : -1;
    out[MSR_DIRTY_SPLIT_PENDING] = e->split_pending;
    return MSR_OK;
}

extern "C" int msr_dense_topk_bf16(msr_engine* e, const float* q, int32_t n_queries, int32_t k,
                                   int32_t max_chunks_per_doc, int32_t* out_doc, float* out_score, int32_t* out_chunk,
                                   int32_t* out_n, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    const bool args_ok = dense_topk_args(e, n_queries, k, max_chunks_per_doc, q, out_doc, out_score, out_n);
    if (const int rc = dense_entry_ok(e, "msr_dense_topk_bf16", true, args_ok, k)) return rc;
    if (n_queries == 0) return MSR_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const int64_t N = e->dense.n_docs;
    // candidate margin: 2 eps_q from the measured rounding errors of the image and of each query (msr_batch.hip)
    // More than 128 queries: the tiled GEMM (msr_gemm.hip), GM_SLICE queries per pair of passes.  It needs whole
    // documents inside 256-row tiles, at least 2 k tiles (the sample bound) and no per-document row limit.
    if (e->gemm_ok && max_chunks_per_doc == 0 && n_queries > BT_SLICE && e->gemm.n_tiles >= 2 * k) {
        for (int q0 = 0; q0 < n_queries; q0 += GM_SLICE) {
            const int nq = std::min(GM_SLICE, n_queries - q0);
            HIP_TRY(e, msr_prep_queries(q + (int64_t)q0 * MSR_DIM, nq, e->gm_qn, nq, st));
            HIP_TRY(e, msr_batch_margin(e->gm_qn, nq, e->bf_err, e->bf_margin, st));
            hipEvent_t ev_buf[4];
            hipEvent_t* ev = pass_events(e, 2, ev_buf);
            // (candidates with the runs of their emitted rows: bt_cand_chunk carries first | len << 13 in, the arg-max row out)
            HIP_TRY(e, msr_gemm_candidates(e->gemm, e->dense, e->gm_qn, nq, k, e->bf_margin, e->bt_cand_doc, e->bt_cand_chunk,
                                           e->bt_cand_n, ev, st));
            pass_events_used(e, 2, ev);
            HIP_TRY(e, msr_batch_rescore_rows(e->dense, e->gm_qn, nq, k, (const int32_t*)e->gemm.pairs, 2, msr_gemm_pair_cap(),
                                              e->bt_cand_doc, e->bt_cand_score, e->bt_cand_chunk, e->bt_cand_n,
                                              out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k,
                                              out_chunk ? out_chunk + (int64_t)q0 * k : nullptr, out_n + q0, st));
        }
        return MSR_OK;
    }
    // 33..128 queries: K-split kernel (msr_dense_ks.hip), by the plan of msr_dense_plan.h.  (The image holds unit rows:
    // dense_bf16 carries inverse norms of 1.)
    DenseIndex ix = e->dense_bf16;
#ifdef MSR_DIAG
    // Diagnostic build only: MSR_BF16_WIDE=0 keeps the wave-streaming kernel everywhere -- the plan sees no ring precondition
    static const bool wide_knob = [] { const char* v = getenv("MSR_BF16_WIDE"); return !v || atoi(v) != 0; }();
    if (!wide_knob) ix.wide_ok = ix.wide_ok64 = 0;
#endif
    const DenseBinding b = dense_binding(ix);
    const int slice = dense_bf16_slice(b, max_chunks_per_doc);
    for (int q0 = 0; q0 < n_queries; q0 += slice) {
        const int nq = std::min(slice, n_queries - q0);
        // zero rows up to the query blocks of the instance that runs
        const int nq_pad = 16 * dense_bf16_plan(b, nq, max_chunks_per_doc).qb;
        HIP_TRY(e, msr_prep_queries(q + (int64_t)q0 * MSR_DIM, nq, e->qn, nq_pad, st));
        HIP_TRY(e, msr_batch_margin(e->qn, nq, e->bf_err, e->bf_margin, st));
        const bool timed = e->timing && e->ev_count[0] < msr_engine::EV_RING;
        if (timed) HIP_TRY(e, hipEventRecord(e->ev_start[0][e->ev_count[0]], st));
        HIP_TRY(e, msr_dense_scan_bf16(ix, e->qn, nq, max_chunks_per_doc, (float*)e->score_rows, st));
        if (timed) {
            HIP_TRY(e, hipEventRecord(e->ev_stop[0][e->ev_count[0]], st));
            e->ev_count[0]++;
        }
        // k-th largest approximate score per query
        HIP_TRY(e, msr_select_topk(32, (const float*)e->score_rows, N, e->dense.score_stride, nq, k, e->sel, e->bt_top_doc,
                                   e->bt_top_score, e->bt_top_n, st));
        HIP_TRY(e, msr_batch_finish(e->dense, e->qn, nq, k, max_chunks_per_doc, e->bf_margin, (const float*)e->score_rows,
                                    e->bt_top_score, e->bt_top_n, e->bt_cand_doc, e->bt_cand_score, e->bt_cand_chunk,
                                    e->bt_cand_n, out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k,
                                    out_chunk ? out_chunk + (int64_t)q0 * k : nullptr, out_n + q0, st));
    }
    return MSR_OK;
}

static int rerank_gather_impl(msr_engine* e, const char* fn, const float* q, int32_t n_queries, const int32_t* cand_doc,
                              const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base, int32_t max_chunks,
                              float* out_cos, int32_t* out_meta, int32_t q_per_block, int64_t block_stride, void* stream,
                              const RerankRecords* rec = nullptr) {
    if (!e) return MSR_ERR_INVALID;
    if (!e->have_chunks) return fail(e, MSR_ERR_NOT_BOUND, "%s: chunks not bound", fn);
    if (!q || !cand_doc || !cand_n || (!rec && (!out_cos || !out_meta))) return fail(e, MSR_ERR_INVALID, "%s: null argument", fn);
    int rc = rerank_args_ok(e, fn, n_queries, max_cand, max_chunks);
    if (rc) return rc;
    if (e->url_group && e->url_group_n != e->dense.n_docs)
        return fail(e, MSR_ERR_INVALID, "%s: doc meta bound for %lld docs, chunks for %lld", fn,
                    (long long)e->url_group_n, (long long)e->dense.n_docs);
    if (n_queries == 0) return MSR_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // ONE normalisation and ONE gather launch for up to max(max_queries, 128) queries (the scratch for the normalised queries)
    const int cap = std::max(e->cfg.max_queries, 128);
    for (int q0 = 0; q0 < n_queries; q0 += cap) {
        const int nq = std::min(cap, n_queries - q0);
        if (q0 % q_per_block != 0 && q_per_block < n_queries)
            return fail(e, MSR_ERR_INVALID, "%s: max_queries must be a multiple of queries_per_block for calls this large", fn);
        HIP_TRY(e, msr_prep_queries(q + (int64_t)q0 * MSR_DIM, nq, e->rr_qn, nq, st));
        const int64_t o = (int64_t)q0 * max_cand;
        const bool blocked = q_per_block < n_queries;
        float* co = blocked ? out_cos + (int64_t)(q0 / q_per_block) * block_stride : out_cos + o * MSR_RERANK_MAX_CHUNKS;
        int32_t* mo = blocked ? out_meta + (int64_t)(q0 / q_per_block) * block_stride : out_meta + o * 3;
        RerankRecords rr{nullptr, nullptr, nullptr, 0, 0};
        if (rec) rr = RerankRecords{rec->out, rec->q_base + q0, rec->blk_off + (int64_t)q0 * ((max_cand + 7) / 8), rec->capacity, q0};
        HIP_TRY(e, msr_rerank_gather(e->dense, e->url_group, e->rr_qn, nq, cand_doc + o, cand_n + q0, max_cand, doc_base,
                                     row_base, max_chunks, co, mo, blocked ? q_per_block : nq, blocked ? block_stride : 0, rr, st));
    }
    return MSR_OK;
}

extern "C" int msr_rerank_gather(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                                 const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base,
                                 int32_t max_chunks, float* out_cos, int32_t* out_meta, void* stream) {
    return rerank_gather_impl(e, "msr_rerank_gather", q, n_queries, cand_doc, cand_n, max_cand, doc_base, row_base, max_chunks,
                              out_cos, out_meta, n_queries > 0 ? n_queries : 1, 0, stream);
}

extern "C" int msr_rerank_gather_blocks(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                                        const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base,
                                        int32_t max_chunks, int32_t* out_blocks, int32_t queries_per_block,
                                        int64_t block_words, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (queries_per_block < 1 || block_words < (int64_t)queries_per_block * max_cand * (MSR_RERANK_MAX_CHUNKS + 3))
        return fail(e, MSR_ERR_INVALID, "msr_rerank_gather_blocks: a block of %lld words cannot hold %d queries", (long long)block_words,
                    queries_per_block);
    // block b = [cos of its queries: qpb x max_cand x 10 | meta: qpb x max_cand x 3 | padding]
    return rerank_gather_impl(e, "msr_rerank_gather_blocks", q, n_queries, cand_doc, cand_n, max_cand, doc_base, row_base,
                              max_chunks, (float*)out_blocks, out_blocks + (int64_t)queries_per_block * max_cand * MSR_RERANK_MAX_CHUNKS,
                              queries_per_block, block_words, stream);
}

extern "C" int msr_rerank_plan(msr_engine* e, int32_t n_queries, const int32_t* cand_doc, const int32_t* cand_n,
                               int32_t max_cand, const int32_t* shard_bounds, int32_t n_shards, int32_t my_shard,
                               int32_t queries_per_shard, int32_t* counts, int32_t* send_base, int32_t* send_blk,
                               int32_t* recv_off, int32_t* pair, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!cand_doc || !cand_n || !shard_bounds || !counts || !send_base || !send_blk || !recv_off || !pair || n_queries < 0 ||
        max_cand < 1 || max_cand > 1024 || n_shards < 1 || n_shards > 64 || my_shard < 0 || my_shard >= n_shards ||
        queries_per_shard < 1 || (int64_t)queries_per_shard * n_shards < n_queries)
        return fail(e, MSR_ERR_INVALID, "msr_rerank_plan: bad argument (n_shards=%d, my_shard=%d, queries_per_shard=%d)", n_shards,
                    my_shard, queries_per_shard);
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_rerank_plan_run(n_queries, cand_doc, cand_n, max_cand, shard_bounds, n_shards, my_shard, queries_per_shard,
                                   counts, send_base, send_blk, recv_off, pair, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_rerank_gather_records(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                                         const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base,
                                         int32_t max_chunks, const int32_t* send_base, const int32_t* send_blk,
                                         int32_t* out_records, int64_t capacity_records, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!send_base || !send_blk || !out_records || capacity_records < 0)
        return fail(e, MSR_ERR_INVALID, "msr_rerank_gather_records: bad argument");
    const RerankRecords rec{out_records, send_base, send_blk, capacity_records, 0};
    return rerank_gather_impl(e, "msr_rerank_gather_records", q, n_queries, cand_doc, cand_n, max_cand, doc_base, row_base,
                              max_chunks, nullptr, nullptr, n_queries > 0 ? n_queries : 1, 0, stream, &rec);
}

extern "C" int msr_rerank_scatter(msr_engine* e, const int32_t* records, int64_t capacity_records, const int32_t* counts,
                                  const int32_t* recv_off, int32_t n_shards, int32_t n_queries, int32_t queries_per_shard,
                                  int32_t first_query, int32_t n_my_queries, int32_t max_cand, float* out_cos, int32_t* out_meta,
                                  void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!records || capacity_records < 0 || !counts || !recv_off || !out_cos || !out_meta || n_shards < 1 || n_shards > 64 || max_cand < 1 ||
        max_cand > 1024 || n_my_queries < 0 || n_my_queries > queries_per_shard || first_query < 0 ||
        first_query + n_my_queries > n_queries)
        return fail(e, MSR_ERR_INVALID, "msr_rerank_scatter: bad argument (n_shards=%d, first_query=%d, n_my_queries=%d)", n_shards,
                    first_query, n_my_queries);
    if (n_my_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_rerank_scatter_run(records, capacity_records, counts, recv_off, n_shards, n_queries, queries_per_shard, first_query,
                                      n_my_queries, max_cand, out_cos, out_meta, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_rerank_fuse(msr_engine* e, int32_t n_queries, const int32_t* cand_doc, const double* cand_bm25,
                               const int32_t* cand_n, int32_t max_cand, const float* cos, const int32_t* meta,
                               const msr_rerank_params* params, int32_t* out_doc, double* out_score,
                               double* out_orig, int32_t* out_chunk, int32_t* out_n, int32_t* out_rows, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!cand_doc || !cand_bm25 || !cand_n || !cos || !meta || !params || !out_doc || !out_score || !out_orig ||
        !out_chunk || !out_n || !out_rows)
        return fail(e, MSR_ERR_INVALID, "msr_rerank_fuse: null argument");
    int rc = rerank_args_ok(e, "msr_rerank_fuse", n_queries, max_cand, params->max_chunks);
    if (rc) return rc;
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const RerankParams p{params->smoothing, params->max_boost, params->max_decay, params->max_chunks};
    HIP_TRY(e, msr_rerank_fuse_run(n_queries, cand_doc, cand_bm25, cand_n, max_cand, p, cos, meta, out_doc, out_score,
                                   out_orig, out_chunk, out_n, out_rows, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_rerank_combine(msr_engine* e, const float* cos_parts, const int32_t* meta_parts, int32_t n_parts,
                                  int64_t part_stride_bytes, int32_t n_queries, int32_t max_cand, float* out_cos,
                                  int32_t* out_meta, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!cos_parts || !meta_parts || !out_cos || !out_meta || n_parts < 1 || n_parts > 64 || n_queries < 0 || max_cand < 1 ||
        max_cand > 1024 || part_stride_bytes < 0 || (part_stride_bytes & 3) || (n_parts > 1 && part_stride_bytes == 0))
        return fail(e, MSR_ERR_INVALID, "msr_rerank_combine: bad argument (n_parts=%d, max_cand=%d)", n_parts, max_cand);
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const int64_t rows = (int64_t)n_queries * max_cand;
    HIP_TRY(e, msr_or_parts(cos_parts, n_parts, part_stride_bytes, rows * MSR_RERANK_MAX_CHUNKS, out_cos, (hipStream_t)stream));
    HIP_TRY(e, msr_or_parts(meta_parts, n_parts, part_stride_bytes, rows * 3, out_meta, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_rerank(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                          const double* cand_bm25, const int32_t* cand_n, int32_t max_cand,
                          const msr_rerank_params* params, int32_t* out_doc, double* out_score, double* out_orig,
                          int32_t* out_chunk, int32_t* out_n, int32_t* out_rows, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!params) return fail(e, MSR_ERR_INVALID, "msr_rerank: null params");
    // unsharded convenience: gather (this engine owns every document) + fuse, slice by slice
    const int slice = std::max(e->cfg.max_queries, 128);    // the gather scratch holds this many queries
    for (int q0 = 0; q0 < n_queries; q0 += slice) {
        const int nq = std::min(slice, n_queries - q0);
        const int64_t o = (int64_t)q0 * max_cand;
        int rc = msr_rerank_gather(e, q ? q + (int64_t)q0 * MSR_DIM : nullptr, nq, cand_doc ? cand_doc + o : nullptr,
                                   cand_n ? cand_n + q0 : nullptr, max_cand, 0, 0, params->max_chunks, e->rerank_cos,
                                   e->rerank_meta, stream);
        if (rc) return rc;
        rc = msr_rerank_fuse(e, nq, cand_doc + o, cand_bm25 ? cand_bm25 + o : nullptr, cand_n + q0, max_cand,
                             e->rerank_cos, e->rerank_meta, params, out_doc ? out_doc + o : nullptr,
                             out_score ? out_score + o : nullptr, out_orig ? out_orig + o : nullptr,
                             out_chunk ? out_chunk + o : nullptr, out_n ? out_n + q0 : nullptr,
                             out_rows ? out_rows + q0 : nullptr, stream);
        if (rc) return rc;
    }
    return MSR_OK;
}

extern "C" int msr_merge_topk_payload(msr_engine* e, const int32_t* in_doc, const void* in_score, const int32_t* in_n,
                                      const int32_t* in_payload, int32_t n_parts, int64_t part_stride_bytes,
                                      int32_t n_queries, int32_t k, int32_t score_bits, int32_t* out_doc, void* out_score,
                                      int32_t* out_n, int32_t* out_payload, void* stream) {
    if (!e) return MSR_ERR_INVALID;
    if (!in_doc || !in_score || !in_n || !out_doc || !out_score || !out_n || n_parts < 1 || n_parts > 64 ||
        n_queries < 0 || k < 1 || k > MSR_MAX_K || (score_bits != 32 && score_bits != 64) ||
        (in_payload != nullptr) != (out_payload != nullptr) || part_stride_bytes < 0 || (part_stride_bytes & 7))
        return fail(e, MSR_ERR_INVALID, "msr_merge_topk: bad argument (n_parts=%d, k=%d)", n_parts, k);
    {   // the merge tree's LDS layout: n_parts rounded up to a power of two lists of k rounded up to a power of two (>= 64) entries
        int64_t lists = 1, entries = 64;
        while (lists < n_parts) lists <<= 1;
        while (entries < k) entries <<= 1;
        if (lists * entries > MSR_MERGE_MAX_ENTRIES)
            return fail(e, MSR_ERR_INVALID, "msr_merge_topk: n_parts=%d x k=%d needs %lld lists x %lld entries (both rounded up to "
                        "powers of two) = %lld > the limit of %d entries", n_parts, k, (long long)lists, (long long)entries,
                        (long long)(lists * entries), MSR_MERGE_MAX_ENTRIES);
    }
    if (n_queries == 0) return MSR_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, msr_merge_lists(score_bits, in_doc, in_score, in_n, in_payload, n_parts, part_stride_bytes, n_queries, k, out_doc,
                               out_score, out_n, out_payload, (hipStream_t)stream));
    return MSR_OK;
}

extern "C" int msr_merge_topk(msr_engine* e, const int32_t* in_doc, const void* in_score, const int32_t* in_n,
                              int32_t n_parts, int32_t n_queries, int32_t k, int32_t score_bits, int32_t* out_doc,
                              void* out_score, int32_t* out_n, void* stream) {
    return msr_merge_topk_payload(e, in_doc, in_score, in_n, nullptr, n_parts, 0, n_queries, k, score_bits, out_doc, out_score,
                                  out_n, nullptr, stream);
}

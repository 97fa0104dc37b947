/*
 * msretr.h -- C ABI of the MI355X-native two-stage retriever (libmsretr.so).
 *
 * The reference (StephenTaf/Modern-Search-Engines-Project) has no FFI / plugin interface: its query path
 * is three Python call sites.  Each entry point below replaces one of them and is what a binding for that
 * call site would bind (see INTEGRATION.md for the ctypes stubs):
 *
 *   msr_bm25_topk   <- BM25.search scoring loop + sort + cut      indexer/bm25_indexer.py:434-488
 *     (+ _within: the same restricted to document sets, e.g. a site: search; no reference counterpart)
 *   msr_dense_topk  <- Retriever.quick_search (dense full scan)   search_api.py:60,87 (retriever.py absent;
 *                      cosine reranker/reranker_api.py:285, per-doc max :370, report p.2)
 *   msr_rerank      <- /rerank endpoint arithmetic                reranker/reranker_api.py:27-63,273-334,357-372
 *   msr_merge_topk  <- (new) merge of per-shard top-k after the RCCL all-gather; no reference counterpart
 *   msr_bind_*      <- the per-query SQL fetches, done ONCE        bm25_indexer.py:413-448, reranker_api.py:36-61
 *
 * Conventions
 *   - Every function returns 0 on success or a negative msr_status; it never throws and never returns
 *     memory the caller has to free.  msr_last_error() gives the text of the last failure.
 *   - All array arguments are DEVICE pointers into HBM of the engine's device unless marked [host].
 *     The caller owns them (typically torch tensors: tensor.data_ptr()) and must keep the bound index
 *     arrays alive until msr_destroy / the next msr_bind_*.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).  Every kernel, copy and
 *     clear of a call is issued on that stream and on no other (it may be a non-blocking stream with work pending:
 *     inputs are read and scratch is cleared in stream order).  The QUERY calls only enqueue: they return while the
 *     work is pending, and results are valid once the stream has drained.  The calls that wait for the stream say so
 *     in their own comment -- the binds that check an index on the device (msr_bind_postings, msr_bind_chunks,
 *     msr_bind_tokens, msr_bind_vocab, msr_bind_facet), msr_gather_rows, msr_dense_topk_grouped, the diagnostics
 *     msr_debug_scratch_dirty, msr_dense_pass_info (the whole device) and msr_kernel_time_ms, and the offline index
 *     builds -- and no other call does.  msr_create returns with the engine's scratch cleared (it waits for the null
 *     stream once).  Calls that take `stream` and launch nothing (msr_bind_doc_meta, msr_bind_doc_domains,
 *     msr_bind_signatures) ignore it.  tests/stream_cases.py holds the table and tests/test_gpu_streams.py checks it
 *     on a stream with pending work.
 *   - A document is addressed by its dense index: the rank of its doc_id in ascending order, so
 *     "ascending index" == "ascending doc_id" (the reference's tie order, bm25_indexer.py:445,484).
 *     A shard adds `doc_base` to its local indices before the merge.
 *   - One engine per (device, stream); an engine is not thread-safe, distinct engines are independent.
 */
#ifndef MSRETR_H
#define MSRETR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSR_ABI_VERSION 16        /* 4: msr_unbind, msr_merge_postings; 5: msr_compact_postings; 6: msr_*_topk_within;
                                     7: msr_gather_rows, msr_dense_topk_grouped; 8: msr_bm25_score_docs, msr_union_candidates;
                                     9: msr_debug_bm25_split; 10: msr_debug_select, msr_merge_topk_payload refuses what its merge
                                     tree cannot hold (MSR_MERGE_MAX_ENTRIES); 11: msr_debug_exclusive_scan; 12: msr_term_sets;
                                     13: msr_bind_tokens, msr_phrase_sets, msr_combine_sets; 14: msr_proximity_sets;
                                     15: msr_best_windows; also 15 (calls added, none changed: a library
                                     that lacks them fails to load by symbol): msr_bind_vocab, msr_fuzzy_scratch_bytes,
                                     msr_fuzzy_terms; msr_debug_chunk_layout; msr_dense_pass_info;
                                     msr_wildcard_scratch_bytes, msr_wildcard_terms; msr_facet_table, msr_bind_facet,
                                     msr_facet_scratch_bytes, msr_facet_counts; msr_doc_signatures, msr_bind_signatures,
                                     msr_collapse_scratch_bytes, msr_collapse_duplicates;
                                     16: msr_debug_count_nonzero, msr_debug_scratch_dirty */
#define MSR_DIM 768               /* config.py:2 EMBEDDING_DIMENSION */
#define MSR_MAX_K 1024            /* config.py:13 TOP_K_RETRIEVAL = 1000 */
#define MSR_MAX_QUERY_TERMS 64
#define MSR_RERANK_MAX_CHUNKS 10  /* reranker_api.py:58 */
#define MSR_TERMSET_SPAN_DOCS 8192 /* msr_term_sets: consecutive documents one work item of its kernel owns (a multiple of 1024) */
#define MSR_PHRASE_MAX_TERMS 16    /* msr_phrase_sets / msr_proximity_sets: most term ids a row may hold */
#define MSR_PROX_MAX_SPAN 64       /* msr_proximity_sets / msr_best_windows: the widest window, in tokens */
#define MSR_SNIPPET_MAX_WEIGHT (1 << 20) /* msr_best_windows: the largest weight of a term (16 of them sum to 2^24 exactly) */
#define MSR_FUZZY_MAX_LEN 32       /* msr_fuzzy_terms: the longest word and the longest term, in code points */
#define MSR_FUZZY_MAX_WORDS 1024   /* msr_fuzzy_terms: most words of one call */
#define MSR_FUZZY_MAX_LIMIT 16     /* msr_fuzzy_terms: most candidates returned per word */
#define MSR_FUZZY_SPAN_TERMS 1024  /* msr_fuzzy_terms: consecutive vocabulary terms one workgroup of its first kernel owns */
#define MSR_FUZZY_WORD_GROUP 16    /* msr_fuzzy_terms: words that kernel stages in LDS at a time */
#define MSR_WILD_MAX_LEN 32        /* msr_wildcard_terms: the longest pattern, in symbols, and the longest term it matches */
#define MSR_WILD_MAX_PATTERNS 1024 /* msr_wildcard_terms: most patterns of one call */
#define MSR_WILD_MAX_LIMIT 16      /* msr_wildcard_terms: most matches returned per pattern */
#define MSR_FACET_MAX_LIMIT 64     /* msr_facet_counts: most facet values returned per row */
#define MSR_SIG_WORDS 64           /* msr_doc_signatures: 32-bit words of a document's min-hash signature */
#define MSR_SIG_MAX_SHINGLE 8      /* msr_doc_signatures: the widest shingle, in tokens */
#define MSR_COLLAPSE_MAX_CAND 1024 /* msr_collapse_duplicates: the longest fused list (config.py:13 TOP_K_RETRIEVAL = 1000) */
#define MSR_MERGE_MAX_ENTRIES 8192 /* msr_merge_topk(_payload): pow2ceil(n_parts) * max(64, pow2ceil(k)) may not exceed this */

typedef enum msr_status {
    MSR_OK = 0,
    MSR_ERR_INVALID = -1,    /* bad argument (null pointer, size out of range, wrong dim) */
    MSR_ERR_NOT_BOUND = -2,  /* the index part this call needs has not been bound */
    MSR_ERR_HIP = -3,        /* a HIP runtime call failed; text in msr_last_error */
    MSR_ERR_NOMEM = -4       /* scratch allocation failed */
} msr_status;

typedef struct msr_engine msr_engine;

typedef struct msr_config {
    int32_t struct_size;      /* sizeof(msr_config), for forward compatibility */
    int32_t device;           /* HIP device ordinal */
    int32_t dim;              /* must be MSR_DIM */
    int32_t max_queries;      /* queries processed per internal slice; scratch is sized for this many */
    int32_t max_k;            /* largest k any call will ask for, <= MSR_MAX_K */
    int32_t rerank_max_docs;  /* largest candidate list per query for msr_rerank, <= 1024 */
    int32_t scan_layout;      /* 0 = row-major embeddings; 1 = 16-row interleaved */
    int32_t scan_variant;     /* 0 = default: f16-split products when every row norm is in [0.5, 2], else exact f32;
                                 2 = always the exact-f32 MFMA kernel; 7 = f16-split on the 32-query kernel; 14 = the K-split kernel
                                 (what 0 resolves to on unit-norm rows); 15 = the K-split kernel over a pre-split f16 hi/lo copy of
                                 the rows (+4 bytes per value of HBM, ~4 % faster).  Any other value: msr_create fails */
    int32_t flags;            /* MSR_CFG_* bits; unknown bits: msr_create fails (ABI 3) */
} msr_config;

/* msr_config.flags */
#define MSR_CFG_NO_ROW_COPY 1 /* do not build the fragment-order copy of the embedding matrix (msr_bind_chunks): the 256-query
                                 pass then reads the caller's row-major matrix (same results bit for bit, ~13 % slower pass,
                                 half the embedding footprint); also declines the f16 image of the rows that launches of
                                 several query groups read (max_queries >= 512; msr_row_image_state) */
#define MSR_CFG_SINGLE_EMIT 2 /* the streaming pass of msr_dense_topk emits in ONE launch per query group, with thresholds from
                                 the sample pass alone, instead of cutting the emit pass into segments and raising the
                                 thresholds between them (same results bit for bit, more entries written and filtered: the
                                 reference form for tests and measurements; msr_dense_pass_info) */

/* BM25 parameters travel with the postings (bm25_indexer.py:57 k1=1.2, b=0.75). */
typedef struct msr_rerank_params {
    double smoothing;          /* reranker/config.yaml:28   0.15 */
    double max_boost;          /* reranker_api.py:317       0.10 */
    double max_decay;          /* reranker_api.py:318       0.05 */
    int32_t max_chunks;        /* reranker_api.py:58        10   */
    int32_t reserved;
} msr_rerank_params;

int msr_abi_version(void);
/* msr_create: allocates the engine's per-query scratch on cfg->device and clears the buffers documented "zero between
 * calls"; the clears are issued on the null stream and the call waits for them, so the first call on ANY stream -- a
 * non-blocking one included -- finds them done.  Not a hot path. */
int msr_create(const msr_config* cfg, msr_engine** out);
int msr_destroy(msr_engine* e);
/* e may be NULL: returns the text of the last failed msr_create on this thread. */
const char* msr_last_error(const msr_engine* e);

/* Stage-1 index: CSR postings over the dense doc index, sorted by doc inside each term.
 *   term_off[n_terms+1] i64, post_doc[n_postings] i32, post_tf[n_postings] i32   bm25_term_freq  (:97-104)
 *   doc_len[n_docs] i32                                                          bm25_doc_stats  (:88-94)
 *   idf[n_terms] f32 (as stored: REAL, may be negative)                          bm25_term_stats (:106-113)
 *   avgdl f32 (REAL)                                                             bm25_corpus_stats (:116-122)
 * The index is validated on the device and the term offsets are read on the host (the skip and dense tables of the long
 * lists are built from them): the call synchronises the stream, several times.  One-time, at bind.
 */
int msr_bind_postings(msr_engine* e, const int64_t* term_off, int64_t n_terms, const int32_t* post_doc,
                      const int32_t* post_tf, int64_t n_postings, const int32_t* doc_len, int64_t n_docs,
                      const float* idf, float avgdl, double k1, double b, void* stream);

/* Stage-2 index: chunk embeddings sorted by (doc index, chunk_id); doc d owns rows
 * [doc_off[d], doc_off[d+1]).  emb is f32 [n_chunks][768] row-major (scan_layout 0) or the interleaved
 * image produced by msr_interleave_rows (scan_layout 1).  inv_norm[n_chunks] f32 = 1/||row|| (0-norm -> 1),
 * or NULL to have the engine compute it.       indexer/embedder.py:31-52, indexer/indexer.py:165
 * Engine-owned memory this call allocates besides small tables: when cfg.max_queries >= 256 (and the corpus qualifies for
 * the streaming pass: row-major, documents of <= 256 chunks, >= 64 row tiles) a copy of the matrix in the order the
 * 256-query pass loads it, 1.03 x n_chunks x 3072 bytes; the caller's matrix stays bound and is what
 * every other kernel reads, so it must stay alive.  SURVEY 8b's "the handle owns only small scratch" is deliberately not
 * kept here: the copy is a trade of HBM for bandwidth, with a switch (MSR_CFG_NO_ROW_COPY) and a fallback (msr_row_copy_state).
 * When cfg.max_queries >= 512 (calls that put several 256-query groups into one launch: those launches are bound by the
 * matrix pipes, not by HBM) also an f16 image of the rows, (n_chunks + 512) x 1536 bytes: the values the 256-query pass
 * otherwise converts in registers, group after group -- the same products, the same results bit for bit.  Launches of ONE
 * group (<= 256 queries per call: the HBM-bound case) never read it; same switch, same fallback (msr_row_image_state).
 * The document offsets are read on the host (the spans and row tiles are cut there) and the range of the row norms picks the
 * scan's arithmetic: the call synchronises the stream.  One-time, at bind. */
int msr_bind_chunks(msr_engine* e, const float* emb, int64_t n_chunks, const int32_t* doc_off,
                    int64_t n_docs, const float* inv_norm, void* stream);
/* What became of that copy: 0 = not applicable (max_queries < 256 or the corpus does not qualify), 1 = built and used,
 * 2 = declined by MSR_CFG_NO_ROW_COPY, 3 = its allocation failed and the engine fell back to the row-major matrix (the bind
 * still succeeds).  -1: null handle. */
int msr_row_copy_state(const msr_engine* e);
/* The same for the f16 image of the rows that launches of several 256-query groups read: 0 = not applicable (max_queries < 512
 * or the corpus does not qualify), 1 = built and used, 2 = declined by MSR_CFG_NO_ROW_COPY, 3 = its allocation failed (those
 * launches then convert the f32 rows in registers as a single-group launch does).  -1: null handle. */
int msr_row_image_state(const msr_engine* e);
/* Device memory the handle owns right now, in bytes (scratch, tables built at bind, the copies above); the caller's bound
 * arrays are not included. */
int64_t msr_owned_bytes(const msr_engine* e);

/* Drop every binding: postings, chunks, document metadata and domain tables, the tables and copies built at bind, the scratch
 * sized by the corpus, and a pending msr_dense_topk_begin (its msr_dense_topk_end then fails).  Afterwards the engine is as
 * created: every query call returns MSR_ERR_NOT_BOUND, and the next msr_bind_postings / msr_bind_chunks pair may have any
 * n_docs (a larger corpus after an index update).  The caller makes sure no enqueued work still uses the old binding
 * (synchronise the stream first); the arrays it bound may be freed once this returns. */
int msr_unbind(msr_engine* e);

/* Per-document metadata the rerank stage needs: url_group[n_docs] i32 = id of the document's URL with
 * the query string removed, or -1 when the document is not in urlsDB.   reranker_api.py:38-47 */
int msr_bind_doc_meta(msr_engine* e, const int32_t* url_group, int64_t n_docs, void* stream);

/* Arithmetic of the bound dense scan's SWEEPS (calls of <= 64 queries, and the fallback): 0 = exact f32 MFMA (bit-for-bit
 * a k-ordered fmaf chain), 1 = f32 rows split into two f16 pieces, three f16 MFMAs per k-step with f32 accumulation
 * (|error| <= 8e-6 on the cosine for row norms in [0.5, 2], proof in DESIGN.md); -1 = no chunks bound.  When
 * msr_scan_width() says 128 or 256, calls of more than 64 queries take one streaming pass per 128 (256) queries instead:
 * an f16 filter with a measured margin, then EXACT f32 cosines for every returned document. */
int msr_scan_arith(const msr_engine* e);

/* Most queries one pass over the embedding matrix serves in msr_dense_topk: 256 / 128 when the streaming pass is available
 * (f16-split arithmetic bound, every document within one 256-row tile, enough tiles; 256 needs max_queries >= 256 and a
 * call of more than 128 queries), 64 when only the K-split kernel is (row-major layout, no per-document row limit, a
 * corpus that meets its preconditions; both arithmetics), else 32; -1 = no chunks bound. */
int msr_scan_width(const msr_engine* e);
/* Queries per pass over the matrix of the kernel the MOST RECENT msr_dense_topk call ran (256 / 128: the streaming pass;
 * 64 / 32: the sweeps -- also what a call takes whose k or max_chunks_per_doc the streaming pass does not serve); 0 before
 * the first call.  For whoever attributes a measured kernel time to a kernel (bench.py). */
int msr_dense_path(const msr_engine* e);
/* What the streaming pass of the MOST RECENT msr_dense_topk / msr_dense_topk_begin call did (its last slice of queries, when a
 * call is served in several): *segments = emit launches per query group -- 1: one launch over all row tiles (a small corpus,
 * or MSR_CFG_SINGLE_EMIT), 2: the pass was cut after the first T1 tiles and the emission thresholds raised to what their tile
 * maxima vouch for; 0: the call ran on the sweeps (then *entries = 0) --, *entries = (row, query, score) entries the pass
 * appended to its per-wave buffers, summed over the waves (counted past a buffer's capacity when one overflowed).  DIAGNOSTIC
 * and a DEVICE-WIDE WAIT: it takes no stream, waits for the whole device (hipDeviceSynchronize: every stream of every engine)
 * and copies the counters to the host with a blocking copy; it belongs in tests and measurements, never on a serving path. */
int msr_dense_pass_info(msr_engine* e, int32_t* segments, int64_t* entries);
/* The same for the <= 128-query sweeps of msr_dense_topk_bf16 (after msr_enable_bf16): 128, 64, or -1. */
int msr_batch_width(const msr_engine* e);
/* 1 if calls of msr_dense_topk_bf16 with more than 128 queries run as the tiled matrix-core GEMM (every document fits a
 * 256-row tile and the corpus has enough tiles), else 0 (such calls are served by repeated sweeps). */
int msr_batch_gemm_ok(const msr_engine* e);

/* Re-order row-major rows into the 16-row interleaved scan layout (dst may not alias src).
 * n_rows is padded up to a multiple of 16 in dst (pad rows zero): dst holds ceil16(n_rows)*768 floats. */
int msr_interleave_rows(msr_engine* e, const float* src, int64_t n_rows, float* dst, void* stream);

/* BM25 top-k for Q queries.  Query q owns q_terms/q_qtf[q_term_off[q] .. q_term_off[q+1]): its UNIQUE
 * term ids in first-occurrence order and how often each occurs in the query (bm25_indexer.py:405-409);
 * ids outside [0, n_terms) or with empty posting lists are skipped (:430).  Scores are float64 and
 * bit-identical to the reference's accumulation order (:466-478).  A document is a candidate only if at
 * least one posting touched it and score >= min_score (:461,480).  Output row q holds out_n[q] <= k
 * entries ordered by (score desc, doc index asc) (:484-485); the rest of the row is -1 / -inf. */
int msr_bm25_topk(msr_engine* e, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                  int32_t n_queries, int32_t k, double min_score, int32_t* out_doc, double* out_score,
                  int32_t* out_n, void* stream);

/* Document sets (restriction of a query to part of the corpus).  A set is a bitset of
 * uint32 words: document d is bit d & 31 of word d >> 5.  set_bits holds n_sets such rows, set_stride words apart
 * (set_stride >= ceil(n_docs / 32); bits at or above n_docs are ignored).  q_set[n_queries] (int32) picks query q's row;
 * -1 = unrestricted; any other value outside [0, n_sets) = the empty set (no row outside the n_sets rows is read).
 * n_sets == 0 is the unrestricted call (set_bits / q_set are not read).  Refused with MSR_ERR_INVALID, outputs untouched:
 * n_sets < 0; set_bits or q_set NULL while n_sets > 0; set_stride < ceil(n_docs / 32) while n_sets > 0.
 *
 * msr_bm25_topk_within: row q holds the first k entries, in msr_bm25_topk's order, of the documents of query q's set that
 *   msr_bm25_topk's rule accepts (touched by a posting, score >= min_score), with msr_bm25_topk's scores bit for bit: idf and
 *   avgdl stay those of the whole bound index (a set is not a sub-corpus).  out_n[q] may be below k; the rest of the row is
 *   -1 / -inf.  The set acts where the candidates are emitted (inside the scoring kernel), so the documents of the set
 *   ranked behind the whole corpus's top k are found.  Cost: that of msr_bm25_topk (one bit load per candidate). */
int msr_bm25_topk_within(msr_engine* e, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                         int32_t n_queries, int32_t k, double min_score,
                         const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* q_set,
                         int32_t* out_doc, double* out_score, int32_t* out_n, void* stream);

/* Document sets built from posting lists: the producer of the rows that the *_within calls and
 * msr_dense_topk_grouped consume.  Row r of out_bits (rows out_stride words apart, the layout above: document d is bit d & 31
 * of word d >> 5) becomes
 *     base(r)  AND  D(t) for every must term t of row r  AND NOT  D(t) for every not term t of row r
 * with D(t) the documents of term t's bound posting list; row r's must terms are must_terms[must_off[r] .. must_off[r + 1]),
 * its not terms not_terms[not_off[r] .. not_off[r + 1]) (int32 offsets from 0, n_rows + 1 of each; lists of any length --
 * this is not msr_bm25_topk's MSR_MAX_QUERY_TERMS plan).  Conventions:
 *   - a must term outside [0, n_terms), or with an empty list, makes the row empty;
 *   - a not term outside [0, n_terms), or with an empty list, is ignored;
 *   - repeated terms are allowed; a term in both lists makes the row empty; an empty must list means "all documents";
 *   - base(r) follows q_set's rules: row_base[r] == -1, or n_base == 0 (base_bits / row_base are then not read), is every
 *     document; a value in [0, n_base) picks that row of base_bits (n_base rows base_stride words apart); any other value is
 *     the empty set, and no row outside the n_base rows is read.
 * Every word [0, ceil(n_docs / 32)) of every row is written (the buffer need not be zeroed), bits at or above n_docs are 0,
 * words [ceil(n_docs / 32), out_stride) are not touched.  out_bits must not alias base_bits.  Repeated calls give the same
 * bytes.  The call only enqueues on `stream` (every array is a device pointer; the offsets are read on the device) and keeps
 * no scratch in the engine.  Refused with MSR_ERR_INVALID before any launch, outputs untouched: n_rows < 0; with n_rows > 0 a
 * NULL out_bits, must_off or not_off; out_stride < ceil(n_docs / 32); n_base < 0; with n_base > 0 a NULL base_bits or
 * row_base, or base_stride < ceil(n_docs / 32).  MSR_ERR_NOT_BOUND without postings.  n_rows == 0 succeeds and launches
 * nothing.  Cost: 4 bytes read per posting of every listed term (less what an already empty span of MSR_TERMSET_SPAN_DOCS
 * documents skips) plus the base rows, 4 ceil(n_docs / 32) bytes written per row. */
int msr_term_sets(msr_engine* e, int32_t n_rows, const int32_t* must_off, const int32_t* must_terms,
                  const int32_t* not_off, const int32_t* not_terms,
                  const uint32_t* base_bits, int32_t n_base, int64_t base_stride, const int32_t* row_base,
                  uint32_t* out_bits, int64_t out_stride, void* stream);

/* Phrase search.  The forward index is the token-id stream every document was indexed from:
 * tok_off int64 [n_docs + 1] and tok_ids int32 [n_tokens], document d's stream at tok_ids[tok_off[d] .. tok_off[d + 1]), in
 * the dense document order of the bound postings.
 *
 * msr_bind_tokens: device pointers, caller-owned; the engine keeps the pointers, as it does for the postings.  Checked once on
 *   the device (the call synchronises the stream), MSR_ERR_INVALID otherwise: tok_off[0] == 0, non-decreasing,
 *   tok_off[n_docs] == n_tokens; n_docs equals the bound postings' document count; every id in [0, n_terms) of the bound
 *   postings.  tok_ids may be NULL when n_tokens == 0.  MSR_ERR_NOT_BOUND without postings.  msr_unbind and
 *   msr_bind_postings drop the binding. */
int msr_bind_tokens(msr_engine* e, const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int64_t n_tokens,
                    void* stream);

/* msr_phrase_sets: row r of out_bits becomes { d in cand(r) : document d contains phrase r }, the phrase being
 *   phrase_terms[phrase_off[r] .. phrase_off[r + 1]) (int32 offsets from 0, n_rows + 1 of them).  Document d contains the
 *   phrase p[0 .. L) iff some i with 0 <= i <= len(d) - L has tok[d][i + j] == p[j] for every j: a match never crosses from
 *   one document into the next, a phrase longer than the document never matches, L == 1 is term containment.  A row whose
 *   phrase is empty, longer than MSR_PHRASE_MAX_TERMS, or holds an id outside [0, n_terms) is written EMPTY (by the kernel,
 *   no host round trip).  cand(r) follows q_set's and row_base's rules: row_cand[r] == -1, or n_cand == 0 (cand_bits /
 *   row_cand are then not read), is every document; a value in [0, n_cand) picks that row of cand_bits (rows cand_stride
 *   words apart); any other value is the empty set, and no row outside the n_cand rows is read.  Candidate bits at or above
 *   n_docs are ignored.  Layout and write contract as msr_term_sets: every word [0, ceil(n_docs / 32)) of every row is
 *   written, bits at or above n_docs are 0, words [ceil(n_docs / 32), out_stride) are not touched; out_bits must not alias
 *   cand_bits; repeated calls give the same bytes; the call only enqueues (offsets are read on the device), no engine
 *   scratch.  Refused before any launch, outputs untouched: MSR_ERR_NOT_BOUND without tokens; MSR_ERR_INVALID for
 *   n_rows < 0, with n_rows > 0 a NULL out_bits or phrase_off, out_stride < ceil(n_docs / 32), n_cand < 0, with n_cand > 0 a
 *   NULL cand_bits or row_cand or cand_stride < ceil(n_docs / 32).  n_rows == 0 succeeds and launches nothing.  Cost per
 *   row: 4 bytes per token of the candidate documents (less what a hit's early exit skips) plus 4 ceil(n_docs / 32) bytes
 *   read and written. */
int msr_phrase_sets(msr_engine* e, int32_t n_rows, const int32_t* phrase_off, const int32_t* phrase_terms,
                    const uint32_t* cand_bits, int32_t n_cand, int64_t cand_stride, const int32_t* row_cand,
                    uint32_t* out_bits, int64_t out_stride, void* stream);

/* Proximity search: words within a window of the forward index.  Row r is
 *   (p[0 .. L), span, ordered): p = phrase_terms[phrase_off[r] .. phrase_off[r + 1]) as in msr_phrase_sets, span = row_span[r],
 *   ordered = row_ordered[r] != 0 (int32 [n_rows] each), with 1 <= L <= MSR_PHRASE_MAX_TERMS and 1 <= span <=
 *   MSR_PROX_MAX_SPAN.  Row r of out_bits becomes { d in cand(r) : document d matches row r }, document d being the sequence
 *   tok[d][0 .. len).
 *   ORDERED: d matches iff there are positions i_0 < i_1 < ... < i_{L-1} inside d with tok[d][i_j] == p[j] for every j and
 *   i_{L-1} - i_0 + 1 <= span.  A repeated id needs as many different positions; span == L is exactly msr_phrase_sets'
 *   phrase; span < L matches nothing.
 *   ANY ORDER: let T be the set of distinct ids of p; d matches iff there is one position per id of T, all inside d, with
 *   max - min + 1 <= span.  A repeated id counts once; |T| == 1 is term containment; span < |T| matches nothing.
 *   BOTH: positions never leave the document (a match never uses tokens of two documents); an empty document matches
 *   nothing.  A row with L < 1, L > MSR_PHRASE_MAX_TERMS, an id outside [0, n_terms), span < 1 or span > MSR_PROX_MAX_SPAN is
 *   written EMPTY (by the kernel, no host round trip).  cand(r) follows the row_cand / n_cand rules of msr_phrase_sets.
 *   Layout and write contract as msr_term_sets / msr_phrase_sets: every word [0, ceil(n_docs / 32)) of every row is written,
 *   bits at or above n_docs are 0, words [ceil(n_docs / 32), out_stride) are not touched; repeated calls give the same bytes;
 *   the call only enqueues (offsets, spans and modes are read on the device), no engine scratch; out_bits must not alias
 *   cand_bits.  Refused before any launch, outputs untouched: MSR_ERR_NOT_BOUND without tokens; MSR_ERR_INVALID for what
 *   msr_phrase_sets refuses, and for a NULL row_span or row_ordered with n_rows > 0.  n_rows == 0 succeeds and launches
 *   nothing.  Cost per row: as msr_phrase_sets (every token of a candidate document is read once, 4 bytes, until the first
 *   match). */
int msr_proximity_sets(msr_engine* e, int32_t n_rows, const int32_t* phrase_off, const int32_t* phrase_terms,
                       const int32_t* row_span, const int32_t* row_ordered,
                       const uint32_t* cand_bits, int32_t n_cand, int64_t cand_stride, const int32_t* row_cand,
                       uint32_t* out_bits, int64_t out_stride, void* stream);

/* Query-biased snippets: the best window of a document for a weighted list of terms.
 *   ROW r is (p[0 .. L), w[0 .. L), span): p = row_terms[row_off[r] .. row_off[r + 1]), w = row_weights[same range],
 *   span = row_span[r] (row_off int32 [n_rows + 1], row_span int32 [n_rows]), with 1 <= L <= MSR_PHRASE_MAX_TERMS,
 *   0 <= w[j] <= MSR_SNIPPET_MAX_WEIGHT and 1 <= span <= MSR_PROX_MAX_SPAN.  A repeated id counts once, with the weight and
 *   the bit of its first occurrence.
 *   PAIR i is (pair_doc[i], pair_row[i]).  Let s = tok[d][0 .. n) be the document's own stream (n < 2^31).  For every start a
 *   in [0, n) the window is s[a .. min(a + span, n)); hits(a) = the number of positions of the window whose token is a term of
 *   the row; cover(a) = the sum of w[j] over the DISTINCT ids present in the window.  The pair's answer is the start with the
 *   largest (cover, hits), compared lexicographically; among equal ones the SMALLEST a.  If no position of the document
 *   holds a term of the row (an empty document included) the pair has no window.  Entry i of the five outputs:
 *     out_start int32   the position inside the document, or -1
 *     out_cover int32   cover(start)
 *     out_hits  int32   hits(start)
 *     out_mask  uint64  bit k = the token at start + k is a term of the row; bits at or above the window's length are 0
 *     out_terms uint32  bit j = p[j] stands in the window; a repeated id sets only the bit of its first occurrence
 *   NO WINDOW is (-1, 0, 0, 0, 0).  The kernel writes the same five values, without a host round trip, for a pair_doc outside
 *   [0, n_docs), a pair_row outside [0, n_rows), and a row with L < 1, L > MSR_PHRASE_MAX_TERMS, an id outside [0, n_terms),
 *   a weight outside [0, MSR_SNIPPET_MAX_WEIGHT] or a span outside 1 .. MSR_PROX_MAX_SPAN.  A window never uses a token of a
 *   neighbouring document: the bound of every read is the document's end.  All arithmetic is integer.
 *   All pointers are device pointers.  The call only enqueues (one launch, one wave per pair) and uses no engine scratch;
 *   repeated calls give the same bytes; entries at or above n_pairs are not touched.  Refused before any launch, outputs
 *   untouched: MSR_ERR_NOT_BOUND without tokens (msr_bind_tokens); MSR_ERR_INVALID for a NULL pointer with n_pairs > 0, a
 *   negative count, or n_rows == 0 with n_pairs > 0.  n_pairs == 0 succeeds and launches nothing.  Cost per pair: every token
 *   of the document is read once, 4 bytes; there is no early exit. */
int msr_best_windows(msr_engine* e, int32_t n_pairs, const int32_t* pair_doc, const int32_t* pair_row,
                     int32_t n_rows, const int32_t* row_off, const int32_t* row_terms, const int32_t* row_weights,
                     const int32_t* row_span, int32_t* out_start, int32_t* out_cover, int32_t* out_hits, uint64_t* out_mask,
                     uint32_t* out_terms, void* stream);

/* Typo-tolerant lookup: the vocabulary terms nearest to a word.
 *   DISTANCE d(w, t): optimal string alignment (restricted Damerau-Levenshtein) over 16-bit code points: an insertion, a
 *   deletion, a substitution and a swap of two ADJACENT code points cost 1 each, and no substring is edited twice:
 *   d("ca", "abc") = 3, d("ab", "ba") = 1.
 *   CANDIDATES of word w with tolerance m in {0, 1, 2}: the terms t with weight[t] > 0, at most MSR_FUZZY_MAX_LEN code points
 *   and d(w, t) <= m, ORDERED by distance ascending, then weight descending, then term id ascending (a total order).
 *
 * msr_bind_vocab: term t's code points are chars[char_off[t] .. char_off[t + 1]) (char_off int64 [n_terms + 1], chars uint16
 *   [n_chars], weight uint32 [n_terms]).  Device pointers, caller-owned; the engine keeps the pointers, as it does for the
 *   tokens.  Checked once on the device (the call synchronises the stream), MSR_ERR_INVALID otherwise: char_off[0] == 0,
 *   non-decreasing, char_off[n_terms] == n_chars; every weight below 2^31; n_terms equal to the bound postings' term count.
 *   chars may be NULL when n_chars == 0.  MSR_ERR_NOT_BOUND without postings.  The call builds one table of 8 bytes per term
 *   (a 64-bit signature of the term's character set, the lookup's filter), owned by the engine, counted by msr_owned_bytes
 *   and released, with the binding, by msr_unbind and msr_bind_postings.  A failed call leaves no vocabulary bound.
 *
 * msr_fuzzy_scratch_bytes: bytes of scratch one msr_fuzzy_terms call over a vocabulary of n_terms terms needs for n_words
 *   words and `limit` candidates (-1 for arguments the call would refuse; 0 for n_words == 0).  The caller supplies the
 *   scratch (8-byte aligned); the engine keeps none.
 *
 * msr_fuzzy_terms: word i's code points are word_chars[word_off[i] .. word_off[i + 1]) (int32 offsets), its tolerance
 *   word_max[i].  Row i of out_term / out_dist (int32 [n_words][limit]) receives the first out_n[i] = min(out_total[i], limit)
 *   candidates in the order above (term id, distance), the remaining slots of the row -1; out_total[i] = the number of ALL
 *   candidates.  The kernel itself writes the row empty (out_n = out_total = 0, every slot -1) for a word of length 0 or of
 *   more than MSR_FUZZY_MAX_LEN code points and for a tolerance outside {0, 1, 2}.  All pointers are device pointers.  The
 *   call only enqueues (two launches); repeated calls give the same bytes (no atomics); nothing is written at or beyond row
 *   n_words.  Refused before any launch, outputs untouched: MSR_ERR_NOT_BOUND without a vocabulary; MSR_ERR_INVALID for
 *   n_words < 0 or > MSR_FUZZY_MAX_WORDS, limit outside [1, MSR_FUZZY_MAX_LIMIT], and with n_words > 0 a NULL pointer, a
 *   scratch that is not 8-byte aligned or scratch_bytes < msr_fuzzy_scratch_bytes(n_terms, n_words, limit).  n_words == 0
 *   succeeds and launches nothing. */
int msr_bind_vocab(msr_engine* e, const int64_t* char_off, const uint16_t* chars, const uint32_t* weight, int64_t n_terms,
                   int64_t n_chars, void* stream);
int64_t msr_fuzzy_scratch_bytes(int64_t n_terms, int32_t n_words, int32_t limit);
int msr_fuzzy_terms(msr_engine* e, int32_t n_words, const int32_t* word_off, const uint16_t* word_chars, const int32_t* word_max,
                    int32_t limit, int32_t* out_term, int32_t* out_dist, int32_t* out_n, int32_t* out_total, void* scratch,
                    int64_t scratch_bytes, void* stream);

/* Prefix and wildcard lookup: the vocabulary terms a pattern matches, over the vocabulary bound
 * with msr_bind_vocab.
 *   PATTERN: 1 .. MSR_WILD_MAX_LEN symbols, each a 16-bit code point.  `*` (0x002A) matches any run of zero or more code points,
 *   `?` (0x003F) exactly one; every other symbol matches itself.  There is no escape: a term that itself holds 0x2A or 0x3F is
 *   matched only through a metacharacter.  The match is anchored at both ends (the whole term must match); `**` means `*`; a
 *   pattern without a metacharacter is an exact lookup.
 *   MATCHES of pattern p: the terms t with weight[t] > 0, at most MSR_WILD_MAX_LEN code points and match(p, t), ORDERED by
 *   weight descending, then term id ascending (a total order).
 *
 * msr_wildcard_scratch_bytes: bytes of scratch one msr_wildcard_terms call over a vocabulary of n_terms terms needs for
 *   n_patterns patterns and `limit` matches (-1 for arguments the call would refuse; 0 for n_patterns == 0): the formula of
 *   msr_fuzzy_scratch_bytes, n_patterns * ceil(n_terms / 1024) * (8 * limit + 4).  The caller supplies the scratch (8-byte
 *   aligned); the engine keeps none.
 *
 * msr_wildcard_terms: pattern i's symbols are pat_chars[pat_off[i] .. pat_off[i + 1]) (int32 offsets).  Row i of out_term
 *   (int32 [n_patterns][limit]) receives the first out_n[i] = min(out_total[i], limit) matches in the order above, the
 *   remaining slots of the row -1; out_total[i] = the number of ALL matches.  The kernel itself writes the row empty (out_n =
 *   out_total = 0, every slot -1) for a pattern of 0 or of more than MSR_WILD_MAX_LEN symbols.  All pointers are device
 *   pointers.  The call only enqueues (two launches); repeated calls give the same bytes (no atomics); nothing is written at
 *   or beyond row n_patterns.  Refused before any launch, outputs untouched: MSR_ERR_NOT_BOUND without a vocabulary;
 *   MSR_ERR_INVALID for n_patterns < 0 or > MSR_WILD_MAX_PATTERNS, limit outside [1, MSR_WILD_MAX_LIMIT], and with
 *   n_patterns > 0 a NULL pointer, a scratch that is not 8-byte aligned or scratch_bytes <
 *   msr_wildcard_scratch_bytes(n_terms, n_patterns, limit).  n_patterns == 0 succeeds and launches nothing. */
int64_t msr_wildcard_scratch_bytes(int64_t n_terms, int32_t n_patterns, int32_t limit);
int msr_wildcard_terms(msr_engine* e, int32_t n_patterns, const int32_t* pat_off, const uint16_t* pat_chars, int32_t limit,
                       int32_t* out_term, int32_t* out_n, int32_t* out_total, void* scratch, int64_t scratch_bytes, void* stream);

/* Facet counts: how many documents of a query's WHOLE match set carry each facet value, and how many
 * match at all.  A facet is one int32 value per document: value[d] in [0, n_values), or -1 for "none".  For row r
 *     M(r) = base(r)  AND  (OR of D(t) for t in any_terms[any_off[r] .. any_off[r + 1]))
 *     hits[r] = |M(r)|,   count[r][v] = |{d in M(r) : value[d] == v}|
 * with D(t) and base(r) exactly msr_term_sets': a term outside [0, n_terms) or with an empty list contributes nothing, repeated
 * terms are allowed, an EMPTY list is no term condition (M = base); row_base[r] == -1 or n_base == 0 is every document, a row
 * index picks that row, anything else is empty; bits at or above n_docs never count.  Documents with value -1 are counted in
 * hits only, so sum_v count[r][v] <= hits[r].  The top list of a row holds the values with count > 0 in (count desc, value asc)
 * order, the first `limit` of them; n_values_hit[r] is the number of values with count > 0.
 *
 * msr_facet_table (host; no device is touched): the table the kernels need.  With S = MSR_TERMSET_SPAN_DOCS, for each span s of
 *   S consecutive documents span_values[span_off[s] .. span_off[s + 1]) holds the distinct values of the span, strictly
 *   ascending; local[d] is the position of value[d] in its span's list (at most S - 1; 0xFFFF for value -1); for every value v
 *   value_pos[value_off[v] .. value_off[v + 1]) holds the positions in span_values that hold v, ascending.  Sizes: local
 *   [n_docs], span_off [ceil(n_docs / S) + 1], span_values and value_pos [T], value_off [n_values + 1].  Returns T =
 *   span_off[n_spans] <= n_docs; a negative number for a value outside [-1, n_values) or a NULL pointer.  Called with local ==
 *   NULL it only counts and returns T (the other outputs are not touched): the caller sizes the arrays with that.
 *
 * msr_bind_facet: device pointers, caller-owned, borrowed like the forward index; local must be 16-byte aligned.  The table is
 *   checked once on the device (the call synchronises the stream), MSR_ERR_INVALID unless: n_docs equals the bound postings'
 *   count; span_off[0] == 0, span_off is non-decreasing and each span has at most S entries; every local[d] is below its span's
 *   entry count or equals 0xFFFF; span_values is in [0, n_values) and strictly ascending within a span; value_off[0] == 0,
 *   value_off is non-decreasing and value_off[n_values] == T = span_off[n_spans]; value_pos is strictly ascending within a value
 *   and span_values[value_pos[i]] == v for every i of value v (together: value_pos is a bijection).  A refused table leaves the
 *   previous binding in place.  MSR_ERR_NOT_BOUND without postings.  msr_unbind and msr_bind_postings drop the binding; all
 *   five pointers NULL unbinds.
 *
 * msr_facet_scratch_bytes: bytes of scratch one msr_facet_counts call of n_rows rows needs: per row 2 T rounded up to 16, plus
 *   4 per span.  Negative (MSR_ERR_INVALID / MSR_ERR_NOT_BOUND) for n_rows < 0 / without a bound table.
 *
 * msr_facet_counts: every array is a device pointer; the call only enqueues on `stream` (two kernels, no global atomic, no
 *   memset); no output has to be zeroed beforehand; repeated calls give the same bytes.  out_hits / out_n_values_hit [n_rows];
 *   out_top_value / out_top_count [n_rows][limit], the rest of a row -1 / 0; out_counts (nullable) [n_rows][count_stride]:
 *   every element [0, n_values) of every row is written, elements past n_values are left untouched.  Refused with
 *   MSR_ERR_INVALID before any launch, outputs untouched: n_rows < 0; limit outside [0, MSR_FACET_MAX_LIMIT]; with n_rows > 0 a
 *   NULL any_off, out_hits or out_n_values_hit; NULL top arrays with limit > 0; count_stride < n_values with out_counts given;
 *   scratch_bytes below msr_facet_scratch_bytes(e, n_rows), or a scratch that is NULL or not 16-byte aligned when bytes are
 *   needed; msr_term_sets' refusals of the base arguments.  MSR_ERR_NOT_BOUND without postings or without a facet table.
 *   n_rows == 0 succeeds and launches nothing.  Cost per row: 4 bytes per posting of the listed terms, 2 bytes per document of a
 *   non-empty word of M(r), the base row, and 2 T bytes written and read again. */
int64_t msr_facet_table(const int32_t* value, int64_t n_docs, int32_t n_values, uint16_t* local, int32_t* span_off,
                        int32_t* span_values, int32_t* value_off, int32_t* value_pos);
int msr_bind_facet(msr_engine* e, const uint16_t* local, const int32_t* span_off, const int32_t* span_values,
                   const int32_t* value_off, const int32_t* value_pos, int64_t n_docs, int32_t n_values, void* stream);
int64_t msr_facet_scratch_bytes(const msr_engine* e, int32_t n_rows);
int msr_facet_counts(msr_engine* e, int32_t n_rows, const int32_t* any_off, const int32_t* any_terms,
                     const uint32_t* base_bits, int32_t n_base, int64_t base_stride, const int32_t* row_base,
                     int32_t limit, int32_t* out_hits, int32_t* out_n_values_hit,
                     int32_t* out_top_value, int32_t* out_top_count,   /* [n_rows][limit]; rest of a row -1 / 0 */
                     int32_t* out_counts, int64_t count_stride,        /* nullable: all counts, [n_rows][count_stride] */
                     void* scratch, int64_t scratch_bytes, void* stream);

/* msr_combine_sets: out[r] = AND of in[s] for s in and_rows[and_off[r] .. and_off[r + 1])  AND NOT  OR of in[s] for s in
 *   not_rows[not_off[r] .. not_off[r + 1]), rows of in_bits (n_in rows in_stride words apart) in the layout above.  An empty
 *   AND list means every document below n_docs; a row index outside [0, n_in) empties the row in the AND list and is ignored
 *   in the NOT list (no row outside the n_in rows is read).  Input bits at or above n_docs are ignored.  The write contract
 *   of msr_term_sets; out_bits must not alias in_bits; one elementwise kernel, only enqueued.  Refused with MSR_ERR_INVALID
 *   before any launch, outputs untouched: n_rows < 0; with n_rows > 0 a NULL out_bits, and_off or not_off; out_stride <
 *   ceil(n_docs / 32); n_in < 0; with n_in > 0 a NULL in_bits or in_stride < ceil(n_docs / 32).  MSR_ERR_NOT_BOUND without
 *   postings (they give n_docs).  n_rows == 0 succeeds and launches nothing. */
int msr_combine_sets(msr_engine* e, int32_t n_rows, const int32_t* and_off, const int32_t* and_rows,
                     const int32_t* not_off, const int32_t* not_rows,
                     const uint32_t* in_bits, int32_t n_in, int64_t in_stride,
                     uint32_t* out_bits, int64_t out_stride, void* stream);

/* Read-only, launches nothing: how msr_bm25_topk(_within) splits the work of ONE internal slice of n_queries queries
 * (1 <= n_queries <= max_queries; a call of more queries runs slices of max_queries and one of the rest) over the bound
 * postings.  *tiles_per_item = consecutive 1024-document tiles one wave of the scoring kernel walks (1, 2, 4 or 8);
 * *n_segments = ceil(tiles / *tiles_per_item) = work items per query = segments of a query's candidate row that the select
 * walks.  Results never depend on the split; the export exists so that tests can ASSERT which split a call ran instead of
 * assuming it.  MSR_ERR_NOT_BOUND without postings, MSR_ERR_INVALID for n_queries out of range or a NULL output. */
int msr_debug_bm25_split(msr_engine* e, int32_t n_queries, int32_t* tiles_per_item, int32_t* n_segments);

/* Test-only: the engine's own exact top-k select (its scratch, its kernels: what every *_topk entry point ends in) over RAW
 * score rows of the caller, so that tests can steer it by the bit patterns of the scores.  Only enqueues; every array is a
 * device pointer.  mode:
 *   MSR_SELECT_F32         scores float  [n_queries][stride], row q = elements 0 .. n-1, element i = document i
 *   MSR_SELECT_F64         the same over double rows
 *   MSR_SELECT_F32_WITHIN  MSR_SELECT_F32 with query q restricted to set q_set[q] of set_bits [n_sets][set_stride] (bit d & 31
 *                          of word d >> 5; q_set -1 = every document, any other value outside [0, n_sets) = none)
 *   MSR_SELECT_F64_LIST    scores double / idx int32 [n_queries][stride]: row q is cut into n_seg segments seg_stride elements
 *                          apart, segment s holds counts[q * n_seg + s] pairs (score, document idx) in any order from its first
 *                          position on (n is ignored).  win_base (nullable, [n_queries]): the first pass bins the 20-bit key
 *                          prefixes win_base[q] .. win_base[q] + 4095, both ends clamped (what msr_bm25_topk does with a bound
 *                          derived from the query); the result never depends on it.
 * Arguments a mode does not use are ignored.  gate (nullable): device word(s); where the word is 0 every kernel returns at once
 * and the outputs (and out_state) of those queries are left as they were: gate_per64 = 0: gate[0] decides for all queries, else
 * gate[q / 64] for query q.
 * Result, rows of k: the k best VALID elements in the order (score descending, document ascending), out_n[q] = min(k, valid
 * elements), (-1, -inf) behind it.  Valid: not NaN and not -inf; +inf is valid.  Scores come back bit for bit, except that
 * -0.0 and +0.0 are ONE key: both order by document alone among themselves and come back as +0.0.
 * out_state (nullable, [n_queries]): the select's per-query state after its streaming passes, before the final kernel (which
 * does not write it back): done = 1: the candidates at or above the resolved prefix were compacted (n_above + the tie bin's
 * members <= 4096, or fewer valid elements than k -- then n_sel < k is their number); done = 0: more than 4096 elements share
 * the resolved prefix (or a window pass ended in a clamped bin: mask_hi = 0) and the final kernel resolves the remaining digits
 * over the row itself.  mask_hi / mask_lo: the key bits resolved (score part / ~document part), pref_*: their values; n_above:
 * elements strictly above the prefix; k_rem = k - n_above.
 * Refused with MSR_ERR_INVALID before any launch: mode unknown; n_queries outside [1, max_queries]; k outside [1, max_k];
 * scores or an output NULL; n < 0, n >= 2^31 or stride < n; list mode: idx or counts NULL, n_seg < 1, seg_stride < 0 or
 * n_seg * seg_stride > stride; within mode: n_sets < 1, set_bits or q_set NULL, set_stride < ceil(n / 32). */
enum { MSR_SELECT_F32 = 0, MSR_SELECT_F64 = 1, MSR_SELECT_F32_WITHIN = 2, MSR_SELECT_F64_LIST = 3 };
typedef struct msr_select_state {
    uint64_t pref_hi, mask_hi;
    uint32_t pref_lo, mask_lo;
    int32_t k_rem, n_above, done, n_sel;
} msr_select_state;
int msr_debug_select(msr_engine* e, int32_t mode, const void* scores, int64_t n, int64_t stride, int32_t n_queries, int32_t k,
                     const int32_t* idx, const int32_t* counts, int32_t n_seg, int64_t seg_stride, const uint64_t* win_base,
                     const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* q_set, const int32_t* gate,
                     int32_t gate_per64, int32_t* out_doc, void* out_score, int32_t* out_n, msr_select_state* out_state,
                     void* stream);

/* Test-only: *out (device pointer to ONE int64) <- the number of non-zero 32-bit words among dev[0 .. n_words) (device pointer,
 * 4-byte aligned).  A word counts by its BITS: -0.0f (0x80000000) and a NaN are non-zero.  Handle-less like
 * msr_debug_exclusive_scan, so that the counter itself can be tested on a caller's buffers; unlike it, it allocates nothing and
 * only enqueues (a clear of *out, then one kernel: plain loads of the counted words, a reduction per workgroup, one integer
 * add per workgroup into *out -- the counted buffer is never written and no atomic touches it).  n_words = 0: *out <- 0, dev
 * may be NULL.  MSR_ERR_INVALID for n_words < 0, a NULL out, or n_words > 0 with a NULL or misaligned dev (text in
 * msr_last_error(NULL)). */
int msr_debug_count_nonzero(const void* dev, int64_t n_words, int64_t* out, void* stream);

/* Test-only: a direct view of the state an engine call must leave behind for the next one.  Some engine buffers are documented
 * "zero between calls": every kernel that counts into them puts the zero back on every exit, so that no call has to clear them
 * first.  out (HOST pointer, n_out >= MSR_DIRTY_SLOTS entries, entries past MSR_DIRTY_SLOTS are not written): out[slot] <- the
 * number of non-zero 32-bit words (msr_debug_count_nonzero) over the buffer's WHOLE allocated extent -- not the rows of the
 * last call -- or -1 for a buffer that is not allocated (no chunks bound, the streaming pass or the bf16 path not built):
 *   MSR_DIRTY_SEL_HIST        the select's histograms, max(max_queries, 128) x 4096 words
 *   MSR_DIRTY_SEL_CAND_N      the select's candidate counts, max(max_queries, 128) words (the bind checks borrow words 0 and 1)
 *   MSR_DIRTY_GEMM_PAIR_N     pair counts of the bf16 GEMM path (msr_enable_bf16 on a corpus with row tiles)
 *   MSR_DIRTY_F32_PAIR_N      pair counts of the f32 streaming pass (65 queries and up; 128 x its query groups)
 *   MSR_DIRTY_F32_CAND_N      candidate counts of the same pass
 *   MSR_DIRTY_BT_CAND_N       candidate counts of the batched bf16 path (allocated by the first msr_enable_bf16, kept by rebinds)
 *   MSR_DIRTY_SPLIT_PENDING   not a count: the queries of an msr_dense_topk_begin whose msr_dense_topk_end has not come (0: none)
 * Every count is 0 after every call that returned, whatever it returned; a test asserts that after each call it makes.
 * Buffers that each user clears on entry instead (the gate words of the streaming pass, the flag word of the bind checks) and
 * buffers that every call rewrites before reading (score rows, candidate rows, the BM25 plan) carry no invariant and have no slot.
 * SYNCHRONISES the stream (the counts come back to the host) -- no other msr_debug_* call with a handle does; it reads device
 * memory only, so calling it between an msr_dense_topk_begin and its end is allowed.  MSR_ERR_INVALID for a NULL out or
 * n_out < MSR_DIRTY_SLOTS. */
enum { MSR_DIRTY_SEL_HIST = 0, MSR_DIRTY_SEL_CAND_N = 1, MSR_DIRTY_GEMM_PAIR_N = 2, MSR_DIRTY_F32_PAIR_N = 3,
       MSR_DIRTY_F32_CAND_N = 4, MSR_DIRTY_BT_CAND_N = 5, MSR_DIRTY_SPLIT_PENDING = 6, MSR_DIRTY_SLOTS = 7 };
int msr_debug_scratch_dirty(msr_engine* e, int64_t* out, int32_t n_out, void* stream);

/* Hybrid candidates (dense hits join the BM25 list).
 *   msr_bm25_score_docs: the BM25 scores of NAMED documents -- a point lookup, no posting list is streamed.  Queries packed as
 *     for msr_bm25_topk (unique term ids in first-occurrence order, <= 64 per query).  doc is [n_queries][max_docs] document
 *     indices, doc_n[q] of row q valid (doc_n NULL: all max_docs; a value outside [0, max_docs] is clamped).  For a valid
 *     slot naming document d: out_score = the float64 sum the reference forms for d (bm25_indexer.py:466-478): the
 *     contributions (idf * tf_component) * qtf of the query's valid terms that d contains, added in the query's order from
 *     0.0 -- bit for bit the score msr_bm25_topk returns for (query, d); out_touched = 1 if d contains at least one of them
 *     (msr_bm25_topk's "touched by a posting"), else 0 with score 0.0.  No min_score: a negative sum is returned as it is.
 *     A slot past doc_n[q], or holding an index outside [0, n_docs), gets 0.0 / 0 and reads nothing of the index.  A document
 *     may repeat in a row (equal results).  Reads only what msr_bind_postings built (postings with tf_components, skip table,
 *     dense tables): no engine scratch, no state, valid after any re-bind.  Cost: per (slot, term) one table load, or a
 *     binary search of <= 11 dependent loads; ~25 600 slots in a few tens of microseconds.
 *     Refused with MSR_ERR_INVALID: n_queries < 0, max_docs < 0, a NULL array that would be read or written.
 *   msr_union_candidates: row q of the output = the lexical list lex_doc / lex_score [n_queries][k_lex] (lex_n[q] entries)
 *     unchanged and in its order, followed by the documents of dense_doc [n_queries][k_dense] (dense_n[q] entries) that the
 *     lexical list does not hold, in dense rank order, each with its score dense_bm25[q][j] (from msr_bm25_score_docs).
 *     Entries of the dense list that are negative, or repeat an earlier entry of it, are skipped.  out_src[q][m]: 1 = the
 *     lexical list only, 2 = the dense list only, 3 = both.  out_n[q] <= k_lex + k_dense; the rest of a row (max_cand columns)
 *     is -1 / -inf / 0.  The output is what msr_rerank_gather / msr_rerank_fuse take as cand_doc / cand_bm25 / cand_n.
 *     Counts outside [0, k] are clamped.  Refused with MSR_ERR_INVALID, outputs untouched: k_lex or k_dense outside
 *     [0, MSR_MAX_K]; k_lex + k_dense > max_cand; max_cand < 1; a NULL array that would be read or written. */
int msr_bm25_score_docs(msr_engine* e, const int32_t* q_term_off, const int32_t* q_terms, const int32_t* q_qtf,
                        int32_t n_queries, const int32_t* doc, const int32_t* doc_n, int32_t max_docs,
                        double* out_score, int32_t* out_touched, void* stream);
int msr_union_candidates(msr_engine* e, int32_t n_queries,
                         const int32_t* lex_doc, const double* lex_score, const int32_t* lex_n, int32_t k_lex,
                         const int32_t* dense_doc, const double* dense_bm25, const int32_t* dense_n, int32_t k_dense,
                         int32_t* out_doc, double* out_score, int32_t* out_src, int32_t* out_n, int32_t max_cand,
                         void* stream);

/* Dense full scan for Q queries: score(d) = max over the document's first `max_chunks_per_doc` chunks
 * (0 = all) of cosine(q, chunk), cosine as sklearn computes it in float32 (reranker_api.py:285), to within the
 * 1e-5 tolerance of the task (see msr_scan_arith for the arithmetic actually used).
 * q is [n_queries][768] f32, NOT normalised (reranker_api.py:355).  Output rows as for msr_bm25_topk,
 * with float32 scores and out_chunk = row index of the arg-max chunk (first maximum). */
int msr_dense_topk(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t max_chunks_per_doc,
                   int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_n, void* stream);

/* msr_dense_topk restricted to document sets (encoding and refusals: msr_bm25_topk_within).  Every query of a restricted call
 * runs on the SWEEPS -- the kernels an unrestricted call of <= 64 queries runs (K-split 64 / narrow 32 queries per pass over
 * the matrix, msr_scan_arith's arithmetic, msr_dense_path() = 64 or 32) --, whatever n_queries: not the 256-query streaming
 * pass, so the scores are the sweep's (|error| <= 8e-6 with the f16-split products), not exact-f32 rescored ones.  Row q is the
 * top k of query q's set by the per-document maximum cosine, same order, ties, chunk rows and max_chunks_per_doc as
 * msr_dense_topk; documents outside the set never enter the select.  A cosine does not depend on other documents: with the
 * same sweep kernel the result equals msr_dense_topk over the index without the documents outside the set, bit for bit.
 * Cost: one sweep per 64 queries (~4.5 x the per-query cost of the 256-query pass at 5 M chunks). */
int msr_dense_topk_within(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t max_chunks_per_doc,
                          const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* q_set,
                          int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_n, void* stream);

/* Documents similar to documents ("pages like this one", near-duplicate checks).
 *   msr_gather_rows: out[i][0..768) <- chunk row rows[i] as given to msr_bind_chunks (f32, NOT normalised), bit for bit,
 *     whatever layout the engine holds (row-major, or the 16-row interleaved image of scan_layout 1).  A row outside
 *     [0, n_chunks) is refused (MSR_ERR_INVALID, out untouched): checked on the device, so the call synchronises the stream.
 *   msr_dense_topk_grouped: q [n_rows][768] query rows (typically gathered source rows), cut into n_groups groups by the CSR
 *     group_off [n_groups + 1] (group g = rows [group_off[g], group_off[g + 1])); excl_off [n_groups + 1] / excl_doc: per group
 *     the documents never returned (typically the sources themselves).  For group g and a document d not excluded,
 *       S_g(d) = max over the rows r of g of score_r(d),
 *     score_r(d) the f32 score msr_dense_topk returns for query row r (max over all chunks of d, max_chunks_per_doc = 0).
 *     Row g of the output holds the top k of the documents with S_g(d) >= min_score (-INFINITY: no threshold) in the order
 *     (score desc, doc index asc): out_doc, out_score = S_g(d), out_chunk = the arg-max chunk row of d in the row that gave the
 *     maximum, out_src_row = that row (an index into q; equal maxima: the lowest row).  out_n[g] <= k entries (all eligible
 *     documents when there are fewer); the rest of the row is -1 / -inf / -1 / -1.  A group without rows has out_n = 0.
 *     Where the per-row lists come from: with n_rows <= max_queries from exactly ONE msr_dense_topk(q, n_rows,
 *     k + max_g |excl_g|, 0) call -- with sets (n_sets > 0; encoding and refusals of msr_bm25_topk_within, g_set [n_groups]
 *     picks group g's row) the msr_dense_topk_within call in which every row takes its group's set -- so the result equals that
 *     call followed by a merge on the host, bit for bit.  Larger calls make one such call per max_queries rows (whole rows);
 *     a group may hold any number of rows.  A row whose dense list is empty (a NaN row) adds nothing; a zero row adds the
 *     cosines 0 msr_dense_topk gives it.  Exact, ties included: a document of the group's top k reaches its maximum in some row
 *     r, where at most k - 1 eligible and |excl_g| excluded documents rank above it -- it is in row r's top k + |excl_g|.
 *     Refused with MSR_ERR_INVALID, outputs untouched: k < 1; k + max |excl_g| > max_k; group_off not monotone from 0 to
 *     n_rows; excl_off not monotone from 0; an excl_doc outside [0, n_docs) (checked on the device); min_score NaN; q NULL with
 *     n_rows > 0; group_off / excl_off NULL; an output NULL with n_groups > 0; excl_doc NULL with exclusions; the set rules;
 *     while an msr_dense_topk_begin is pending.  MSR_ERR_NOT_BOUND without chunks.  The call reads the two offset arrays on
 *     the host (one synchronisation of the stream); scratch ~44 bytes per row and list entry is kept by the engine. */
int msr_gather_rows(msr_engine* e, const int32_t* rows, int32_t n, float* out, void* stream);
int msr_dense_topk_grouped(msr_engine* e, const float* q, int32_t n_rows, const int32_t* group_off, int32_t n_groups,
                           const int32_t* excl_off, const int32_t* excl_doc, int32_t k, float min_score,
                           const uint32_t* set_bits, int32_t n_sets, int64_t set_stride, const int32_t* g_set,
                           int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_src_row, int32_t* out_n,
                           void* stream);

/* msr_dense_topk in two halves, for a doc-sharded index: between them the caller exchanges ONE float per query across the
 * shards (msretr/distributed.py: an all-reduce MIN over RCCL), after which every shard rescores only the documents that can
 * be in the top-k of the WHOLE corpus instead of its own top-k -- 1 / shards of the exact-f32 rescoring per rank.
 *   msr_dense_split_max(e, k): most queries one begin / end pair takes (0: this engine cannot split -- corpus without row
 *     tiles, fewer than 2 k tiles -- use msr_dense_topk).  Pairs take MORE than 64 queries.
 *   msr_dense_topk_begin: the passes over this shard's rows and the thresholds of its own tile maxima.  out_part[q] f32
 *     [n_queries] (device) <- a cosine that k_part documents of THIS shard are guaranteed to reach EXACTLY (their filter
 *     scores minus the measured error margin); -inf when the shard has fewer than k_part row tiles.  With
 *     k_part = ceil(k / shards), the minimum of out_part[q] over all shards is a lower bound of the k-th exact cosine of the
 *     whole corpus: shards x k_part >= k documents reach it.
 *   msr_dense_topk_end: bound [n_queries] (device; NULL: none) = that minimum.  Candidates whose filter score lies below
 *     bound - (half the filter's measured error margin) cannot be in the global top-k and are dropped before the candidate lists and the exact rescoring.  Output
 *     as msr_dense_topk, except that out_n[q] may be < k: the shard returns every document it can contribute to the global
 *     top-k (merge the shards' lists with msr_merge_topk_payload as usual; the merged list is the unsharded one, bit for bit).
 * One begin may be pending per engine; the matching end must follow with the same n_queries and k.  An msr_unbind between
 * them (an index update) cancels the begin: the end then fails (MSR_ERR_NOT_BOUND while no chunks are bound) and launches
 * nothing. */
int msr_dense_split_max(const msr_engine* e, int32_t k);
int msr_dense_topk_begin(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t k_part, float* out_part,
                         void* stream);
int msr_dense_topk_end(msr_engine* e, int32_t n_queries, int32_t k, const float* bound, int32_t* out_doc, float* out_score,
                       int32_t* out_chunk, int32_t* out_n, void* stream);

/* Batched variant of msr_dense_topk for throughput (BASELINE config 5).  Candidates come from a bf16 image of the
 * NORMALISED rows (v_mfma_f32_16x16x32_bf16, f32 accumulation), whose scores carry a proven error bound; every document
 * within twice that bound of the k-th approximate score is re-scored in f32 from the f32 rows, so the final top-k is
 * exact (same ordering rule as msr_dense_topk).  Up to 128 queries per call: one sweep of the image (msr_batch_width).
 * More: a tiled GEMM, 1024 queries per pass over the image, that never writes the score matrix (msr_batch_gemm_ok; design
 * in csrc/msr_gemm.hip).  A query whose candidate set exceeds the engine's capacity comes back with out_n = -1: rerun it
 * with msr_dense_topk.  msr_enable_bf16 builds the image (+2 bytes per embedding value of HBM) and the scratch of the
 * GEMM path (~0.8 GB); row-major layout only. */
int msr_enable_bf16(msr_engine* e, void* stream);
int msr_dense_topk_bf16(msr_engine* e, const float* q, int32_t n_queries, int32_t k, int32_t max_chunks_per_doc,
                        int32_t* out_doc, float* out_score, int32_t* out_chunk, int32_t* out_n, void* stream);

/* Rerank/fuse of stage-1 candidates, reranker_api.py:337-372.  Query qi has cand_n[qi] <= max_cand
 * candidates in row qi of cand_doc / cand_bm25 (any order).  Candidates not in urlsDB, losing the URL
 * dedup (MIN(id) wins) or without chunks are dropped; the others come back ordered by
 * (new_similarity desc, doc index asc): out_doc, out_score (new_similarity), out_orig (min-max
 * normalised BM25 of the winning row), out_chunk (row index of the winning chunk), out_n, and
 * out_rows[qi] = number of chunk rows that took part (RerankResponse.total_documents, :410).  A document repeated in
 * the candidate list counts once, with the BM25 score of its FIRST slot. */
int msr_rerank(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
               const double* cand_bm25, const int32_t* cand_n, int32_t max_cand,
               const msr_rerank_params* params, int32_t* out_doc, double* out_score, double* out_orig,
               int32_t* out_chunk, int32_t* out_n, int32_t* out_rows, void* stream);

/* Domain diversification of fused lists on the device (reranker_api.py:170-236 hybrid_diversification; :376-397 the response
 * models rejecting NULL title / url / text), so that a batch brings back top_k rows per query instead of max_cand.
 *   msr_bind_doc_domains: domain[d] i32 for every document index the fused lists may hold (GLOBAL indices): the id of
 *     urlparse(url).netloc.lower() (any numbering; equal ids = same domain), or -1 for a document that never appears in a
 *     response.  Borrowed like the other bound arrays; NULL unbinds (every document accepted, each its own domain).
 *   msr_diversify: fused_* [n_queries][max_cand] / fused_n [n_queries] as msr_rerank / msr_rerank_fuse return them (ordered by
 *     (new_similarity desc, doc asc)).  diversify != 0: one result per domain among the domains whose best entry scores
 *     >= relevance_threshold (0.8), then one per remaining domain up to top_k, then -- if still short of top_k -- the dropped
 *     entries with their scores shifted below the last kept one (delta = first_dropped - last_kept + 1e-4, clamped at 0),
 *     float64, the reference's operations in the reference's order.  diversify == 0: the first top_k accepted entries.
 *     out_* [n_queries][max_cand] (like the reference, the list may exceed top_k when more than top_k domains are "high");
 *     rows past out_n[q] are -1 / -inf. */
int msr_bind_doc_domains(msr_engine* e, const int32_t* domain, int64_t n_docs, void* stream);
int msr_diversify(msr_engine* e, int32_t n_queries, const int32_t* fused_doc, const double* fused_score,
                  const double* fused_orig, const int32_t* fused_chunk, const int32_t* fused_n, int32_t max_cand,
                  int32_t top_k, double relevance_threshold, int32_t diversify, int32_t* out_doc, double* out_score,
                  double* out_orig, int32_t* out_chunk, int32_t* out_n, void* stream);

/* Near-duplicate collapse: min-hash signatures of the forward index's documents, and the collapse of
 * each query's fused list by them, between msr_rerank_fuse and msr_diversify.  All arithmetic is uint32, mod 2^32.
 *     fmix(x):  x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16      (murmur3's finaliser)
 *     shingles of a document with stream s[0 .. n), n >= 1, width w:  L = min(w, n), starts a = 0 .. n - L,
 *         h(a) = fmix(x ^ L)  with  x = 0;  for j < L: x = (x ^ (s[a + j] + 1)) * 0x01000193
 *       (a shingle never uses a token of a neighbouring document; a document shorter than w is ONE shingle of all its tokens)
 *     sig[k] = min over a of (A[k] h(a) + B[k]),  A[k] = fmix(2 k + 1) | 1,  B[k] = fmix(2 k + 2),  k < MSR_SIG_WORDS
 *     a document with n == 0 has the EMPTY signature: all words 0xFFFFFFFF
 *     matches(x, y) = |{k : sig_x[k] == sig_y[k]}|  (matches / 64 estimates the Jaccard overlap of the two shingle sets)
 *     dup(x, y)  iff  matches(x, y) >= min_matches and neither signature is EMPTY
 * Collapse of one query's list, slots 0 .. n - 1 in fused order, greedy by leader: slot i is PASSIVE when its document index
 * lies outside the signature table, its signature is EMPTY, or a doc-domain table is bound (msr_bind_doc_domains) and holds a
 * negative id for it or does not reach it (msr_diversify rejects that document: it must not swallow a page that can be
 * shown).  Passive slots are always kept, never lead, never drop.  Any other slot i is DROPPED iff some kept, non-passive
 * slot j < i has dup(i, j); its leader is the smallest such j.  A dropped row leads nothing: A ~ B, B ~ C, A !~ C keeps A and
 * C.  The kept rows, in order, are the output list.
 *
 * msr_doc_signatures: out_sig [d1 - d0][MSR_SIG_WORDS] (device) <- the signatures of documents [d0, d1) of the bound forward
 *   index with shingle width `shingle`.  Only enqueues (one kernel); no engine scratch, no atomics; nothing outside the
 *   rows is written; repeated calls give the same bytes.  MSR_ERR_NOT_BOUND without tokens; MSR_ERR_INVALID, nothing
 *   launched, unless 0 <= d0 <= d1 <= n_docs and 1 <= shingle <= MSR_SIG_MAX_SHINGLE, and for a NULL out_sig with d1 > d0.
 *   d0 == d1 succeeds without a launch.
 * msr_bind_signatures: sig [n_docs][MSR_SIG_WORDS], a device pointer, caller-owned and borrowed like the facet table's; n_docs
 *   must equal the bound postings' count (MSR_ERR_INVALID; MSR_ERR_NOT_BOUND without postings).  NULL unbinds.  msr_unbind
 *   and msr_bind_postings drop the binding.  The table is not read by the bind.
 * msr_collapse_scratch_bytes: bytes of caller scratch one msr_collapse_duplicates call needs (the dup bit matrix:
 *   n_queries * max_cand * ceil(max_cand / 32) words, rounded up to 16 bytes); MSR_ERR_INVALID (negative) for n_queries < 0
 *   or max_cand outside [1, MSR_COLLAPSE_MAX_CAND].  The engine keeps none.
 * msr_collapse_duplicates: fused_* [n_queries][max_cand] / fused_n [n_queries] as msr_rerank_fuse returns them; fused_n[q] is
 *   clamped to [0, max_cand] on the device.  out_* have the shape and padding of msr_diversify's outputs (-1 / -inf / 0.0 /
 *   -1 past out_n[q]) and feed msr_diversify unchanged.  out_drop_doc / out_drop_leader / out_drop_matches
 *   [n_queries][max_cand] int32: in the order they were dropped, the dropped document, its leader's DOCUMENT index and
 *   matches(dropped, leader); -1 / -1 / 0 past out_drop_n[q].  No output may alias an input.  Two kernels over the scratch,
 *   only enqueued, no global atomic, no memset, nothing to zero beforehand; repeated calls give the same bytes.  Refused
 *   before any launch, outputs untouched: MSR_ERR_NOT_BOUND without bound signatures; MSR_ERR_INVALID for min_matches
 *   outside [1, MSR_SIG_WORDS], max_cand outside [1, MSR_COLLAPSE_MAX_CAND], n_queries < 0, a NULL pointer with n_queries >
 *   0, scratch_bytes below msr_collapse_scratch_bytes or a scratch that is not 16-byte aligned.  n_queries == 0 succeeds and
 *   launches nothing. */
int msr_doc_signatures(msr_engine* e, int64_t d0, int64_t d1, int32_t shingle, uint32_t* out_sig, void* stream);
int msr_bind_signatures(msr_engine* e, const uint32_t* sig, int64_t n_docs, void* stream);
int64_t msr_collapse_scratch_bytes(int32_t n_queries, int32_t max_cand);
int msr_collapse_duplicates(msr_engine* e, int32_t n_queries, const int32_t* fused_doc, const double* fused_score,
                            const double* fused_orig, const int32_t* fused_chunk, const int32_t* fused_n, int32_t max_cand,
                            int32_t min_matches, int32_t* out_doc, double* out_score, double* out_orig, int32_t* out_chunk,
                            int32_t* out_n, int32_t* out_drop_doc, int32_t* out_drop_leader, int32_t* out_drop_matches,
                            int32_t* out_drop_n, void* scratch, int64_t scratch_bytes, void* stream);

/* HOST function (every pointer is host memory; no device is touched): the batch result lines of search_api.py:290,
 * "{query_num}\t{rank}\t{url}\t{score:.3f}\n", for n_queries final lists in one call.  Query q's number is the bytes
 * qnum_blob[qnum_off[q] .. qnum_off[q+1]); its list is doc / score [q * stride .. + n[q]) (rank = position + 1); the URL of
 * document d is url_blob[url_off[d] .. url_off[d+1]) (UTF-8; d outside [0, n_docs): empty); max_url_len = the longest URL in
 * bytes (sizes the output without touching the table; <= 0: computed here, one pass over url_off).  The score is printed exactly as
 * Python's format(score, ".3f").  Returns the bytes written; if `capacity` is below the function's upper bound of them nothing
 * is written and the result is -(that bound) (call with capacity 0 to size the buffer); INT64_MIN for a bad argument. */
int64_t msr_format_lines(const char* qnum_blob, const int64_t* qnum_off, int32_t n_queries, const int32_t* doc,
                         const double* score, const int32_t* n, int32_t stride, const char* url_blob, const int64_t* url_off,
                         int64_t n_docs, int64_t max_url_len, char* out, int64_t capacity);

/* The two halves of msr_rerank, for a doc-sharded index (the reference-exact hybrid needs a
 * second exchange).  cand_doc holds GLOBAL document indices and is identical on every rank.
 *   msr_rerank_gather: for the candidates this shard owns (doc_base <= doc < doc_base + n_docs) writes the
 *     cosines of their first <= max_chunks chunks into out_cos[q][m][0..10) and
 *     out_meta[q][m] = (rows, url_group + 2, row_base + first row); everything else is written as 0.
 *     Summing out_cos / out_meta over the shards (one RCCL all-reduce, integer SUM of the raw bits,) yields the arrays of the whole
 *     candidate list, because exactly one shard contributes a non-zero entry.
 *   msr_rerank_fuse: the float64 chain of reranker_api.py:360-372 on those arrays; touches no index, so
 *     every rank computes the same result.  Outputs as msr_rerank (out_doc are global indices); of repeated slots of one
 *     document the first counts. */
int msr_rerank_gather(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                      const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base,
                      int32_t max_chunks, float* out_cos, int32_t* out_meta, void* stream);
/* msr_rerank_gather writing straight into the send buffer of the all-to-all that carries every query's halves to the rank
 * that fuses it (msretr/distributed.py): out_blocks is [n_blocks][block_words] int32; block b belongs to the rank that owns
 * queries [b * queries_per_block, (b + 1) * queries_per_block) and holds their cos rows ([queries_per_block][max_cand][10],
 * float bits) followed by their meta rows ([queries_per_block][max_cand][3]); block_words >= queries_per_block * max_cand * 13
 * (any padding is left untouched).  One launch for all queries of the call (cfg.max_queries of them at a time; for larger
 * calls max_queries must be a multiple of queries_per_block). */
int msr_rerank_gather_blocks(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                             const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base,
                             int32_t max_chunks, int32_t* out_blocks, int32_t queries_per_block, int64_t block_words,
                             void* stream);
int msr_rerank_fuse(msr_engine* e, int32_t n_queries, const int32_t* cand_doc, const double* cand_bm25,
                    const int32_t* cand_n, int32_t max_cand, const float* cos, const int32_t* meta,
                    const msr_rerank_params* params, int32_t* out_doc, double* out_score, double* out_orig,
                    int32_t* out_chunk, int32_t* out_n, int32_t* out_rows, void* stream);

/* Join of the per-shard halves of msr_rerank_gather after they have been exchanged (msretr/distributed.py sends every
 * shard's half of a query to the rank that fuses that query: one all-to-all).  Part p holds cos [n_queries][max_cand][10] at
 * cos_parts + p * part_stride_bytes and meta [n_queries][max_cand][3] at meta_parts + p * part_stride_bytes (4-byte aligned;
 * 16-byte aligned pointers and stride take the wide path).  out = bitwise OR over the parts: exactly one shard owns a
 * candidate's document and wrote non-zero words for it, so the OR is that shard's entry.  No reference counterpart
 * (reranker_api.py:27-63 fetches all rows from one database). */
int msr_rerank_combine(msr_engine* e, const float* cos_parts, const int32_t* meta_parts, int32_t n_parts,
                       int64_t part_stride_bytes, int32_t n_queries, int32_t max_cand, float* out_cos,
                       int32_t* out_meta, void* stream);

/* The COMPACT form of that exchange (round 4; msretr/distributed.py uses it by default).  A rank of an N-way run owns ~1/N of a
 * query's candidates, so the blocks of msr_rerank_gather_blocks are mostly zero words (52 KB per query and rank at max_cand =
 * 1000).  Here a rank sends one RECORD of 16 words per candidate slot it owns -- [slot, rows, url_group + 2, first row,
 * cos x 10 (float bits), query, 0] -- and every rank can size the exchange without talking to anyone: the merged candidate
 * lists are replicated and the shards are document ranges (shard s owns shard_bounds[s] <= doc < shard_bounds[s + 1], device
 * array of n_shards + 1), so
 *   msr_rerank_plan counts, for ALL shards, counts[s][q] = candidates of query q that shard s owns, and derives from it
 *     send_base[q] / send_blk[q][ceil(max_cand / 8)]: the record number of the first owned slot of query q / of each block of
 *       8 slots within the query, in THIS rank's send buffer (records ordered by query, then slot: the records for the
 *       queries of rank o -- queries [o * queries_per_shard, (o + 1) * queries_per_shard) -- are contiguous),
 *     recv_off[s][j]: the record number, in the receive buffer, of the first record source s sends for my j-th query,
 *     pair[s][o]: records source s sends to rank o -- the split sizes of the all-to-all (x 16 words), which the host reads;
 *   msr_rerank_gather_records is msr_rerank_gather writing those records (nothing for slots of other shards; out_records
 *     holds capacity_records records -- n_queries * max_cand is always enough -- and a record whose number is not below that
 *     is not written);
 *   msr_rerank_scatter puts the received records (a buffer of capacity_records records: nothing past it is read) of my
 *     queries [first_query, first_query + n_my_queries) into the dense
 *     out_cos [n_my_queries][max_cand][10] / out_meta [..][3] msr_rerank_fuse reads (zeroed first: a slot nobody owns stays
 *     "no document").  The result equals msr_rerank_combine over the dense halves, bit for bit.
 * All arrays are device pointers.  No reference counterpart (reranker_api.py:27-63 fetches all rows from one database). */
int msr_rerank_plan(msr_engine* e, int32_t n_queries, const int32_t* cand_doc, const int32_t* cand_n, int32_t max_cand,
                    const int32_t* shard_bounds, int32_t n_shards, int32_t my_shard, int32_t queries_per_shard,
                    int32_t* counts, int32_t* send_base, int32_t* send_blk, int32_t* recv_off, int32_t* pair, void* stream);
int msr_rerank_gather_records(msr_engine* e, const float* q, int32_t n_queries, const int32_t* cand_doc,
                              const int32_t* cand_n, int32_t max_cand, int32_t doc_base, int32_t row_base,
                              int32_t max_chunks, const int32_t* send_base, const int32_t* send_blk, int32_t* out_records,
                              int64_t capacity_records, void* stream);
int msr_rerank_scatter(msr_engine* e, const int32_t* records, int64_t capacity_records, const int32_t* counts,
                       const int32_t* recv_off, int32_t n_shards, int32_t n_queries, int32_t queries_per_shard,
                       int32_t first_query, int32_t n_my_queries, int32_t max_cand, float* out_cos, int32_t* out_meta,
                       void* stream);

/* Merge n_parts per-shard top-k lists (the payload of the RCCL all-gather) into the global top-k.
 * in_doc [n_parts][n_queries][k] i32 GLOBAL doc indices, in_score same shape (score_bits = 32: f32,
 * 64: f64), in_n [n_parts][n_queries].  Order: score desc, doc index asc -- identical on every rank.
 * Every part must be in that order already (what msr_bm25_topk / msr_dense_topk return, with doc indices made global by
 * adding the shard's base): the kernel merges sorted lists, it does not sort.
 *   - in_n[p][q] outside [0, k] is clamped to it.  An entry inside the counted prefix whose score is NaN or -inf is dropped
 *     (the rest of its list is merged as if it were not there); out_n[q] = min(k, entries that remain), (-1, -inf) behind it.
 *     -0.0 and +0.0 are one key and come back as +0.0.
 *   - The same document in two lists (nothing a sharded run produces: a document has one owner) is NOT de-duplicated: both
 *     entries are merged like any other; with equal scores they come out next to each other, and which of the two payloads
 *     stands first is unspecified.
 *   - Limit: n_parts <= 64, k <= MSR_MAX_K and pow2ceil(n_parts) * max(64, pow2ceil(k)) <= MSR_MERGE_MAX_ENTRIES (the merge
 *     tree's layout in LDS: 8 x 1000, 16 x 512, 64 x 128 are served; 17 x 480 = 32 x 512 is not, although 17 * 480 <= 8192).
 *     Anything else is refused with MSR_ERR_INVALID and a message naming the limit, before any launch, outputs untouched. */
int msr_merge_topk(msr_engine* e, const int32_t* in_doc, const void* in_score, const int32_t* in_n,
                   int32_t n_parts, int32_t n_queries, int32_t k, int32_t score_bits, int32_t* out_doc,
                   void* out_score, int32_t* out_n, void* stream);
/* The same with (a) an optional 32-bit payload per entry that travels with it: in_payload [n_parts][n_queries][k] ->
 * out_payload [n_queries][k] (-1 past out_n; both NULL: none) -- the dense lists carry their arg-max chunk row this way, so
 * the per-document arg-max of reranker_api.py:370 survives the merge without a second lookup; (b) part_stride_bytes != 0
 * (a multiple of 8): part p of EVERY input array starts that many bytes after part p - 1, i.e. the arrays are read in place
 * from the receive buffer of ONE all-gather whose per-rank record is [doc | score | n | payload ...]; 0: contiguous arrays. */
int msr_merge_topk_payload(msr_engine* e, const int32_t* in_doc, const void* in_score, const int32_t* in_n,
                           const int32_t* in_payload, int32_t n_parts, int64_t part_stride_bytes, int32_t n_queries,
                           int32_t k, int32_t score_bits, int32_t* out_doc, void* out_score, int32_t* out_n,
                           int32_t* out_payload, void* stream);

/* BM25 index build on the GPU (handle-less, OFFLINE: unlike every other entry point this one allocates
 * its own workspace and synchronises the stream).  Replaces the term counting and table writes of BM25.build_index
 * (indexer/bm25_indexer.py:16-54, 203-250; doc_freq :130-147) given pre-tokenised documents: document i (documents in
 * ascending doc_id order, only those with at least one token) owns tok_ids[tok_off[i] .. tok_off[i+1]), term ids in
 * [0, n_terms) -- checked on the device, MSR_ERR_INVALID otherwise.  When capacity >= the number of postings: writes
 * term_off[n_terms + 1] and post_doc / post_tf (CSR by term, documents ascending inside a term, tf = occurrences).
 * *n_postings [host] always receives the number of postings: call once with capacity 0 to size the arrays (that call may
 * return after the counting phase and leave term_off untouched), then again.  All arrays are device pointers. */
int msr_build_postings(const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int32_t n_terms, int64_t* term_off,
                       int32_t* post_doc, int32_t* post_tf, int64_t capacity, int64_t* n_postings, void* stream);

/* Merge of two CSR-by-term posting tables (index update: the postings of newly indexed documents, B, join those of a built
 * index, A; OFFLINE and handle-less like msr_build_postings: allocates its workspace and synchronises).  Each side:
 * x_term_off[x_terms + 1] i64, x_doc / x_tf i32 (documents strictly ascending inside a term), x_map[x_docs] i32 = the side's
 * dense document index -> the merged one, strictly increasing, in [0, n_docs); a_map NULL = identity (A's documents keep
 * their indices).  n_terms >= a_terms, b_terms: the merged vocabulary (term t >= x_terms has no posting on that side).
 * Writes term_off[n_terms + 1] = a_term_off[min(t, a_terms)] + b_term_off[min(t, b_terms)] and post_doc / post_tf: inside a
 * term the two segments merged by mapped document, post_doc = the mapped index, post_tf copied.  MSR_ERR_INVALID, before
 * anything is written: a malformed offset array, a map out of range or not strictly increasing, capacity < the number of
 * postings, or a document with postings of the same term on both sides (never merged silently).  A posting-level
 * malformation (document index outside its side, a descent inside a term) is found during the merge: MSR_ERR_INVALID, with
 * the output written but unspecified.  All arrays are device pointers. */
int msr_merge_postings(const int64_t* a_term_off, int64_t a_terms, const int32_t* a_doc, const int32_t* a_tf,
                       const int32_t* a_map, int64_t a_docs, const int64_t* b_term_off, int64_t b_terms, const int32_t* b_doc,
                       const int32_t* b_tf, const int32_t* b_map, int64_t b_docs, int64_t n_terms, int64_t n_docs,
                       int64_t* term_off, int32_t* post_doc, int32_t* post_tf, int64_t capacity, void* stream);

/* Compaction of a CSR-by-term posting table (index update: documents removed from a built index; OFFLINE and handle-less
 * like msr_build_postings: allocates its workspace and synchronises).  Input: term_off[n_terms + 1] i64, post_doc / post_tf
 * i32 (documents ascending inside a term) and keep[n_docs] u8, nonzero = the document stays.  The new index of a kept
 * document is the number of kept documents before it.  Writes out_term_off[n_terms + 1] = the kept postings before each
 * term_off[t], and out_doc / out_tf: the kept postings in their order, out_doc renumbered, out_tf copied.  *n_postings
 * [host] always receives the number of kept postings: call once with capacity 0 to size the arrays (that call writes
 * nothing), then again.  MSR_ERR_INVALID, before anything is written: term_off not monotone from 0, a post_doc value
 * outside [0, n_docs), or 0 < capacity < the kept count.  No atomics on the data path: the output is the same every run.
 * All arrays are device pointers. */
int msr_compact_postings(const int64_t* term_off, int64_t n_terms, const int32_t* post_doc, const int32_t* post_tf,
                         const uint8_t* keep, int64_t n_docs, int64_t* out_term_off, int32_t* out_doc, int32_t* out_tf,
                         int64_t capacity, int64_t* n_postings, void* stream);

/* Test-only: the exclusive scan the index build and the compaction share (its kernels, its scratch sized by the one helper
 * both use), over an int64 array of the caller, so that tests can run it at its level boundaries (4096 elements per block: two
 * levels above 4096 elements, three above 4096^2) without building an index of that size.  OFFLINE and handle-less like
 * msr_build_postings: allocates its scratch, synchronises and frees.  out[i] <- in[0] + .. + in[i - 1] for i < n (nothing
 * behind out[n - 1] is written); *total (device pointer, nullable) <- the sum of all n elements (0 for n = 0).  in / out are
 * device pointers to n elements and may not overlap.  MSR_ERR_INVALID for n < 0 or, with n > 0, a NULL in or out. */
int msr_debug_exclusive_scan(const int64_t* in, int64_t n, int64_t* out, int64_t* total, void* stream);

/* Test hook, host only (no device call, no engine): what msr_bind_chunks derives from the document offsets doc_off
 * [n_docs + 1] (HOST pointer).  On entry out[3] holds the CU count to cut the spans for (<= 0: 256).  On return out[0] = 1 if
 * the corpus may take the K-split sweeps (msr_scan_width() 64 and up), out[1] = 1 if also the 128-query bf16 sweep
 * (msr_batch_width() 128), out[2] = 1 if every document fits a 256-row tile, out[3] = the number of spans of the K-split
 * kernels.  MSR_ERR_INVALID for offsets msr_bind_chunks would refuse (text in msr_last_error(NULL)). */
int msr_debug_chunk_layout(const int32_t* doc_off, int64_t n_docs, int32_t out[4]);

/* Timing hooks for bench.py: while enabled, every launch of the dominant kernels is bracketed by a
 * hipEvent pair recorded on the caller's stream (ring of 256 launches per kernel).  msr_kernel_time_ms
 * blocks on the recorded events and returns the SUM of the launch durations and the number of launches
 * since msr_set_timing(e, 1).  which: 0 = dense scan kernel, 1 = BM25 TAAT kernel, 2 = GEMM emit pass (all row tiles),
 * 3 = GEMM sample pass (every 16th tile). */
int msr_set_timing(msr_engine* e, int32_t enabled);
int msr_kernel_time_ms(msr_engine* e, int32_t which, float* out_ms, int32_t* out_launches);
/* Measurement hook of the DIAGNOSTIC build (libmsretr_diag.so, -DMSR_DIAG: knock-out switches of the GEMM kernels,
 * tools/gemm_check.py --dbg).  The product library knows no key and returns MSR_ERR_INVALID: it has no switches, no
 * environment variables and one implementation per kernel. */
int msr_tune(msr_engine* e, int32_t key, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* MSRETR_H */

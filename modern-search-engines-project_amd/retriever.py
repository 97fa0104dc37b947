"""Retriever facade: the query -> ranked-documents API of the reference.

  * Retriever(embedder, indexer, db_path).quick_search(query, top_k, return_unique_docs=True)
        the call shape left in search_api.py:60,87 (retriever.py itself is missing from the reference):
        dense retrieval over ALL chunk embeddings, one result per document (max over its chunks).
  * Retriever.search(...) / batch_search(...) / batch_search_to_file(...)
        the live two-stage path of search_api.py:69-152 and :204-367: preprocess_query -> BM25 top-1000 ->
        rerank -> top-100, formatted for the UI / as `qnum<TAB>rank<TAB>url<TAB>score` lines.
"""
import weakref
from dataclasses import replace

import numpy as np

from .bm25 import BM25
from . import facets as _facets
from . import fuzzy as _fuzzy
from . import wildcard as _wildcard
from .docset import DeviceSets
from .engine import DeviceEngine
from .index import CorpusIndex
from .query import Conditions, SearchOptions, parse_queries
from .reranker import Reranker
from .serial import serialised
from .snippets import SNIPPET_TOKENS, query_row, render, term_weights
from .text import LineFormatter, extract_domain, extract_domain_topic, format_result_line, preprocess_query, read_queries_file

TOP_K_RETRIEVAL = 1000     # config.py:13
TOP_K_RERANKING = 100      # config.py:14
RERANK_MAX_CHUNKS = 10     # reranker_api.py:58
DENSE_K = 100              # mode="hybrid": dense candidates that join the BM25 list (default)
SIGNATURE_SHINGLE = 4      # collapse_duplicates=True: tokens per shingle of the documents' min-hash signatures (DESIGN K18)
MATCHED_BY = {1: "lexical", 2: "dense", 3: "both"}       # msr_union_candidates' out_src


def hybrid_k_lex(top_k, rerank_max_docs, dense_k):
    """Lexical candidates of a hybrid step: the rerank chain holds <= rerank_max_docs candidates per query, dense_k of them are
    the dense stage's.  ValueError when either list would be empty."""
    if int(dense_k) < 1:
        raise ValueError(f"dense_k must be >= 1 (got {dense_k})")
    k_lex = min(int(top_k), int(rerank_max_docs) - int(dense_k))
    if k_lex < 1:
        raise ValueError(f"dense_k {dense_k} leaves no room for lexical candidates (top_k {top_k}, rerank_max_docs "
                         f"{rerank_max_docs})")
    return k_lex


class Retriever:
    def __init__(self, embedder=None, indexer=None, db_path=None, tokenizer=None, device=0, freeze_gc=False,
                 span_tokenizer=None, **engine_kw):
        """span_tokenizer: `tokenizer` with each token's place -- a callable text -> iterable of (term, begin, end) over the
        same tokens in the same order (text.simple_tokenize_spans is simple_tokenize's); snippets=True needs it beside a
        custom tokenizer (DESIGN K14)."""
        if isinstance(indexer, DeviceEngine):
            self.engine = indexer
        else:
            index = indexer if isinstance(indexer, CorpusIndex) else CorpusIndex.from_duckdb(db_path)
            self.engine = DeviceEngine(index, device=device, **engine_kw)
        self.index = self.engine.index
        self.embedder = embedder
        self.bm25 = BM25(self.engine, tokenizer=tokenizer) if self.index.term_off is not None else None
        self.reranker = Reranker(self.engine, encoder=embedder) if self.index.doc_off is not None else None
        ids = self.index.doc_ids
        self._ids = ids.cpu().numpy() if hasattr(ids, "cpu") else np.asarray(ids)
        self._domains_bound = False
        self._facet_bound = None
        self._formatter = None
        self._pinned = {}
        self._tokenizer, self._span_tokenizer = tokenizer, span_tokenizer
        self._term_names = None
        if freeze_gc:
            # The corpus side of a retriever is millions of long-lived Python objects (URL / title / text strings, the id maps):
            # every full garbage collection walks them -- tens of milliseconds, in the middle of a 10 ms batch.  They never
            # die, so they are moved to the permanent generation (gc.freeze), as a long-running server would do after start-up.
            import gc
            gc.collect()
            gc.freeze()

    @serialised
    def update_index(self, ix: CorpusIndex):
        """Serve `ix` from now on (an index grown by index_build.bm25_add_token_ids + chunk_index.attach_chunks, shrunk by
        index_build.remove_documents, or both -- a replace): the engine
        rebinds (DeviceEngine.rebind), and everything copied from the old index is refreshed -- the id map, the domain table,
        the line formatter, the per-chunk engine of return_unique_docs=False (closed; rebuilt on first use), the BM25 and
        Reranker facades.  Under the engine's lock (serial.py): a request of another thread sees the old index or the new one,
        whole."""
        ce = getattr(self, "_chunk_engine", None)
        if ce is not None:
            ce.close()
        self._chunk_engine = None
        self.engine.rebind(ix)
        self.index = ix
        ids = ix.doc_ids
        self._ids = ids.cpu().numpy() if hasattr(ids, "cpu") else np.asarray(ids)
        self._domains_bound = False
        self._facet_bound = None
        self._formatter = None
        self._term_names = None
        if ix.term_off is None:
            self.bm25 = None
        elif self.bm25 is None:
            self.bm25 = BM25(self.engine)
        else:
            self.bm25.attach(ix)
        if ix.doc_off is None:
            self.reranker = None
        elif self.reranker is None:
            self.reranker = Reranker(self.engine, encoder=self.embedder)
        else:
            self.reranker.attach(ix)

    def _embed(self, query, query_embedding=None):
        if query_embedding is not None:
            return np.asarray(query_embedding, np.float32)
        if self.embedder is None:
            raise ValueError("a query string needs an embedder (callable or object with .encode)")
        enc = self.embedder.encode if hasattr(self.embedder, "encode") else self.embedder
        return np.asarray(enc(query), np.float32)

    # ------------------------------------------------------------------ dense full scan
    @serialised
    def quick_search_batch(self, queries=None, top_k=10, return_unique_docs=True, query_embeddings=None,
                           max_chunks_per_doc=0, within=None):
        """within: None, a DocSet of this index (every query) or a list of DocSet / None per query: the dense top_k of the
        documents in the set (msr_dense_topk_within; docset.py)."""
        if not return_unique_docs:
            return self._chunk_search_batch(queries, top_k, query_embeddings, within)
        qv = np.stack([self._embed(q, None if query_embeddings is None else query_embeddings[i])
                       for i, q in enumerate(queries if queries is not None else [None] * len(query_embeddings))])
        doc, score, chunk, n = [x.cpu().numpy() for x in self.engine.dense_topk(qv, k=top_k, max_chunks_per_doc=max_chunks_per_doc,
                                                                                within=within)]
        ix = self.index
        cid = ix.chunk_ids.cpu().numpy() if hasattr(ix.chunk_ids, "cpu") else np.asarray(ix.chunk_ids)
        out = []
        for r in range(len(qv)):
            rows = []
            for j in range(int(n[r])):
                i = int(doc[r, j])
                rows.append({"rank": j + 1, "doc_id": int(self._ids[i]), "score": float(score[r, j]),
                             "best_chunk_id": int(cid[int(chunk[r, j])]),
                             "url": ix.urls[i] if ix.urls is not None else None,
                             "title": ix.titles[i] if ix.titles is not None else None})
            out.append(rows)
        return out

    def _chunk_search_batch(self, queries, top_k, query_embeddings, within=None):
        """return_unique_docs=False: the top_k CHUNKS by cosine, several per document allowed (the other half of the call
        shape at search_api.py:87; retriever.py itself is absent from the reference, so the row format is ours: the
        unique-document row plus `chunk_id`).  Runs the same scan kernels over a view of the corpus in which every chunk is
        its own document (built once, on first use; the embedding matrix is shared, not copied)."""
        from .engine import DeviceEngine
        from .index import CorpusIndex
        ix = self.index
        if getattr(self, "_chunk_engine", None) is None:
            C = int(ix.n_chunks)
            # the engine's own device tensor when it holds the rows as they are (row-major layout): shared, not copied
            emb = self.engine._t["emb"] if getattr(self.engine, "scan_layout", 0) == 0 else ix.emb
            view = CorpusIndex(doc_ids=np.arange(C, dtype=np.int64), doc_off=np.arange(C + 1, dtype=np.int32),
                               chunk_ids=ix.chunk_ids, emb=emb, total_docs=C)
            self._chunk_engine = DeviceEngine(view, device=self.engine.device, max_queries=32,
                                              max_k=self.engine.max_k, rerank_max_docs=0)
            off = ix.doc_off.cpu().numpy() if hasattr(ix.doc_off, "cpu") else np.asarray(ix.doc_off)
            self._chunk_doc_off = off.astype(np.int64)
        qv = np.stack([self._embed(q, None if query_embeddings is None else query_embeddings[i])
                       for i, q in enumerate(queries if queries is not None else [None] * len(query_embeddings))])
        if within is not None:                               # document sets -> the chunk view's sets: a chunk is in if its document is
            within = [self._chunk_set(s) for s in within] if isinstance(within, (list, tuple)) else self._chunk_set(within)
        row, score, _, n = self._chunk_engine.dense_topk(qv, k=top_k, want_chunk=False, within=within)
        row, score, n = row.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()
        cid = ix.chunk_ids.cpu().numpy() if hasattr(ix.chunk_ids, "cpu") else np.asarray(ix.chunk_ids)
        out = []
        for r in range(len(qv)):
            rows = []
            for j in range(int(n[r])):
                c = int(row[r, j])
                i = int(np.searchsorted(self._chunk_doc_off, c, side="right") - 1)       # the chunk's document
                rows.append({"rank": j + 1, "doc_id": int(self._ids[i]), "chunk_id": int(cid[c]), "score": float(score[r, j]),
                             "url": ix.urls[i] if ix.urls is not None else None,
                             "title": ix.titles[i] if ix.titles is not None else None})
            out.append(rows)
        return out

    def _chunk_set(self, ds):
        """A DocSet of this index -> the DocSet of the per-chunk view (every chunk of a document in the set).  Cached on `ds`
        itself for the current view, so it lives exactly as long as the caller's set."""
        from .docset import DocSet
        if ds is None:
            return None
        ds.check(self.index)
        view = self._chunk_engine.index
        got = getattr(ds, "_chunk_view", None)
        if got is None or got[0]() is not view:
            got = ds._chunk_view = (weakref.ref(view),
                                    DocSet.from_mask(view, np.repeat(ds.mask, np.diff(self._chunk_doc_off))))
        return got[1]

    @serialised
    def quick_search(self, query=None, top_k=10, return_unique_docs=True, query_embedding=None, max_chunks_per_doc=0,
                     within=None):
        return self.quick_search_batch([query], top_k, return_unique_docs,
                                       None if query_embedding is None else [query_embedding], max_chunks_per_doc,
                                       within=None if within is None else [within])[0]

    # ------------------------------------------------------------------ similar documents (msr_dense_topk_grouped)
    @serialised
    def similar_batch(self, groups, top_k=10, max_source_chunks=RERANK_MAX_CHUNKS, within=None, min_score=None):
        """Documents like the given ones, one ranked list per group, in ONE engine call.  groups: per entry one doc_id or a list
        of doc_ids (the sources).  Each source contributes its first max_source_chunks chunk rows (0 = all; the default 10 is
        the reference's <= 10 chunks per document, reranker_api.py:35,58); a document's score is its best cosine to any
        source row.  The sources are never returned.  within: None, a DocSet (every group) or a list of DocSet / None per
        group; min_score: None or a threshold (e.g. 0.95 for a near-duplicate check).  Rows as quick_search's plus
        source_doc_id / source_chunk_id (the source row that gave the score).  An unknown doc_id raises LookupError."""
        ix = self.index
        ids = self._ids
        off = ix.doc_off.cpu().numpy() if hasattr(ix.doc_off, "cpu") else np.asarray(ix.doc_off)
        rows, row_src, group_off, exclude = [], [], [0], []
        for grp in groups:
            src = [grp] if np.ndim(grp) == 0 else list(grp)
            seen = []
            for d in src:
                i = int(np.searchsorted(ids, int(d)))
                if i >= len(ids) or int(ids[i]) != int(d):
                    raise LookupError(f"doc_id {d} is not in the index")
                if i not in seen:
                    seen.append(i)
            for i in seen:
                a, b = int(off[i]), int(off[i + 1])
                if max_source_chunks:
                    b = min(b, a + int(max_source_chunks))
                rows.extend(range(a, b))
                row_src.extend([i] * (b - a))
            group_off.append(len(rows))
            exclude.append(seen)
        eng = self.engine
        q = eng.gather_rows(np.asarray(rows, np.int64))
        doc, score, chunk, srow, n = [x.cpu().numpy() for x in eng.dense_topk_grouped(q, group_off, exclude, k=top_k,
                                                                                        min_score=min_score, within=within)]
        cid = ix.chunk_ids.cpu().numpy() if hasattr(ix.chunk_ids, "cpu") else np.asarray(ix.chunk_ids)
        out = []
        for g in range(len(exclude)):
            res = []
            for j in range(int(n[g])):
                i, r = int(doc[g, j]), int(srow[g, j])
                res.append({"rank": j + 1, "doc_id": int(ids[i]), "score": float(score[g, j]),
                            "best_chunk_id": int(cid[int(chunk[g, j])]),
                            "url": ix.urls[i] if ix.urls is not None else None,
                            "title": ix.titles[i] if ix.titles is not None else None,
                            "source_doc_id": int(ids[row_src[r]]), "source_chunk_id": int(cid[rows[r]])})
            out.append(res)
        return out

    @serialised
    def similar(self, doc_ids, top_k=10, max_source_chunks=RERANK_MAX_CHUNKS, within=None, min_score=None):
        """The documents most similar to doc_ids (one id or a list): similar_batch with one group."""
        return self.similar_batch([doc_ids], top_k, max_source_chunks, within=None if within is None else [within],
                                  min_score=min_score)[0]

    # ------------------------------------------------------------------ live two-stage path
    # search_api.py:88-130 (single query) and :243-304 (batch): preprocess_query -> bm_25.search(top 1000) -> POST /rerank ->
    # formatted rows.  In the reference every arrow is a Python list of dicts (1000 per query, each with a 200-character
    # snippet or the full document text) and an HTTP/JSON hop.  Here stage 1 -> stage 2 -> diversification stay on the
    # device: msr_bm25_topk -> msr_rerank_gather -> msr_rerank_fuse -> msr_diversify, and only the FINAL <= ~100 rows per
    # query come back to the host, as arrays; URLs / titles / snippets are looked up for those rows only.
    def _doc_domains(self):
        """int32 [N]: domain id (extract_domain(url), reranker_api.py:170-176) of every document, -1 for documents that never
        appear in a response: no urlsDB row, or a NULL title / url / text (the reference's pydantic models reject them,
        :376-397).  Without URL metadata every url is "" -- ONE domain, as the facade's Reranker has it."""
        ix = self.index
        N = ix.n_docs
        if ix.urls is None:
            return np.zeros(N, np.int32)
        ids, out = {}, np.empty(N, np.int32)
        titles, texts = ix.titles, ix.texts
        for i, u in enumerate(ix.urls):
            if u is None or (titles is not None and titles[i] is None) or (texts is not None and texts[i] is None):
                out[i] = -1
            else:
                out[i] = ids.setdefault(extract_domain(u), len(ids))
        return out

    def _ensure_response_tables(self):
        if not self._domains_bound:
            self.engine.bind_doc_domains(self._doc_domains())
            self._domains_bound = True

    def _check_options(self, opts, patterns=False):
        """What the options need, checked before any device work: values in range (SearchOptions.check; patterns: the call
        has explicit patterns) and, of this index and engine, what the features that are on read.  snippets: the spans of a
        custom tokenizer (ValueError), a forward index and texts (MsrError, as phrase search); facets: postings and URLs;
        fuzzy, wildcards and patterns: term strings (ValueError); collapse_duplicates: a forward index (MsrError)."""
        from ._abi import MsrError
        opts.check(patterns)
        if opts.collapse_duplicates and not self.engine.has_tokens:
            raise MsrError(-2, "collapse_duplicates: the index has no forward index (tok_off / tok_ids): build it with "
                               "keep_tokens=True or attach the token streams with index_build.attach_tokens, then update_index")
        if opts.snippets:
            if self._tokenizer is not None and self._span_tokenizer is None:
                raise ValueError("snippets=True with a custom tokenizer needs Retriever(span_tokenizer=...): the tokenizer's "
                                 "(term, begin, end) form (text.simple_tokenize_spans is simple_tokenize's)")
            if not self.engine.has_tokens:
                raise MsrError(-2, "snippets: the index has no forward index (tok_off / tok_ids): build it with keep_tokens=True "
                                   "or attach the token streams with index_build.attach_tokens, then update_index")
            if self.index.texts is None:
                raise MsrError(-2, "snippets: the index has no texts to cut a passage from")
        if opts.facets and (self.bm25 is None or self.index.urls is None):
            raise ValueError("facets=True needs an index with postings and URLs (CorpusIndex.urls)")
        for on, name, verb in ((opts.fuzzy, "fuzzy", "correct a word"), (opts.wildcards or patterns, "wildcards", "expand a pattern")):
            if on and (self.bm25 is None or not self.engine.has_vocab):
                raise ValueError(f"{name}=True needs an index with a vocabulary (CorpusIndex.vocab: term strings); a "
                                 f"term-id-only index cannot {verb}")

    def _ensure_facet(self, by):
        """The facet table of key `by`, bound lazily per index (one table at a time: another key rebinds) and again after
        update_index, like the response tables -> the key's value names."""
        value, names = _facets.facet_values(self.index, by)
        if self._facet_bound != by or not self.engine.has_facet:
            self.engine.bind_facet(value, len(names))
            self._facet_bound = by
        return names

    def _ensure_signatures(self):
        """The documents' min-hash signatures, built on the device and bound lazily per index and again after update_index
        (the rebind drops the tensor with the postings'), like the facet table."""
        if not self.engine.has_signatures:
            self.engine.bind_signatures(self.engine.doc_signatures(SIGNATURE_SHINGLE))

    def _facet_chunk(self, term_ids, within, facet):
        """One facet_counts call for a chunk's queries: the counting terms (facets.counting_terms) of the ids that are scored,
        inside `within` -- what stage 1 is restricted to, the chunk's DeviceSets when operators, phrases or proximity built
        one.  A query without a valid term gets a list that matches nothing (0 hits); a chunk of such queries makes no call."""
        Q, limit = len(term_ids), int(facet["limit"])
        lists = [_facets.counting_terms(self.index, t) or [-1] for t in term_ids]
        if any(l != [-1] for l in lists):
            hits, n_hit, tv, tc = self.engine.facet_counts(lists, within=within, limit=limit)
        else:
            hits, n_hit = np.zeros(Q, np.int32), np.zeros(Q, np.int32)
            tv, tc = np.full((Q, limit), -1, np.int32), np.zeros((Q, limit), np.int32)
        for key, part in (("hits", hits), ("n_values_hit", n_hit), ("top_value", tv), ("top_count", tc)):
            facet[key] += list(part)

    FINAL_COLS = 128           # columns of the final lists copied back per query (top_k = 100 + slack; a longer list -- more
    #                            than top_k "high" domains -- makes that chunk come back in full)

    def _fused_chunk(self, term_ids, qv, top_k, within=None, mode="lexical", dense_k=DENSE_K):
        """Stage 1 and the rerank chain up to the fused lists of one chunk -> (fused, union): what rerank_fuse returns and, in
        hybrid mode, what union_candidates does (else None).  Only enqueues."""
        eng, cfg = self.engine, self.reranker.cfg
        union = None
        if mode == "hybrid":
            k_lex = hybrid_k_lex(top_k, eng.rerank_max_docs, dense_k)
            packed = eng.pack_queries(term_ids)
            lex = eng.bm25_topk(None, k=k_lex, packed=packed, within=within)
            dd, _, _, dn = eng.dense_topk(qv, k=int(dense_k), want_chunk=False, within=within)
            dbm, _ = eng.bm25_score_docs(None, dd, dn, packed=packed)
            union = eng.union_candidates(lex, dd, dbm, dn)
            b = (union[0], union[1], union[3])
        else:
            b = eng.bm25_topk(term_ids, k=top_k, within=within)
        cos, meta = eng.rerank_gather(qv, b[0], b[2], max_chunks=RERANK_MAX_CHUNKS)
        return eng.rerank_fuse(b[0], b[1], b[2], cos, meta, smoothing=cfg["smoothing"], max_chunks=RERANK_MAX_CHUNKS), union

    def _enqueue_chunk(self, term_ids, qv, top_k, slot, within=None, mode="lexical", dense_k=DENSE_K, cond=None, facet=None,
                       min_matches=None, match=None):
        """Device work of one chunk + the asynchronous copy of its final rows into pinned host buffers.  Only enqueues.
        within (None | DocSet | list per query of the chunk): stage 1 restricted to the sets; the rerank chain is unchanged.
        mode="hybrid": stage 1 = the BM25 top k_lex (hybrid_k_lex) followed by the dense top dense_k documents it lacks, each
        with its true BM25 score (msr_bm25_score_docs, msr_union_candidates); the candidates and where each came from are
        copied to pinned buffers beside the final rows (the job's sixth entry).
        cond (None | the Conditions of the chunk's queries, over term ids): its term lists make ONE term_sets call in front of
        stage 1, which turns them, inside `within`, into device sets that take within's place in both stages; nothing else
        changes.  With phrase lists ONE phrase_sets call takes the term_sets call's place (it makes that call itself, with
        the phrases' candidate rows).
        facet (None | the dict of final_list_chunks' facets=): ONE facet_counts call over the chunk's scored terms inside the
        sets stage 1 is restricted to (_facet_chunk); its answer comes back to the host before stage 1 is enqueued.
        min_matches (None | 1 .. 64, SearchOptions.min_matches): ONE collapse_duplicates call between fuse and diversify; what
        it dropped is copied to pinned buffers beside the final rows (the job's seventh entry; the sixth is then None in
        lexical mode).
        match (None | (slots, needs) of the chunk's queries, match.slots / match.need): ONE match.match_sets call behind the
        conditions' call, inside what that built; its sets take within's place in both stages and in the facet counts."""
        import torch
        eng, cfg = self.engine, self.reranker.cfg
        if cond is not None:
            within = cond.sets(eng, within)
        if match is not None:
            from .match import match_sets
            within = match_sets(eng, match[0], match[1], within)
        if facet is not None:
            self._facet_chunk(term_ids, within, facet)
        fused, union = self._fused_chunk(term_ids, qv, top_k, within, mode, dense_k)
        drops = None
        if min_matches is not None:
            fused, drops = eng.collapse_duplicates(fused, min_matches)
        fin = eng.diversify(fused, top_k=int(cfg["top_k"]), diversification=bool(cfg.get("diversification", False)))
        Qc, W = len(term_ids), min(self.FINAL_COLS, int(fin[0].shape[1]))
        pin = self._pinned.get(slot)
        if pin is None or pin[0].shape[0] < Qc or pin[0].shape[1] != W:
            rows = max(Qc, 256)
            pin = self._pinned[slot] = (torch.empty((rows, W), dtype=torch.int32, pin_memory=True),
                                        torch.empty((rows, W), dtype=torch.float64, pin_memory=True),
                                        torch.empty((rows, W), dtype=torch.int32, pin_memory=True),
                                        torch.empty((rows,), dtype=torch.int32, pin_memory=True))
        pin[0][:Qc].copy_(fin[0][:, :W], non_blocking=True)
        pin[1][:Qc].copy_(fin[1][:, :W], non_blocking=True)
        pin[2][:Qc].copy_(fin[3][:, :W], non_blocking=True)
        pin[3][:Qc].copy_(fin[4], non_blocking=True)
        upin = None
        if union is not None:
            M = int(union[0].shape[1])
            upin = self._pinned.get(("union", slot))
            if upin is None or upin[0].shape[0] < Qc or upin[0].shape[1] != M:
                rows = max(Qc, 256)
                upin = self._pinned[("union", slot)] = (torch.empty((rows, M), dtype=torch.int32, pin_memory=True),
                                                        torch.empty((rows, M), dtype=torch.int32, pin_memory=True),
                                                        torch.empty((rows,), dtype=torch.int32, pin_memory=True))
            upin[0][:Qc].copy_(union[0], non_blocking=True)
            upin[1][:Qc].copy_(union[2], non_blocking=True)
            upin[2][:Qc].copy_(union[3], non_blocking=True)
        dpin = None
        if drops is not None:
            M = int(drops[0].shape[1])
            dpin = self._pinned.get(("drops", slot))
            if dpin is None or dpin[0].shape[0] < Qc or dpin[0].shape[1] != M:
                rows = max(Qc, 256)
                dpin = self._pinned[("drops", slot)] = tuple(torch.empty((rows, M), dtype=torch.int32, pin_memory=True)
                                                             for _ in range(3)) + (torch.empty((rows,), dtype=torch.int32,
                                                                                               pin_memory=True),)
            for k in range(4):
                dpin[k][:Qc].copy_(drops[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(eng.device))
        if dpin is not None:
            return (fin, pin, ev, Qc, W, upin, dpin)
        return (fin, pin, ev, Qc, W) if upin is None else (fin, pin, ev, Qc, W, upin)

    @staticmethod
    def _collect_chunk(job):
        """Wait for a chunk's copies -> (doc, score, chunk row, n) numpy arrays of that chunk (copies: the pinned buffers are
        reused two chunks later)."""
        fin, pin, ev, Qc, W = job[:5]
        ev.synchronize()
        n = pin[3][:Qc].numpy().copy()
        S = int(n.max()) if Qc else 0
        if S > W:                                            # (rare) a list longer than the copied columns: this chunk in full
            return fin[0][:, :S].cpu().numpy(), fin[1][:, :S].cpu().numpy(), fin[3][:, :S].cpu().numpy(), n
        return pin[0][:Qc, :S].numpy().copy(), pin[1][:Qc, :S].numpy().copy(), pin[2][:Qc, :S].numpy().copy(), n

    @staticmethod
    def _collect_source(job, doc, n):
        """Hybrid mode, after _collect_chunk: int32 [Qc, S], where each final row's document came from (msr_union_candidates'
        out_src: 1 lexical, 2 dense, 3 both; 0 past n) -- looked up by document index in the chunk's candidate lists."""
        udoc, usrc, un = job[5]
        Qc = job[3]
        udoc, usrc, un = udoc[:Qc].numpy(), usrc[:Qc].numpy(), un[:Qc].numpy()
        S = doc.shape[1]
        live = np.arange(S)[None, :] < np.asarray(n)[:, None]
        src = np.where(live, 1, 0).astype(np.int32)              # lexical only, unless the dense list names the document
        uq, um = np.nonzero((usrc >= 2) & (np.arange(udoc.shape[1])[None, :] < un[:, None]))      # <= dense_k slots per query
        if len(uq) == 0 or not live.any():
            return src
        key = (uq.astype(np.int64) << 32) | udoc[uq, um].astype(np.int64)
        order = np.argsort(key, kind="stable")
        key, val = key[order], usrc[uq, um][order]
        fq, fr = np.nonzero(live)
        want = (fq.astype(np.int64) << 32) | doc[fq, fr].astype(np.int64)
        pos = np.minimum(np.searchsorted(key, want), len(key) - 1)
        hit = key[pos] == want
        src[fq[hit], fr[hit]] = val[pos[hit]]
        return src

    @staticmethod
    def _collect_drops(job, dedup):
        """After _collect_chunk (the event has been waited for): what the chunk's collapse dropped, appended per query to
        dedup["drops"] as int32 [n, 3] rows (dropped document, leader document, matches), in drop order."""
        Qc = job[3]
        d_doc, d_lead, d_m, d_n = (x[:Qc].numpy() for x in job[6])
        for q in range(Qc):
            n = int(d_n[q])
            dedup["drops"].append(np.stack([d_doc[q, :n], d_lead[q, :n], d_m[q, :n]], axis=1).astype(np.int32))

    @serialised
    def final_list_chunks(self, term_id_lists=None, query_vectors=None, top_k=TOP_K_RETRIEVAL, chunk=None, prepare=None,
                          n_queries=None, within=None, mode="lexical", dense_k=DENSE_K, operators=False, must=None,
                          must_not=None, phrases=False, must_phrases=None, must_not_phrases=None, proximity=False, fuzzy=None,
                          wildcards=None, facets=None, match="any"):
        """The whole live path, chunk by chunk, on the device; yields (first query, doc index int32 [Qc, S], new_similarity
        float64 [Qc, S], winning chunk row int32 [Qc, S], n int32 [Qc]) per chunk of queries, rows in final rank order.
        Software-pipelined: while the GPU works on chunk i the host packs chunk i + 1 and the caller consumes chunk i - 1.
        prepare(a, b) (optional, with n_queries) -> (term id lists, vectors) of queries a .. b, evaluated just before the chunk
        is enqueued (text preprocessing inside the pipeline); otherwise term_id_lists / query_vectors hold all queries.
        within: None, a DocSet (every query), a list of DocSet / None per query or a DeviceSets of all Q queries (each chunk
        takes its queries' part; not together with must / must_not): BM25 stage restricted to the set, then the
        unchanged rerank / fuse / diversify on those candidates (the min-max normalisation spans the restricted candidates).
        What the options do: query.SearchOptions; here the queries are term ids, so the options come in this form:
        mode="hybrid": the candidates are the BM25 top min(top_k, rerank_max_docs - dense_k) AND the dense top dense_k (both
        within the set, if any), see _enqueue_chunk; every chunk then carries a sixth array, int32 [Qc, S]: where each row's
        document came from (1 lexical, 2 dense, 3 both).  A query without a known term still gets its dense candidates.
        must / must_not / must_phrases / must_not_phrases (query.Conditions): the terms are strings or ids and a phrase is a
        list of them (or a text.Near) -- one DeviceEngine.term_sets or phrase_sets call per chunk builds the sets on the
        device, inside `within`; in hybrid mode the dense candidates are restricted too.  operators / phrases / proximity:
        there is no text to parse -- True is refused (search / search_batch / batch_search parse; or text.parse_operators,
        parse_phrases, parse_proximity and the lists).
        fuzzy: None, or a dict {"terms": per query the term STRINGS that term_id_lists was mapped from}: per chunk the lookup
        stands in front of stage 1 (the place term_sets has) and replaces each -1 of the chunk's term ids and must ids
        (fuzzy.correct).  The generator fills fuzzy["corrections"] (per query {typed: used}) and fuzzy["ids"] (the term ids that
        were scored).  The lookup's answer comes back to the host before the chunk is enqueued: with fuzzy the host does not
        run ahead of the device.  Not with prepare=.
        wildcards: None, or a dict {"patterns": per query its pattern strings, "limit": 1 .. 16}: per chunk the lookup stands
        where the fuzzy lookup does (behind it when both are given: a pattern is never corrected) and appends each query's
        expansions behind its term ids (wildcard.expand).  The generator fills wildcards["expansions"] (per query {pattern:
        {...}}) and wildcards["ids"] (the term ids that were scored).  Like fuzzy, the answer comes back before the chunk is
        enqueued; same refusal of prepare=.
        facets: None, or a dict {"by": "host" | "domain", "limit": 1 .. 64}.  The generator fills facets["hits"],
        ["n_values_hit"], ["top_value"], ["top_count"] (per query) and ["names"] (the key's value names).
        match: "any" (default), a match value ("all", m, "75%": SearchOptions) or a dict {"value": that value}: each query's
        term ids are its slots (match.slots, with the expansions of each pattern as one slot) and ONE match.match_sets call per
        chunk restricts both stages to the pages that fill enough of them.  The generator fills the dict's ["slots"] (per
        query its groups of term ids), ["need"] (per query an int, None: no slot) and ["info"] (per query the `match` value
        of search_batch's results).
        Threads: the generator holds the engine's lock (serial.py) from its first next() to exhaustion, close() or an
        exception -- also while the caller works between two chunks: the pinned buffers, the facet table and the index
        belong to this call until then, so no other request can read or overwrite a chunk's rows.  Finish or close it on the
        thread that started it (the lock is that thread's), and soon: every other request on this engine waits."""
        match = self._match_dict(match)
        opts = SearchOptions(mode, dense_k, operators, phrases, proximity, match="any" if match is None else match["value"])
        cond = Conditions(must, must_not, must_phrases, must_not_phrases)
        yield from self._chunks(term_id_lists, query_vectors, top_k, chunk, prepare, n_queries, within, opts, cond, fuzzy, wildcards,
                                facets, match=match)

    @staticmethod
    def _match_dict(match):
        """final_list_chunks' match= -> None (off) or the dict the generator fills."""
        if isinstance(match, dict):
            return match
        return {"value": match} if SearchOptions(match=match).match_on else None

    def _chunks(self, term_id_lists, query_vectors, top_k, chunk, prepare, n_queries, within, opts, cond, fuzzy, wildcards, facets,
                parsed=False, dedup=None, match=None):
        """final_list_chunks over the two values.  Of opts it reads mode, dense_k and the text switches -- parsed: they were
        applied by parse_queries (else True is refused); fuzzy / wildcards / facets: final_list_chunks' dicts, which hold
        those features' limits.  dedup: None, or a dict: collapse_duplicates is on with opts' duplicate_threshold; the generator
        fills dedup["drops"] (per query, _collect_drops).  match: None, or final_list_chunks' dict (its "terms", if given:
        per query the term strings the ids were mapped from, for the words of the slots that no term fills)."""
        import torch
        eng = self.engine
        opts = replace(opts, snippets=False, fuzzy=fuzzy is not None, wildcards=wildcards is not None,
                       match="any" if match is None else match["value"],
                       max_expansions=(wildcards or {}).get("limit", 8), facets=facets is not None,
                       facet_by=(facets or {}).get("by", "host"), facet_limit=(facets or {}).get("limit", 10),
                       collapse_duplicates=dedup is not None)
        self._check_options(opts)
        if dedup is not None:
            self._ensure_signatures()
            dedup.update(min_matches=opts.min_matches, drops=[])
        if fuzzy is not None:
            if prepare is not None or len(fuzzy["terms"]) != len(term_id_lists):
                raise ValueError("fuzzy: needs the term strings of every query (not with prepare=)")
            fuzzy["corrections"], fuzzy["ids"] = [], []
        if wildcards is not None:
            if prepare is not None or len(wildcards["patterns"]) != len(term_id_lists):
                raise ValueError("wildcards: needs the patterns of every query (not with prepare=)")
            wildcards["expansions"], wildcards["ids"] = [], []
        if match is not None:
            from . import match as _match
            if self.bm25 is None:
                raise ValueError("match= needs an index with postings")
            if prepare is not None:
                raise ValueError("match: needs the term ids of every query (not with prepare=)")
            match.update(slots=[], need=[], info=[])
        if facets is not None:
            facets["names"] = self._ensure_facet(opts.facet_by)
            facets.update(limit=int(opts.facet_limit), hits=[], n_values_hit=[], top_value=[], top_count=[])
        for name, parser, lists in (("operators", "parse_operators", "must= / must_not="),
                                    ("phrases", "parse_phrases", "must_phrases= / must_not_phrases="),
                                    ("proximity", "parse_proximity", "must_phrases= / must_not_phrases=")):
            if getattr(opts, name) and not parsed:
                raise ValueError(f"{name}=True needs the query text: use search / search_batch / batch_search, or parse with "
                                 f"text.{parser} and pass {lists}")
        if top_k > eng.rerank_max_docs or top_k > eng.max_k:
            raise ValueError(f"top_k {top_k} exceeds the engine's max_k / rerank_max_docs ({eng.max_k} / {eng.rerank_max_docs})")
        if opts.mode == "hybrid":
            hybrid_k_lex(top_k, eng.rerank_max_docs, opts.dense_k)
            if int(opts.dense_k) > eng.max_k:
                raise ValueError(f"dense_k {opts.dense_k} exceeds the engine's max_k ({eng.max_k})")
        self._ensure_response_tables()
        Q = len(term_id_lists) if prepare is None else int(n_queries)
        step = int(chunk or max(256, eng.max_queries))
        if isinstance(within, (list, tuple, DeviceSets)) and len(within) != Q:
            raise ValueError(f"within: {len(within)} entries for {Q} queries")
        cond.check(Q)
        pending = None
        for i, a in enumerate(range(0, Q, step)):
            b = min(Q, a + step)
            ids, qv = prepare(a, b) if prepare is not None else (term_id_lists[a:b], query_vectors[a:b])
            qv = eng._dev(np.asarray(qv, np.float32) if not torch.is_tensor(qv) else qv, torch.float32).reshape(-1, 768)
            w = (list(within[a:b]) if isinstance(within, (list, tuple))
                 else within.queries(a, b) if isinstance(within, DeviceSets) else within)
            c = None if cond.empty else cond.slice(a, b).ids(self.index.term_ids, lambda t: self.bm25._tokenize(t))
            if fuzzy is not None:
                ids, m_ids, corr = _fuzzy.correct(self.bm25._lookup, self.bm25._name_of, fuzzy["terms"][a:b], ids,
                                                  None if cond.must is None else cond.must[a:b], None if c is None else c.must)
                c = None if c is None else replace(c, must=m_ids)
                fuzzy["corrections"] += corr
                fuzzy["ids"] += ids
            typed = ids                                          # (what the user's words became; the expansions come behind)
            exp = None
            if wildcards is not None:
                lim = int(opts.max_expansions)
                ids, exp = _wildcard.expand(lambda ps: eng.wildcard_terms(ps, limit=lim), self.bm25._name_of, ids,
                                            wildcards["patterns"][a:b], lim)
                wildcards["expansions"] += exp
                wildcards["ids"] += ids
            m = None
            if match is not None:
                m = self._match_chunk(_match, match, typed, exp, a)
            job = self._enqueue_chunk(ids, qv, top_k, i & 1, within=w, mode=opts.mode, dense_k=opts.dense_k, cond=c, facet=facets,
                                      min_matches=None if dedup is None else dedup["min_matches"], match=m)
            if pending is not None:
                yield (pending[0],) + self._collect(pending[1], dedup)
            pending = (a, job)
        if pending is not None:
            yield (pending[0],) + self._collect(pending[1], dedup)

    def _match_chunk(self, _match, match, typed, exp, a):
        """The slots and needs of one chunk (queries a ..): typed -- per query its term ids after correction, exp -- None or per
        query wildcard.expand's {pattern: {"terms": [...]}}.  Appends to match["slots"] / ["need"] / ["info"] -> (slots,
        needs) for _enqueue_chunk, or None when no query of the chunk has a slot."""
        ix, name_of, terms = self.index, self.bm25._name_of, match.get("terms")
        groups, needs = [], []
        for q, ids in enumerate(typed):
            expansions = None if exp is None else [ix.term_ids(info["terms"]) for info in exp[q].values()]
            g = _match.slots(ix, ids, expansions)
            n = _match.need(match["value"], len(g))
            words = terms[a + q] if terms is not None and len(terms[a + q]) == len(ids) else ()
            unknown = [w for w, t in zip(words, ids) if not 0 <= int(t) < ix.n_terms]
            groups.append(g)
            needs.append(n)
            match["info"].append({"slots": _match.slot_names(g, name_of, unknown), "need": n})
        match["slots"] += groups
        match["need"] += needs
        return (groups, needs) if any(n is not None for n in needs) else None

    @classmethod
    def _collect(cls, job, dedup=None):
        out = cls._collect_chunk(job)
        if dedup is not None:
            cls._collect_drops(job, dedup)
        return out if len(job) == 5 or job[5] is None else out + (cls._collect_source(job, out[0], out[3]),)

    @serialised
    def final_lists(self, term_id_lists, query_vectors, top_k=TOP_K_RETRIEVAL, chunk=None, within=None, mode="lexical",
                    dense_k=DENSE_K, with_source=False, operators=False, must=None, must_not=None, phrases=False,
                    must_phrases=None, must_not_phrases=None, proximity=False, fuzzy=None, wildcards=None, facets=None,
                    match="any"):
        """-> host arrays (doc index int32 [Q, S], new_similarity float64 [Q, S], winning chunk row int32 [Q, S], n int32 [Q]);
        row q holds n[q] entries in final rank order (S = max n, normally the reranker's top_k = 100).  term_id_lists: per
        query its term ids (repeats allowed, unknown < 0); query_vectors [Q, 768].  with_source (hybrid mode only): a fifth
        array, int32 [Q, S]: 1 lexical, 2 dense, 3 both (0 past n).  Everything else: final_list_chunks, whose chunks this
        joins."""
        match = self._match_dict(match)
        opts = SearchOptions(mode, dense_k, operators, phrases, proximity, match="any" if match is None else match["value"])
        cond = Conditions(must, must_not, must_phrases, must_not_phrases)
        return self._final(term_id_lists, query_vectors, top_k, chunk, within, opts, cond, fuzzy, wildcards, facets, with_source,
                           match=match)

    def _final(self, ids, qv, top_k, chunk, within, opts, cond, fuzzy, wildcards, facets, with_source=False, parsed=False,
               dedup=None, match=None):
        """final_lists over the two values: _chunks' chunks joined (parsed, the dicts: _chunks)."""
        opts.check()
        if with_source and opts.mode != "hybrid":
            raise ValueError("with_source needs mode='hybrid'")
        parts = list(self._chunks(ids, qv, top_k, chunk, None, None, within, opts, cond, fuzzy, wildcards, facets, parsed, dedup,
                                  match))
        if not parts:
            z = np.zeros((0, 0), np.int32)
            return (z, np.zeros((0, 0), np.float64), z, np.zeros(0, np.int32)) + ((z,) if with_source else ())
        S = max(p[1].shape[1] for p in parts)
        pad = lambda x, fill: x if x.shape[1] == S else np.concatenate(
            [x, np.full((x.shape[0], S - x.shape[1]), fill, x.dtype)], axis=1)
        out = (np.concatenate([pad(p[1], -1) for p in parts]), np.concatenate([pad(p[2], -np.inf) for p in parts]),
               np.concatenate([pad(p[3], -1) for p in parts]), np.concatenate([p[4] for p in parts]))
        return out + ((np.concatenate([pad(p[5], 0) for p in parts]),) if with_source else ())

    def _front(self, queries, query_embeddings, term_lists, opts, explicit, patterns):
        """The front half of search_batch and batch_search: check the options, preprocess and parse the queries
        (query.parse_queries), tokenise, map and embed them -> (term ids, vectors, Conditions, fz, wc, fc, mt): the dicts of
        final_list_chunks' fuzzy= / wildcards= / facets= / match=, None where the feature is off.  fz also receives "processed"
        (the scoring texts), mt "terms" (the term strings).  The scoring text (patterns, excluded words and phrases removed, quotes gone) is what gets
        tokenised; the text that is embedded keeps a pattern."""
        self._check_options(opts, patterns is not None)
        fz = {} if opts.fuzzy else None
        fc = {"by": opts.facet_by, "limit": int(opts.facet_limit)} if opts.facets else None
        scoring, embed_text, cond, pats = parse_queries([preprocess_query(q) for q in queries], lambda t: self.bm25._tokenize(t),
                                                        opts, explicit, patterns)
        wc = None if pats is None else {"patterns": pats, "limit": int(opts.max_expansions)}
        mt = {"value": opts.match} if opts.match_on else None
        front = self._prepare(queries, query_embeddings, term_lists, scoring, fz if fz is not None else mt, embed_text)
        if mt is not None and fz is not None:
            mt["terms"] = fz["terms"]
        return front + (cond, fz, wc, fc, mt)

    @staticmethod
    def _scored_ids(ids, fz, wc):
        """The term ids that were scored (the snippets look for those words): after correction, with the expansions."""
        return wc["ids"] if wc is not None else fz["ids"] if fz is not None else ids

    def _prepare(self, queries, query_embeddings, term_lists, processed=None, keep=None, embed_text=None):
        """keep (a dict, optional) receives "processed" (the scoring texts) and "terms" (the term lists the ids came from).
        embed_text: None, or per query the text to embed where it differs from the scoring text."""
        if processed is None:
            processed = [preprocess_query(q) for q in queries]
        if term_lists is None:
            term_lists = [self.bm25._tokenize(q) for q in processed]
        if keep is not None:
            keep.update(processed=list(processed), terms=[list(t) for t in term_lists])
        ids = [self.index.term_ids(t) for t in term_lists]
        if isinstance(query_embeddings, np.ndarray) and query_embeddings.ndim == 2:
            qv = np.ascontiguousarray(query_embeddings, np.float32)             # (a matrix of vectors: taken as it is)
        else:
            qv = np.stack([self._embed((embed_text or processed)[i], None if query_embeddings is None else query_embeddings[i])
                           for i in range(len(queries))]) if len(queries) else np.zeros((0, 768), np.float32)
        return ids, qv

    # ------------------------------------------------------------------ query-biased snippets (msr_best_windows, DESIGN K14)
    def _term_name(self, t):
        if self._term_names is None:
            self._term_names = {v: k for k, v in (self.index.vocab or {}).items()}
        return self._term_names.get(t, str(t))

    def _snippets(self, ids, doc, n, snippet_tokens):
        """-> {(query, rank index): (snippet, highlights, missing)} for the returned documents that have a window, and per
        query its row's term strings (None: no row).  ONE best_windows call for all pairs of the call: the row of a query is
        snippets.query_row of its term ids, the weights term_weights, the span snippet_tokens."""
        ix, span = self.index, int(snippet_tokens)
        rows, row_of = [], []
        for q in range(len(ids)):
            row = query_row(ix, ids[q]) if int(n[q]) else None
            row_of.append(None if row is None else len(rows))
            if row is not None:
                rows.append(row)
        names = [None if r is None else [self._term_name(t) for t in rows[r]] for r in row_of]
        pq = [q for q in range(len(ids)) if row_of[q] is not None for _ in range(int(n[q]))]
        pr = [r for q in range(len(ids)) if row_of[q] is not None for r in range(int(n[q]))]
        if not pq:
            return {}, names
        pair_doc = doc[pq, pr]
        out = self.engine.best_windows(pair_doc, [row_of[q] for q in pq], rows, [term_weights(ix, row) for row in rows], span)
        start, _, _, mask, terms = [x.cpu().numpy() for x in out]
        mask, terms = mask.view(np.uint64), terms.view(np.uint32)
        titles, texts, got = ix.titles, ix.texts, {}
        for i, (q, r) in enumerate(zip(pq, pr)):
            if start[i] < 0:
                continue
            d = int(pair_doc[i])
            snippet, highlights = render(titles[d] if titles is not None else None, texts[d], int(start[i]), int(mask[i]), span,
                                         self._span_tokenizer)
            got[q, r] = (snippet, highlights, [w for j, w in enumerate(names[q]) if not int(terms[i]) >> j & 1])
        return got, names

    @serialised
    def search_batch(self, queries, top_k=TOP_K_RETRIEVAL, query_embeddings=None, term_lists=None, query_ids=None, within=None,
                     mode="lexical", dense_k=DENSE_K, operators=False, must=None, must_not=None, phrases=False,
                     must_phrases=None, must_not_phrases=None, proximity=False, snippets=False, snippet_tokens=SNIPPET_TOKENS,
                     fuzzy=False, wildcards=False, max_expansions=8, patterns=None, facets=False, facet_by="host",
                     facet_limit=10, collapse_duplicates=False, duplicate_threshold=0.9, match="any"):
        """-> per query the list of UI documents (search_api.py:110-130); [] when stage 1 finds nothing.  within: None, a DocSet
        (every query) or a list of DocSet / None per query -- results from the documents of the set only (final_list_chunks).
        The switches and limits: query.SearchOptions; must / must_not / must_phrases / must_not_phrases: query.Conditions,
        one entry per query; patterns: per query None or a list of pattern strings.  With fuzzy, wildcards, patterns,
        facets, collapse_duplicates or match each query's result is a fuzzy.Results list."""
        opts = SearchOptions(mode, dense_k, operators, phrases, proximity, snippets, snippet_tokens, fuzzy, wildcards, max_expansions,
                             facets, facet_by, facet_limit, collapse_duplicates, duplicate_threshold, match)
        return self._search(queries, top_k, query_embeddings, term_lists, query_ids, within, opts,
                            Conditions(must, must_not, must_phrases, must_not_phrases), patterns)

    def _search(self, queries, top_k, query_embeddings, term_lists, query_ids, within, opts, explicit, patterns):
        """search_batch over the two values."""
        ids, qv, cond, fz, wc, fc, mt = self._front(queries, query_embeddings, term_lists, opts, explicit, patterns)
        dd = {} if opts.collapse_duplicates else None
        doc, score, _, n, *src = self._final(ids, qv, top_k, None, within, opts, cond, fz, wc, fc, with_source=opts.mode == "hybrid",
                                             parsed=True, dedup=dd, match=mt)
        src = src[0] if src else None                        # (hybrid mode: where each row's document came from)
        ix, snippets = self.index, opts.snippets
        ids = self._scored_ids(ids, fz, wc)
        passages, row_names = self._snippets(ids, doc, n, opts.snippet_tokens) if snippets else (None, None)
        out = []
        for q in range(len(queries)):
            rows = []
            qid = None if query_ids is None else query_ids[q]
            led = self._duplicates_of(dd["drops"][q]) if dd is not None else {}
            for r in range(int(n[q])):
                i = int(doc[q, r])
                url = ix.urls[i] if ix.urls is not None else ""
                title = ix.titles[i] if ix.titles is not None else ""
                text = ix.texts[i] if ix.texts is not None else ""
                rows.append({"query_id": qid, "rank": r + 1, "url": url, "score": float(score[q, r]),
                             "title": title or "No Title",
                             "snippet": (text[:200] + "..." if len(text) > 200 else text) or "No content available",
                             "domain": extract_domain_topic(url), "doc_id": str(int(self._ids[i]))})
                if src is not None:
                    rows[-1]["matched_by"] = MATCHED_BY[int(src[q, r])]
                if i in led:
                    rows[-1]["duplicates"] = led[i]
                if snippets:
                    hit = passages.get((q, r))
                    if hit is not None:
                        rows[-1]["snippet"] = hit[0]
                    rows[-1]["highlights"] = hit[1] if hit is not None else []
                    rows[-1]["missing"] = hit[2] if hit is not None else list(row_names[q] or [])
            if fz is not None or wc is not None or fc is not None or dd is not None or mt is not None:
                corr = fz["corrections"][q] if fz is not None else {}
                rows = _fuzzy.Results(rows, corr, _fuzzy.corrected_text(fz["processed"][q], corr) if fz is not None else None,
                                      wc["expansions"][q] if wc is not None else None,
                                      collapsed=len(dd["drops"][q]) if dd is not None else 0,
                                      match=mt["info"][q] if mt is not None else None)
                if fc is not None:
                    rows.hits, rows.facet_values = int(fc["hits"][q]), int(fc["n_values_hit"][q])
                    rows.facets = _facets.top_list(fc["names"], fc["top_value"][q], fc["top_count"][q])
            out.append(rows)
        return out

    def _duplicates_of(self, drops):
        """One query's drops (int32 [n, 3]: dropped document, leader document, matches) -> {leader document index: the
        "duplicates" entries of its row, in drop order}."""
        ix, led = self.index, {}
        for d, lead, m in drops.tolist():
            led.setdefault(lead, []).append({"doc_id": str(int(self._ids[d])), "url": ix.urls[d] if ix.urls is not None else "",
                                             "title": (ix.titles[d] if ix.titles is not None else "") or "No Title",
                                             "similarity": m / 64.0})
        return led

    @serialised
    def search(self, query, top_k=TOP_K_RETRIEVAL, query_embedding=None, terms=None, query_id=None, within=None,
               mode="lexical", dense_k=DENSE_K, operators=False, must=None, must_not=None, phrases=False, must_phrases=None,
               must_not_phrases=None, proximity=False, snippets=False, snippet_tokens=SNIPPET_TOKENS, fuzzy=False,
               wildcards=False, max_expansions=8, patterns=None, facets=False, facet_by="host", facet_limit=10,
               collapse_duplicates=False, duplicate_threshold=0.9, match="any"):
        """search_batch for one query: must / must_not / must_phrases / must_not_phrases / patterns are ONE list each."""
        one = lambda v: None if v is None else [v]
        opts = SearchOptions(mode, dense_k, operators, phrases, proximity, snippets, snippet_tokens, fuzzy, wildcards, max_expansions,
                             facets, facet_by, facet_limit, collapse_duplicates, duplicate_threshold, match)
        return self._search([query], top_k, one(query_embedding), one(terms), one(query_id), within, opts,
                            Conditions(one(must), one(must_not), one(must_phrases), one(must_not_phrases)), one(patterns))[0]

    @serialised
    def batch_search(self, numbered_queries, query_embeddings=None, term_lists=None, within=None, mode="lexical",
                     dense_k=DENSE_K, operators=False, must=None, must_not=None, phrases=False, must_phrases=None,
                     must_not_phrases=None, proximity=False, snippets=False, snippet_tokens=SNIPPET_TOKENS, fuzzy=False,
                     wildcards=False, max_expansions=8, patterns=None, collapse_duplicates=False, duplicate_threshold=0.9,
                     match="any"):
        """numbered_queries: [(query_num, text)] -> the result entries of search_api.py:276-292 ({query_num, rank, url, score,
        formatted_line}) as a BatchLines sequence: len / indexing / iteration give the reference's dicts, built on access;
        .text() / .write() produce all formatted lines natively (msr_format_lines) without building any.  mode / dense_k:
        search_batch (the entries keep the reference's keys in either mode); operators / must / must_not / phrases /
        must_phrases / must_not_phrases / proximity: search_batch.  snippets=True: every entry gains "snippet" (None where the
        page has no window), "highlights" and "missing" as in search_batch; the formatted lines are what they were.
        fuzzy=True: the returned BatchLines then carries `corrections` (per query {typed term: used term}) and
        `corrected_queries` (per query the corrected text or None); the entries keep their keys.  wildcards / max_expansions /
        patterns: the BatchLines then carries `expansions` (per query {pattern: {...}}).  collapse_duplicates /
        duplicate_threshold: search_batch; the entries and lines are those of the rows that stay, and the BatchLines then
        carries `collapsed` (per query the number of rows dropped) and `duplicates` (per query {leader's url: the
        "duplicates" entries of search_batch}).  match: search_batch; the BatchLines then carries `match` (per query
        {"slots": ..., "need": ...})."""
        opts = SearchOptions(mode, dense_k, operators, phrases, proximity, snippets, snippet_tokens, fuzzy, wildcards, max_expansions,
                             collapse_duplicates=collapse_duplicates, duplicate_threshold=duplicate_threshold, match=match)
        ids, qv, cond, fz, wc, _, mt = self._front([q for _, q in numbered_queries], query_embeddings, term_lists, opts,
                                               Conditions(must, must_not, must_phrases, must_not_phrases), patterns)
        dd = {} if opts.collapse_duplicates else None
        doc, score, _, n = self._final(ids, qv, TOP_K_RETRIEVAL, None, within, opts, cond, fz, wc, None, parsed=True, dedup=dd,
                                       match=mt)
        if self._formatter is None:
            self._formatter = LineFormatter(self.index.urls, self.index.n_docs)
        lines = BatchLines([qn for qn, _ in numbered_queries], doc, score, n, self.index.urls, self._formatter)
        if fz is not None:
            lines.corrections = fz["corrections"]
            lines.corrected_queries = [_fuzzy.corrected_text(p, c) for p, c in zip(fz["processed"], fz["corrections"])]
        if wc is not None:
            lines.expansions = wc["expansions"]
        if mt is not None:
            lines.match = mt["info"]
        if dd is not None:
            url = lambda d: (self.index.urls[d] if self.index.urls is not None else "") or ""
            lines.collapsed = [len(d) for d in dd["drops"]]
            lines.duplicates = [{url(lead): rows for lead, rows in self._duplicates_of(d).items()} for d in dd["drops"]]
        if snippets:
            lines.passages, lines.row_names = self._snippets(self._scored_ids(ids, fz, wc), doc, n, snippet_tokens)
        return lines

    @serialised
    def batch_search_to_file(self, queries_path, out_path, query_embeddings=None, term_lists=None, chunk=None):
        """search_api.py:331-367: queries.txt -> one formatted line per result in out_path; -> number of lines.  (Quotes and
        signs in the file's queries are punctuation here: no operators, no phrases.)  Three things
        run side by side, chunk by chunk: this thread preprocesses / tokenises chunk i + 1 and enqueues it, the GPU ranks
        chunk i, a second host thread waits for chunk i - 1's final rows, formats them (native code, outside the interpreter
        lock) and writes them.  Threads: this thread holds the engine's lock until the second one has drained; the second
        one only waits on events and formats, and takes no lock."""
        import sys
        nq = read_queries_file(queries_path)
        if self._formatter is None:
            self._formatter = LineFormatter(self.index.urls, self.index.n_docs)
        eng = self.engine
        if TOP_K_RETRIEVAL > eng.rerank_max_docs or TOP_K_RETRIEVAL > eng.max_k:
            raise ValueError(f"the batch path needs max_k / rerank_max_docs >= {TOP_K_RETRIEVAL}")
        self._ensure_response_tables()
        texts, nums = [q for _, q in nq], [n for n, _ in nq]
        sub = lambda x, a, b: None if x is None else x[a:b]
        step = int(chunk or max(256, eng.max_queries))
        # two threads hand the interpreter lock back and forth every fraction of a millisecond here; the default switch interval
        # (5 ms) is longer than a whole chunk takes
        old_switch = sys.getswitchinterval()
        sys.setswitchinterval(1e-4)
        try:
            return self._batch_to_file(nq, texts, nums, sub, step, out_path, query_embeddings, term_lists)
        finally:
            sys.setswitchinterval(old_switch)

    def _batch_to_file(self, nq, texts, nums, sub, step, out_path, query_embeddings, term_lists):
        from concurrent.futures import ThreadPoolExecutor
        import torch
        eng, fmt = self.engine, self._formatter
        with open(out_path, "wb") as f, ThreadPoolExecutor(max_workers=1) as pool:
            def consume(a, job):
                doc, score, _, n = self._collect_chunk(job)
                with fmt.lock:                                # (a BatchLines of an earlier request may be formatting with it)
                    f.write(fmt.format(nums[a:a + len(n)], doc, score, n))
                return int(n.sum())
            futs = []
            for i, a in enumerate(range(0, len(nq), step)):
                b = min(len(nq), a + step)
                if i >= 2:
                    futs[i - 2].result()                      # its pinned buffers (slot i & 1) are free again
                ids, qv = self._prepare(texts[a:b], sub(query_embeddings, a, b), sub(term_lists, a, b))
                qv = eng._dev(qv, torch.float32).reshape(-1, 768)
                futs.append(pool.submit(consume, a, self._enqueue_chunk(ids, qv, TOP_K_RETRIEVAL, i & 1)))
            return sum(ft.result() for ft in futs)


class BatchLines:
    """The `results` list of /api/batch_search (search_api.py:276-292, 312-320) over the arrays the device returned: behaves
    like the reference's list of dicts (len, indexing, iteration, equality with a list), but an entry is built when it is
    asked for; the text of all lines comes from the native formatter in one call."""

    def __init__(self, query_nums, doc, score, n, urls, formatter):
        self.query_nums, self.doc, self.score, self.n, self.urls, self._fmt = query_nums, doc, score, n, urls, formatter
        self._start = np.zeros(len(n) + 1, np.int64)
        np.cumsum(n, out=self._start[1:])
        self.passages = self.row_names = None                # Retriever.batch_search(snippets=True) fills them
        self.corrections = self.corrected_queries = None     # ... and fuzzy=True these
        self.expansions = None                               # ... and wildcards=True / patterns= this
        self.collapsed = self.duplicates = None              # ... and collapse_duplicates=True these
        self.match = None                                    # ... and match= this

    def __len__(self):
        return int(self._start[-1])

    def _entry(self, q, r):
        i = int(self.doc[q, r])
        url = (self.urls[i] if self.urls is not None else "") or ""
        sc = float(self.score[q, r])
        qn = self.query_nums[q]
        entry = {"query_num": qn, "rank": r + 1, "url": url, "score": f"{sc:.3f}",
                 "formatted_line": format_result_line(qn, r + 1, url, sc)}
        if self.passages is not None:
            hit = self.passages.get((q, r))
            entry.update(snippet=hit[0] if hit else None, highlights=hit[1] if hit else [],
                         missing=hit[2] if hit else list(self.row_names[q] or []))
        return entry

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[j] for j in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(k)
        q = int(np.searchsorted(self._start, k, side="right") - 1)
        return self._entry(q, int(k - self._start[q]))

    def __iter__(self):
        for q in range(len(self.n)):
            for r in range(int(self.n[q])):
                yield self._entry(q, r)

    def __eq__(self, other):
        return list(self) == list(other)

    def text(self) -> bytes:
        """All formatted lines, each ending in a newline (UTF-8).  A copy: the formatter's buffer is the retriever's, and
        these lines outlive their request."""
        with self._fmt.lock:
            return bytes(self._fmt.format(self.query_nums, self.doc, self.score, self.n))

    def write(self, path):
        with open(path, "wb") as f, self._fmt.lock:
            f.write(self._fmt.format(self.query_nums, self.doc, self.score, self.n))

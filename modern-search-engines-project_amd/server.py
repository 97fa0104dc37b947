"""HTTP facades with the reference's routes and JSON shapes (plumbing, no arithmetic):

    POST /rerank             reranker/reranker_api.py:336-417   (RerankRequest -> RerankResponse, 401 / 500)
    POST /api/search         search_api.py:69-152               ({llm_response, documents:[...]})
    POST /api/batch_search   search_api.py:204-328              (queries.txt -> qnum<TAB>rank<TAB>url<TAB>score lines)
    POST /api/batch_search_file  search_api.py:331-367          (the same, written to batch_search_results.txt)
    POST /api/similar        (no reference counterpart) {doc_ids | doc_id, top_k, sites?, min_score?} -> {documents:[...]}
                             in the /api/search document shape: the pages most like the given ones
                             (Retriever.similar; 400 without ids, 404 for an unknown id)
    GET  /api/health         search_api.py:369-375
    GET  /                   search_api.py:377-380              (the UI page: templates/index.html of the deployment when
                                                                 `ui_dir` is given -- the reference's D3 front end is not
                                                                 part of this build -- else a one-line placeholder)

The reference runs two processes (Flask :5000 + FastAPI :8000) that talk JSON over HTTP; here both sets of
routes sit on one FastAPI app over one Retriever.  The LLM summariser (search_assistant/, a cloud call) is
out of scope: `llm` is an optional callable(query, windows) -> str, otherwise llm_response is "".
Requests may carry `query_embedding` (768 floats) and `terms` (pre-tokenised query) for deployments that
keep the encoder / spaCy in another process.  /api/search also takes `sites` (a list of domains): results only from
documents whose URL's host is one of them or a subdomain (a `site:` search; docset.DocSet.from_sites, restricted inside
the BM25 stage; the sets of the last `site_cache_size` distinct site lists are kept).  The response shape does not change.
Threads: the routes are plain `def` (FastAPI runs them on a thread pool) and the engine is single-threaded; the retriever's
public methods run under the engine's lock (serial.py), and a route that reads the retriever more than once holds the same
lock around all of it.  /api/batch_search_file writes a temporary file and renames it over results_file.
"""
import uuid
from typing import List, Optional, Union

import numpy as np

from .reranker import RerankNotFound
from .serial import lock_of
from .text import extract_domain_topic, preprocess_query, read_queries_file

LLM_MAX_WINDOWS = 10          # config.py:22


def create_app(retriever, llm=None, queries_file="queries.txt", results_file="batch_search_results.txt", ui_dir=None,
               site_cache_size=32):
    import os
    import threading
    import weakref
    from collections import OrderedDict

    from fastapi import FastAPI
    from fastapi.responses import HTMLResponse, JSONResponse
    from pydantic import BaseModel, StrictInt

    class RerankRequest(BaseModel):
        doc_ids: List[str]
        similarities: Optional[List[float]] = None
        query: str
        query_embedding: Optional[List[float]] = None

    class NearSpec(BaseModel):        # a proximity condition in a phrase list (text.Near): the words within a window
        phrase: str
        slop: int = 0                 # other tokens allowed among the words (between the first and the last when ordered)
        ordered: bool = False

    class SearchRequest(BaseModel):
        query: str = ""
        top_k: int = 1000
        query_id: Optional[str] = None
        query_embedding: Optional[List[float]] = None
        terms: Optional[List[str]] = None
        sites: Optional[List[str]] = None
        mode: str = "lexical"         # "hybrid": the dense top dense_k documents join the BM25 candidates (Retriever.search)
        dense_k: int = 100
        operators: bool = False       # `+word` / `-word` in the query: required / excluded words (text.parse_operators)
        must: Optional[List[str]] = None       # terms every result must contain ...
        must_not: Optional[List[str]] = None   # ... and must not contain (Retriever.search)
        phrases: bool = False         # `"a b"` / `-"a b"` in the query: required / excluded phrases (text.parse_phrases)
        # phrases every result must hold, words next to each other (a NearSpec: within a window), and must not hold
        # (Retriever.search; needs a forward index)
        must_phrases: Optional[List[Union[str, NearSpec]]] = None
        must_not_phrases: Optional[List[Union[str, NearSpec]]] = None
        proximity: bool = False       # phrases, and `"a b"~N` / `"a b"~>N`: the words within a window (text.parse_proximity)
        snippets: bool = False        # every row's snippet is the page's best passage for the query, with "highlights" and
        snippet_tokens: int = 30      # "missing" (Retriever.search, DESIGN K14); the passage's width in tokens, 1 .. 64
        fuzzy: bool = False           # a word the vocabulary lacks is replaced by its nearest term (Retriever.search, DESIGN K15);
        #                               the response then carries "corrected_query" and "corrections"
        wildcards: bool = False       # `bibliothek*`, `*bibliothek`, `t?bingen`: a token with `*` / `?` is expanded over the
        max_expansions: int = 8       # vocabulary into at most max_expansions (1 .. 16) scoring terms (Retriever.search, DESIGN
        patterns: Optional[List[str]] = None  # K16); patterns: further patterns; the response then carries "expansions"
        facets: bool = False          # count the WHOLE match set on the device (Retriever.search, DESIGN K17): the response then
        facet_by: str = "host"        # carries "hits", "facets" ([{"value", "count"}], by "host" -- usable as sites=[...] -- or by
        facet_limit: int = 10         # "domain", the first facet_limit (1 .. 64) values) and "facet_values" (distinct values hit)
        collapse_duplicates: bool = False   # near-duplicate pages are shown once (Retriever.search, DESIGN K18): the response then
        duplicate_threshold: float = 0.9    # carries "collapsed"; rows that swallowed copies carry "duplicates"; threshold in (0, 1]
        # "all", a whole number m or a percentage like "75%": only pages that hold all / at least m / that share of the
        # query's words (Retriever.search, DESIGN K19); the response then carries "match": {"slots", "need"}
        match: Union[StrictInt, str] = "any"

    class SimilarRequest(BaseModel):
        doc_ids: Optional[List[Union[int, str]]] = None
        doc_id: Optional[Union[int, str]] = None
        top_k: int = 10
        sites: Optional[List[str]] = None
        min_score: Optional[float] = None

    app = FastAPI(title="Document Reranker API", version="1.0.0")

    # DocSet per normalised list of sites, for the index the retriever serves now: at most `site_cache_size` of them, least
    # recently used first out (an evicted set releases its host mask and its device copy); cleared by an update_index
    site_sets = {"index": lambda: None, "sets": OrderedDict(), "lock": threading.Lock()}   # (routes run on a thread pool)

    def within_sites(sites):
        from .docset import DocSet, normalise_sites
        ix = retriever.index
        key = normalise_sites(sites)
        with site_sets["lock"]:
            if site_sets["index"]() is not ix:   # (an update_index since: the old sets belong to the old index)
                site_sets["index"], site_sets["sets"] = weakref.ref(ix), OrderedDict()
            cache = site_sets["sets"]
            ds = cache.get(key)
            if ds is None:
                ds = cache[key] = DocSet.from_sites(ix, key)
                while len(cache) > max(0, int(site_cache_size)):
                    cache.popitem(last=False)
            else:
                cache.move_to_end(key)
            return ds

    app.state.site_sets = site_sets

    # Routes run on a thread pool and the engine is single-threaded: the facades take the engine's lock per call (serial.py).
    # A route that reads more than one thing of the retriever (the index for the site set, then the search) takes the same
    # re-entrant lock around all of it, so that an update_index falls before or after the request.  Order: the engine's lock
    # first, the site cache's inside it -- never the other way round.  (A retriever without a lock gets the app's own.)
    app_lock = threading.RLock()

    def engine_lock():
        try:
            return lock_of(retriever)
        except AttributeError:
            return app_lock

    @app.post("/rerank")
    def rerank(req: RerankRequest):
        try:
            return retriever.reranker.rerank(req.doc_ids, req.similarities, query=req.query,
                                             query_embedding=req.query_embedding)
        except RerankNotFound as e:
            return JSONResponse(status_code=401, content={"detail": str(e)})
        except Exception as e:
            return JSONResponse(status_code=500, content={"detail": f"Internal server error: {e}"})

    @app.post("/api/search")
    def search(req: SearchRequest):
        try:
            query = preprocess_query(req.query.strip())
            if not query:
                return JSONResponse(status_code=400, content={"error": "Query is required"})
            if req.mode not in ("lexical", "hybrid"):
                return JSONResponse(status_code=400, content={"error": "mode must be 'lexical' or 'hybrid'"})
            qid = req.query_id or uuid.uuid4().hex
            kw = {}
            specs = [p for ps in (req.must_phrases, req.must_not_phrases) for p in ps or () if isinstance(p, NearSpec)]
            wild = req.wildcards or req.patterns is not None
            near = req.proximity or bool(specs)      # a proximity condition the engine cannot hold is the caller's error: 400
            # (feature on, its keywords, its ValueError is the caller's error): only a feature that is on passes its keywords
            features = ((req.mode != "lexical", ("mode", "dense_k"), True),
                        (req.operators or req.must is not None or req.must_not is not None, ("operators", "must", "must_not"), False),
                        (req.phrases or req.must_phrases is not None or req.must_not_phrases is not None,
                         ("phrases", "must_phrases", "must_not_phrases"), False),
                        (near, ("phrases", "proximity", "must_phrases", "must_not_phrases"), True),
                        (req.snippets, ("snippets", "snippet_tokens"), True), (req.fuzzy, ("fuzzy",), True),
                        (wild, ("wildcards", "max_expansions", "patterns"), True),
                        (req.facets, ("facets", "facet_by", "facet_limit"), True),
                        (req.collapse_duplicates, ("collapse_duplicates", "duplicate_threshold"), True),
                        (req.match != "any", ("match",), True))
            for on, names, _ in features:
                if on:
                    kw.update({name: getattr(req, name) for name in names})
            try:
                if near:
                    from .text import Near
                    for name in ("must_phrases", "must_not_phrases"):
                        if kw[name] is not None:
                            kw[name] = [Near(p.phrase, p.slop, p.ordered) if isinstance(p, NearSpec) else p for p in kw[name]]
                with engine_lock():                           # the site set and the search: of ONE index
                    if req.sites is not None:
                        kw["within"] = within_sites(req.sites)
                    docs = retriever.search(req.query, top_k=req.top_k, query_embedding=req.query_embedding,
                                            terms=req.terms, query_id=qid, **kw)
            except ValueError as e:
                if not any(on and bad_request for on, _, bad_request in features):
                    raise
                # a dense_k the engine cannot hold; fuzzy / wildcards on an index without term strings; max_expansions outside
                # 1 .. 16; a required or excluded pattern; a facet_by the engine does not know, a facet_limit outside 1 .. 64;
                # a duplicate_threshold outside (0, 1]; a match value that is none
                return JSONResponse(status_code=400, content={"error": str(e)})
            llm_response = ""
            if llm is not None and docs:
                llm_response = llm(query, [d["snippet"] for d in docs[:LLM_MAX_WINDOWS]])
            if req.fuzzy or wild or req.facets or req.collapse_duplicates or req.match != "any":
                out = {"llm_response": llm_response, "documents": list(docs)}
                if req.match != "any":
                    out.update(match=docs.match)
                if req.collapse_duplicates:
                    out.update(collapsed=docs.collapsed)
                if req.facets:
                    out.update(hits=docs.hits, facets=docs.facets, facet_values=docs.facet_values)
                if req.fuzzy:
                    out.update(corrected_query=docs.corrected_query, corrections=docs.corrections)
                if wild:
                    out.update(expansions=docs.expansions)
                return out
            return {"llm_response": llm_response, "documents": docs}
        except Exception:
            return JSONResponse(status_code=500, content={"error": "Internal server error"})

    @app.post("/api/similar")
    def similar(req: SimilarRequest):
        # pages like the given ones (Retriever.similar): the sources themselves are left out; 400 without ids, 404 for an id the
        # index does not hold
        try:
            ids = list(req.doc_ids or []) + ([] if req.doc_id is None else [req.doc_id])
            if not ids:
                return JSONResponse(status_code=400, content={"error": "doc_ids is required"})
            try:
                ids = [int(d) for d in ids]
            except (TypeError, ValueError):
                return JSONResponse(status_code=400, content={"error": "doc_ids must be integers"})
            with engine_lock():                               # the site set, the search and the texts: of ONE index
                within = None if req.sites is None else within_sites(req.sites)
                try:
                    rows = retriever.similar(ids, top_k=req.top_k, within=within, min_score=req.min_score)
                except LookupError as e:
                    return JSONResponse(status_code=404, content={"error": str(e)})
                ix = retriever.index
                texts = [_doc_text(ix, r["doc_id"]) for r in rows]
            docs = []
            for r, text in zip(rows, texts):
                url = r["url"] or ""
                docs.append({"query_id": None, "rank": r["rank"], "url": url, "score": r["score"],
                             "title": r["title"] or "No Title",
                             "snippet": (text[:200] + "..." if len(text) > 200 else text) or "No content available",
                             "domain": extract_domain_topic(url), "doc_id": str(r["doc_id"]),
                             "source_doc_id": str(r["source_doc_id"])})
            return {"documents": docs}
        except Exception as e:
            return JSONResponse(status_code=500, content={"error": f"Internal server error: {e}"})

    def _doc_text(ix, doc_id):
        if ix.texts is None:
            return ""
        i = int(np.searchsorted(retriever._ids, doc_id))
        return ix.texts[i] or ""

    def _batch():
        """-> (status, body): the body of /api/batch_search (search_api.py:204-328)."""
        try:
            try:
                queries = read_queries_file(queries_file)
            except FileNotFoundError:
                return 404, {"error": "queries.txt file not found"}
            if not queries:
                return 400, {"error": "No valid queries found in queries.txt"}
            results = retriever.batch_search(queries)
            return 200, {"total_queries": len(queries), "total_results": len(results), "results": list(results), "_lines": results,
                         "queries_processed": [{"query_num": n, "query_text": t} for n, t in queries]}
        except Exception as e:
            return 500, {"error": f"Internal server error: {e}"}

    @app.post("/api/batch_search")
    def batch_search():
        status, body = _batch()
        body.pop("_lines", None)
        return body if status == 200 else JSONResponse(status_code=status, content=body)

    @app.post("/api/batch_search_file")
    def batch_search_file():
        # search_api.py:331-367: run the batch search, pass its error through unchanged, else write one formatted line per
        # result and report where they went
        try:
            status, body = _batch()
            if status != 200:
                return JSONResponse(status_code=status, content=body)
            lines = body.get("_lines")
            # into a temporary file beside the target, then renamed over it: two requests at once leave one request's lines,
            # and a reader sees a complete file or none
            path = os.fspath(results_file)
            tmp = f"{path}.{uuid.uuid4().hex}.tmp"
            try:
                if hasattr(lines, "write"):                   # Retriever.batch_search: all lines formatted natively in one call
                    lines.write(tmp)
                else:
                    with open(tmp, "w", encoding="utf-8") as f:
                        for r in body["results"]:
                            f.write(r["formatted_line"] + "\n")
                os.replace(tmp, path)
            except BaseException:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise
            return {"message": f"Results saved to {results_file}", "total_queries": body["total_queries"],
                    "total_results": body["total_results"], "output_file": str(results_file),
                    "format": "query_num<tab>rank<tab>url<tab>score per line"}
        except Exception as e:
            return JSONResponse(status_code=500, content={"error": f"Internal server error: {e}"})

    @app.get("/", response_class=HTMLResponse)
    def index():
        page = os.path.join(ui_dir, "templates", "index.html") if ui_dir else None
        if page and os.path.exists(page):
            with open(page, encoding="utf-8") as f:
                return f.read()
        return "<html><body><p>msretr search API: POST /api/search, /api/batch_search, /api/batch_search_file, /rerank</p></body></html>"

    @app.get("/api/health")
    def health():
        return {"status": "healthy", "search_engine_ready": retriever is not None}

    return app

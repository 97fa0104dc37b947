"""The query options together, against the composed CPU oracle (options_ref.py over options_cases.py):
Retriever.search_batch and search for every batch of the table in both modes and under both settings of diversification,
one search_batch call of 525 queries (three chunks: both pinned slots are reused) with the collapse on, a final list longer
than the columns that are copied back, the BM25.search facade,
and /api/search.  Everything but the scores is compared exactly; the scores within the rerank parity bar."""
from dataclasses import replace
from functools import lru_cache

import numpy as np
import pytest
import torch

import options_ref as ref
from msretr.docset import DocSet
from msretr.retriever import Retriever
from msretr.text import Near
from options_cases import BATCHES, BIG_SITES, WIDE, WIDE_TOP, call_kwargs, crawl, masks

pytestmark = pytest.mark.gpu
PARITY_BAR = 5e-6            # bench.py's rerank_parity
EXTRAS = ("collapsed", "corrections", "corrected_query", "expansions", "hits", "facets", "facet_values")
B = range(len(BATCHES))


@pytest.fixture(scope="module")
def site():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    c = crawl()
    r = Retriever(indexer=c.ix, max_queries=8, max_k=1000)
    within = [[None if m is None else DocSet.from_mask(c.ix, m) for m in masks(c, b)] for b in BATCHES]
    yield c, r, within
    r.engine.close()


@lru_cache(maxsize=None)
def want(b, mode, div):
    """The oracle's answers, once per (batch, mode, diversification) for the whole module."""
    return ref.expected(crawl(), BATCHES[b], mode, div)


def _same(got, exp, what):
    """One query: a result of the engine against evaluate()'s answer."""
    assert [row["doc_id"] for row in got] == [row["doc_id"] for row in exp["rows"]], what
    worst = max((abs(g["score"] - w["score"]) for g, w in zip(got, exp["rows"])), default=0.0)
    print(what, "rows", len(got), "max score difference %.3e" % worst)
    assert worst <= PARITY_BAR, (what, worst)
    for rank, (g, w) in enumerate(zip(got, exp["rows"])):
        assert g["rank"] == rank + 1
        for key in ("matched_by", "duplicates", "snippet", "highlights", "missing"):
            assert g.get(key) == w.get(key) and (key in g) == (key in w), (what, rank, key, g.get(key), w.get(key))
    for name in EXTRAS:
        assert getattr(got, name) == exp[name], (what, name, getattr(got, name), exp[name])


def _equal(a, b, what):
    """Two results of the engine: the same rows, bit for bit, and the same extras."""
    assert list(a) == list(b), what
    for name in EXTRAS:
        assert getattr(a, name) == getattr(b, name), (what, name)


@pytest.mark.parametrize("div", [True, False], ids=["diversified", "plain"])
@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
@pytest.mark.parametrize("b", B, ids=[x.name for x in BATCHES])
def test_search_batch_and_search_against_the_oracle(site, b, mode, div):
    c, r, within = site
    batch = BATCHES[b]
    old = r.reranker.cfg["diversification"]
    r.reranker.cfg["diversification"] = div
    try:
        got = r.search_batch(batch.queries, mode=mode, **call_kwargs(c, batch, within=within[b]))
        assert len(got) == len(batch.queries)
        for q, exp in enumerate(want(b, mode, div)):
            _same(got[q], exp, (batch.name, mode, div, q))
        for q in range(len(batch.queries)):
            one = r.search(batch.queries[q], mode=mode, **call_kwargs(c, batch, q, within=within[b][q]))
            _equal(one, got[q], (batch.name, mode, div, q, "one by one"))
    finally:
        r.reranker.cfg["diversification"] = old


def test_collapse_across_chunk_boundaries(site):
    """525 queries in ONE search_batch call: chunks of 256, 256 and 13, so the pinned buffers of slot 0 (final rows, candidates,
    drops) are written again while chunk 1 is still pending.  Collapse, hybrid, facets, fuzzy and snippets are on.  The list
    is 75 repetitions of SEVEN cases: 256 is no multiple of 7, so a row of a pinned buffer holds another case in every chunk
    and a chunk read from the wrong slot, or after its slot was written again, cannot go unnoticed.  Every repetition equals
    its first occurrence and the oracle."""
    c, r, within = site
    b, reps = 2, 75
    batch = BATCHES[b]
    assert batch.switches["collapse_duplicates"] and batch.switches["facets"] and batch.switches["fuzzy"]
    cases = [q for q in range(len(batch.queries)) if q != 5]
    n = len(cases)
    assert 256 % n and n * reps >= 520 and r.engine.max_queries <= 256
    rep = lambda xs: [xs[q] for q in cases] * reps
    kw = call_kwargs(c, batch, within=rep(within[b]))
    kw.update(query_embeddings=np.tile(kw["query_embeddings"][cases], (reps, 1)), term_lists=rep(kw["term_lists"]))
    kw.update({k: rep(v) for k, v in batch.lists.items()})
    got = r.search_batch(rep(batch.queries), mode="hybrid", **kw)
    assert len(got) == n * reps
    exp = want(b, "hybrid", True)
    assert sum(exp[q]["collapsed"] > 0 for q in cases) >= 4
    for i, q in enumerate(cases):
        _same(got[i], exp[q], ("chunks", q))
    for i in range(n, n * reps):
        _equal(got[i], got[i % n], ("chunks", i))


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_a_final_list_longer_than_the_copied_columns_with_drops(site, mode):
    """_collect_chunk copies FINAL_COLS columns per query back through pinned buffers; a chunk with a longer list comes back
    in full from the device.  With the reranker's top_k raised and diversification off the wide case keeps about 150 rows --
    with the collapse on, so the drops travel beside the full copy -- and its neighbour in the chunk a few dozen."""
    c, r, _ = site
    old = dict(r.reranker.cfg)
    r.reranker.cfg.update(top_k=WIDE_TOP, diversification=False)
    try:
        got = r.search_batch(WIDE.queries, mode=mode, **call_kwargs(c, WIDE, within=None))
        exp = ref.expected(c, WIDE, mode, False, WIDE_TOP)
        assert len(got[0]) > Retriever.FINAL_COLS > len(got[1]) > 0 and got[0].collapsed > 0
        for q in range(2):
            _same(got[q], exp[q], (WIDE.name, mode, q))
    finally:
        r.reranker.cfg.clear()
        r.reranker.cfg.update(old)


@pytest.mark.parametrize("b", B, ids=[x.name for x in BATCHES])
def test_bm25_search_facade_against_the_oracle(site, b):
    """BM25.search with operators, phrases, proximity, fuzzy, wildcards, lists and within on the same cases: the documents of
    the oracle's BM25 list inside the oracle's set, and its scores as float64, exactly."""
    c, r, within = site
    batch, sw = BATCHES[b], BATCHES[b].switches
    some = 0
    for q, text in enumerate(batch.queries):
        kw = {k: sw[k] for k in ("operators", "proximity", "fuzzy", "wildcards", "max_expansions") if k in sw}
        kw.update({k: v[q] for k, v in batch.lists.items()})
        got = r.bm25.search(text, top_k=sw["top_k"], within=within[b][q], **kw)
        rows, corrections, expansions = ref.bm25_search(c, batch, q)
        assert [(row["doc_id"], row["score"]) for row in got] == rows, (batch.name, q)
        assert sw["fuzzy"]                                   # (so every answer is a fuzzy.Results: the attributes are read as they are)
        assert got.corrections == corrections and got.expansions == expansions, (batch.name, q)
        some += len(rows) > 0
    assert some >= 5


def test_http_search_with_every_option_on(site):
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    c, r, _ = site
    batch = BATCHES[0]
    sw = batch.switches
    body = {"query": batch.queries[0], "query_id": "q0", "query_embedding": ref.plans(c, batch)[0].vector.tolist(), "mode": "hybrid",
            "sites": BIG_SITES, "must": ["essen"], "must_not": ["geschlossen"],
            "must_phrases": ["alte aula", {"phrase": "morgens abends", "slop": 1, "ordered": True}, {"phrase": "kuchen kaffee", "slop": 1}],
            "must_not_phrases": ["kein zutritt"], "patterns": ["uni*"]}
    body.update(sw)
    resp = TestClient(create_app(r)).post("/api/search", json=body)
    assert resp.status_code == 200, resp.text
    out = resp.json()
    kw = dict(sw, must=body["must"], must_not=body["must_not"], must_not_phrases=body["must_not_phrases"], patterns=body["patterns"],
              must_phrases=["alte aula", Near("morgens abends", 1, ordered=True), Near("kuchen kaffee", 1)])
    one = r.search(body["query"], query_embedding=np.asarray(body["query_embedding"], np.float32), query_id="q0", mode="hybrid",
                   within=DocSet.from_sites(c.ix, BIG_SITES), **kw)
    assert out["documents"] == [dict(row) for row in one] and len(one) > 0
    assert any("duplicates" in row for row in one) and all("highlights" in row and "matched_by" in row for row in one)
    for name, key in (("collapsed", "collapsed"), ("hits", "hits"), ("facets", "facets"), ("facet_values", "facet_values"),
                      ("corrected_query", "corrected_query"), ("corrections", "corrections"), ("expansions", "expansions")):
        assert out[key] == getattr(one, name), name
    assert one.collapsed > 0 and one.hits > 0 and one.corrections == {"mensaa": "mensa"} and set(one.expansions) == {"biblio*", "uni*"}
    # ... which is the table's everything-on case with one more pattern: the oracle's answer to that
    assert DocSet.from_sites(c.ix, BIG_SITES).mask.tolist() == masks(c, batch)[0].tolist()
    plan = ref.plans(c, batch)[0]
    _same(one, ref.evaluate(c, replace(plan, patterns=plan.patterns + ("uni*",)), "hybrid", True), "http")

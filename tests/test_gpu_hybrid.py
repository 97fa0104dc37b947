"""Hybrid candidates on the GPU (msr_bm25_score_docs, msr_union_candidates, mode="hybrid" of the Retriever; DESIGN K10):
point scores against the oracle bit for bit on every lookup branch, agreement with the streaming kernel (K1), the union
against tests/hybrid_ref.py, the whole hybrid step against the same GPU calls composed by hand (bit for bit) and against
the CPU chain (within the rerank parity bar), the point of the feature (a document without a query term is found), the
default that did not move, within=, update_index and the HTTP route."""
import numpy as np
import pytest
import torch

import hybrid_ref as H
from msretr.docset import DocSet
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import remove_documents
from msretr.retriever import Retriever, hybrid_k_lex
from msretr.synthetic import synthetic_corpus, synthetic_queries
from oracle import bm25_ref
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

RERANK_BAR = 5e-6          # the rerank parity bar of tests/test_gpu_parity.py / test_gpu_within.py against oracle.rerank_ref
DENSE_TOL = 1e-5           # the project's stated dense tolerance


def _z(ix):
    z = {k: _np(getattr(ix, k)) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")}
    z["avgdl"] = ix.avgdl
    return z


def _cpu(*xs):
    return [x.cpu().numpy() for x in xs]


# ------------------------------------------------------------------------------------------------ 1. point scores
N1 = 5 * 1024 + 13                                             # not a multiple of the 1024-document tile
HEAVY, MAX_DENSE = 2048, 64                                    # MSR_BM25_HEAVY_DF, MSR_BM25_MAX_DENSE


def _branch_corpus():
    """Posting lists of every class the point kernel distinguishes: 71 negative-idf lists of >= 2048 postings (64 get a dense
    table, the 7 shortest do not), positive lists of >= 2048 (skip table), of 65 .. 2047 and of <= 64 postings."""
    rng = np.random.default_rng(5)
    df = [int(0.8 * N1)] + [2600 + 10 * i for i in range(1, 71)]            # terms 0 .. 70: df > N / 2
    df += [2048, 2100, 2400]                                                # 71 .. 73: positive idf, skip table
    df += [65, 200, 1000, 2047]                                             # 74 .. 77: binary search of the whole list
    df += [1, 2, 10, 64]                                                    # 78 .. 81
    df += [int(x) for x in rng.integers(1, 300, 118)]                       # 82 .. 199: filler
    V = len(df)
    post_doc = [np.sort(rng.choice(N1, size=f, replace=False)).astype(np.int32) for f in df]
    post_doc[78] = np.array([N1 - 1], np.int32)                             # the last document's own term
    post_doc[79] = np.array([0, 1024], np.int32)                            # the first document, and a tile's first
    term_off = np.zeros(V + 1, np.int64)
    term_off[1:] = np.cumsum([len(p) for p in post_doc])
    dff = np.array(df, np.float64)
    idf = np.log10((N1 - dff + 0.5) / (dff + 0.5)).astype(np.float32)
    pd_ = np.concatenate(post_doc)
    ix = CorpusIndex(doc_ids=np.arange(N1, dtype=np.int64) * 3 + 7, doc_len=rng.integers(5, 400, N1).astype(np.int32),
                     term_off=term_off, post_doc=pd_, post_tf=rng.integers(1, 6, len(pd_)).astype(np.int32), idf=idf,
                     avgdl=190.5, total_docs=N1)
    return ix, np.array(df), idf


def _classes(df, idf):
    """The bind rules restated (msr_engine.hip): skip-table rows for lists >= 2048; dense tables for the <= 64 longest of those
    with negative idf."""
    heavy = df >= HEAVY
    neg_heavy = [t for t in np.argsort(-df, kind="stable") if heavy[t] and idf[t] < 0]
    table = set(int(t) for t in neg_heavy[:MAX_DENSE])
    return heavy, table, set(int(t) for t in neg_heavy[MAX_DENSE:])


def _check_points(eng, z, queries, docs, doc_n):
    score, touched = _cpu(*eng.bm25_score_docs(queries, docs, doc_n))
    N = len(z["doc_len"])
    for q, terms in enumerate(queries):
        n = docs.shape[1] if doc_n is None else int(doc_n[q])
        ws, wt = H.point_scores(z, terms, docs[q, :n])
        assert score[q, :n].tolist() == ws.tolist(), q
        assert touched[q, :n].tolist() == wt.astype(np.int32).tolist(), q
        assert (score[q, n:] == 0).all() and (touched[q, n:] == 0).all(), q
    return score, touched


def test_point_scores_every_lookup_branch_bit_for_bit():
    ix, df, idf = _branch_corpus()
    heavy, table, neg_no_table = _classes(df, idf)
    V = len(df)
    # the corpus takes every branch (checked here, on the CPU)
    assert N1 % 1024 != 0
    assert any(df[t] > N1 / 2 and df[t] >= HEAVY for t in table) and len(table) == MAX_DENSE
    assert len(neg_no_table) == 7 and all(idf[t] < 0 and heavy[t] for t in neg_no_table)
    assert any(heavy[t] and idf[t] > 0 for t in (71, 72, 73))
    assert all(65 <= df[t] <= 2047 for t in (74, 75, 76, 77)) and all(df[t] <= 64 for t in (78, 79, 80, 81))
    z = _z(ix)
    no_tab = sorted(neg_no_table)
    queries = [
        [0, 71, 76, 81, 0, 71, 71],                              # repeated terms: qtf 2 and 3
        [-1, V + 5, 3, 77, -7, V],                               # unknown terms < 0 and >= V
        list(range(0, 40)) + list(range(66, 90)),                # 64 unique terms, every class
        [-5, V + 1],                                             # no valid term
        [],                                                      # no term at all
        no_tab[:3] + [72, 74, 79, 78] + no_tab[3:],               # negative lists without a table, around positive ones
        [78, 79, 80],                                            # rare terms only: most documents hold none of them
        [73, 0, 75, 5, 80, 73],
    ]
    assert len(set(queries[2])) == 64 and set(queries[2]) & neg_no_table and set(queries[2]) & table
    Q, M = len(queries), 48
    rng = np.random.default_rng(6)
    docs = rng.integers(0, N1, (Q, M)).astype(np.int32)
    docs[:, :8] = [0, N1 - 1, 1023, 1024, 2047, 2048, 5 * 1024 - 1, 5 * 1024]   # first / last document, tile edges
    docs[:, 8:11] = docs[:, 11:12]                               # a document repeated in a row
    docs[:, 12] = -1; docs[:, 13] = N1; docs[:, 14] = 2 ** 31 - 1               # no document of the index: 0.0 / 0
    lacking = np.setdiff1d(np.arange(N1), np.concatenate([z["post_doc"][z["term_off"][t]:z["term_off"][t + 1]] for t in (78, 79, 80)]))
    docs[6, 20:30] = lacking[:10]                                # documents holding none of the query's terms
    doc_n = np.array([M, M, M, M, M, 17, M, 0], np.int32)         # rows filled to max_docs, a short row, doc_n = 0
    eng = DeviceEngine(ix, max_queries=4, max_k=100)
    try:
        score, touched = _check_points(eng, z, queries, docs, doc_n)
        assert (touched[6, 20:30] == 0).all() and (score[6, 20:30] == 0).all()
        assert (score[0, 8:11] == score[0, 11]).all() and (touched[3] == 0).all() and (touched[4] == 0).all()
        assert touched[:3].any() and (score[:3] < 0).any() and (score[:3] > 0).any()
        assert (score[:, 12:15] == 0).all() and (touched[:, 12:15] == 0).all()
        _check_points(eng, z, queries, docs, None)               # doc_n = NULL: every slot
        # the score the streaming kernel returns for the same (query, document)
        for ms in (0.0, -1e9):
            d, s, n = _cpu(*eng.bm25_topk(queries, k=100, min_score=ms))
            ps, pt = _cpu(*eng.bm25_score_docs(queries, d, n))
            for q in range(Q):
                assert ps[q, :n[q]].tolist() == s[q, :n[q]].tolist() and (pt[q, :n[q]] == 1).all(), (q, ms)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["bm25_random_a", "bm25_random_b"])
def test_point_scores_on_the_golden_indices(golden_dir, name):
    import json
    import os
    z = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    meta = json.load(open(os.path.join(golden_dir, name + ".json"), encoding="utf-8"))
    ix = CorpusIndex(doc_ids=z["doc_ids"], doc_len=z["doc_len"], term_off=z["term_off"], post_doc=z["post_doc"],
                     post_tf=z["post_tf"], idf=z["idf"], avgdl=float(z["avgdl"]), total_docs=int(z["total_docs"]))
    queries = [q["terms"] for q in meta["queries"]][:40]
    N = len(z["doc_ids"])
    rng = np.random.default_rng(1)
    docs = rng.integers(0, N, (len(queries), 64)).astype(np.int32)
    docs[:, 0], docs[:, 1] = 0, N - 1
    eng = DeviceEngine(ix, max_queries=8, max_k=1000)
    try:
        _check_points(eng, z, queries, docs, None)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. agreement with K1
@pytest.fixture(scope="module")
def big():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = synthetic_corpus(50_021, n_chunks=120_000, n_terms=20_000, seed=21)
    terms, qv = synthetic_queries(ix, 256, seed=22, lo_rank=5, hi_rank=8000)
    return ix, terms, qv.numpy()


def live_count(n):
    return int(n.astype(np.int64).sum())


def test_point_scores_equal_the_streaming_kernel(big):
    ix, terms, _ = big
    assert ix.n_docs >= 50_000 and len(terms) == 256 and all(0 in t for t in terms)      # the city term in every query
    eng = DeviceEngine(ix, max_queries=64, max_k=1000)
    try:
        d, s, n = eng.bm25_topk(terms, k=1000)
        ps, pt = eng.bm25_score_docs(terms, d, n)
        d, s, n, ps, pt = _cpu(d, s, n, ps, pt)
        assert n.max() == 1000 and live_count(n) > 100_000
        live = np.arange(1000)[None, :] < n[:, None]
        assert np.array_equal(ps[live].view(np.int64), s[live].view(np.int64)) and (pt[live] == 1).all()
        assert (ps[~live] == 0).all() and (pt[~live] == 0).all()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. union
def _random_lists(rng, Q, k_lex, k_dense, overlap, n_docs=100_000):
    ld = np.full((Q, k_lex), -1, np.int32); ls = np.full((Q, k_lex), -np.inf); ln = np.zeros(Q, np.int32)
    dd = np.full((Q, k_dense), -1, np.int32); db = np.zeros((Q, k_dense)); dn = np.zeros(Q, np.int32)
    for q in range(Q):
        nl, nd = int(rng.integers(0, k_lex + 1)), int(rng.integers(0, k_dense + 1))
        if q == 0: nl, nd = k_lex, k_dense
        if q == 1: nl = 0
        if q == 2: nd = 0
        pool = rng.choice(n_docs, size=nl + nd, replace=False).astype(np.int32)
        ld[q, :nl], ls[q, :nl], ln[q] = pool[:nl], -np.sort(-rng.standard_normal(nl)), nl
        own = pool[nl:]
        if overlap == 1.0:
            own = rng.choice(pool[:nl], size=nd, replace=nd > nl) if nl else own
        elif overlap > 0 and nl:
            take = rng.random(nd) < overlap
            own = np.where(take, rng.choice(pool[:nl], size=nd), own)
        dd[q, :nd], db[q, :nd], dn[q] = own, rng.standard_normal(nd), nd
        if q % 3 == 0 and nd > 4 and overlap < 1.0:
            dd[q, 1] = -1                                        # a -1 inside the list
            dd[q, 3] = dd[q, 0]                                  # a repeat
    return ld, ls, ln, dd, db, dn


@pytest.mark.parametrize("k_lex,k_dense", [(900, 100), (512, 512), (1, 1023), (1000, 24), (37, 5)])
def test_union_against_the_cpu_helper(k_lex, k_dense):
    ix = synthetic_corpus(3000, n_chunks=0, n_terms=500, seed=2)
    eng = DeviceEngine(ix, max_queries=8, max_k=1000)
    rng = np.random.default_rng(k_lex * 7 + k_dense)
    try:
        for overlap in (0.0, 0.4, 1.0):
            ld, ls, ln, dd, db, dn = _random_lists(rng, 12, k_lex, k_dense, overlap)
            for max_cand in (k_lex + k_dense, k_lex + k_dense + 9):
                doc, score, src, n = _cpu(*eng.union_candidates((ld, ls, ln), dd, db, dn, max_cand=max_cand))
                want = [H.union_list(ld[q, :ln[q]], ls[q, :ln[q]], dd[q, :dn[q]], db[q, :dn[q]]) for q in range(len(ln))]
                wd, ws, wsrc, wn = H.pad_lists(want, max_cand)
                assert n.tolist() == wn.tolist() and np.array_equal(doc, wd) and np.array_equal(src, wsrc)
                assert np.array_equal(score.view(np.int64), ws.view(np.int64))
            if overlap == 1.0:
                assert (src[ln > 0] != 2).all()
            if overlap == 0.0:
                assert (src != 3).all()
        with pytest.raises(Exception, match="msr_union_candidates"):     # max_cand too small: refused, nothing launched
            eng.union_candidates((ld, ls, ln), dd, db, dn, max_cand=k_lex + k_dense - 1)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4-7. the hybrid step
NH, DENSE_K, QH = 20_013, 40, 24


def _planted(ix, qv, dense_k, seed):
    """Unit rows with planted gaps: query i gets dense_k documents of its own whose FIRST chunk row has cosine 0.5 + 0.004 j to
    it (j = 0 .. dense_k - 1); every other row of the corpus is a random unit vector (cosine ~ N(0, 1/768), far below 0.5).
    -> the planted documents [Q, dense_k], best first."""
    rng = np.random.default_rng(seed)
    emb, off = _np(ix.emb), _np(ix.doc_off).astype(np.int64)
    Q = len(qv)
    docs = rng.choice(np.arange(100, ix.n_docs - 100), size=(Q, dense_k), replace=False)
    for i in range(Q):
        q = qv[i].astype(np.float64); q /= np.linalg.norm(q)
        for j in range(dense_k):
            c = 0.5 + 0.004 * (dense_k - 1 - j)
            r = rng.standard_normal(768); r -= (r @ q) * q; r /= np.linalg.norm(r)
            emb[off[docs[i, j]]] = (c * q + np.sqrt(1 - c * c) * r).astype(np.float32)
    ix.emb = torch.as_tensor(emb)
    return docs


def _with_urls(ix):
    ids = _np(ix.doc_ids)
    ix.urls = [None if d % 97 == 0 else f"https://h{d % 41}.example.org/doc{int(ids[d])}" for d in range(ix.n_docs)]
    ix.titles = [f"title {d}" for d in range(ix.n_docs)]
    ix.texts = [f"text of document {d} " * 3 for d in range(ix.n_docs)]
    ix._url_group = None
    return ix


@pytest.fixture(scope="module")
def hyb():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = synthetic_corpus(NH, n_chunks=60_000, n_terms=6000, seed=31)
    terms, qv = synthetic_queries(ix, QH, seed=32, lo_rank=5, hi_rank=3000)
    qv = qv.numpy().copy()
    planted = _planted(ix, qv, DENSE_K, 33)
    terms = [list(t) for t in terms]
    terms[3] = [-1, -2]                                          # a query of unknown words only
    _with_urls(ix)
    eng = DeviceEngine(ix, max_queries=64, max_k=1000, rerank_max_docs=1000)
    r = Retriever(indexer=eng)
    yield ix, terms, qv, planted, r
    eng.close()


def _compose(r, terms, qv, top_k, dense_k, within=None, score_on="oracle"):
    """The hybrid step from the existing GPU calls: bm25_topk, dense_topk, numpy union (oracle scores for the dense list),
    rerank_gather / rerank_fuse / diversify.  -> (doc, score, chunk, n) host arrays [Q, M], and the union's (doc, src, n)."""
    eng, cfg = r.engine, r.reranker.cfg
    z = _z(r.index)
    k_lex = hybrid_k_lex(top_k, eng.rerank_max_docs, dense_k)
    r._ensure_response_tables()
    ld, ls, ln = _cpu(*eng.bm25_topk(terms, k=k_lex, within=within))
    dense = eng.dense_topk(qv, k=dense_k, want_chunk=False, within=within)
    dd, dn = _cpu(dense[0], dense[3])
    lists = []
    for q in range(len(terms)):
        ds, _ = H.point_scores(z, terms[q], dd[q, :dn[q]])
        lists.append(H.union_list(ld[q, :ln[q]], ls[q, :ln[q]], dd[q, :dn[q]], ds))
    cd, cs, csrc, cn = H.pad_lists(lists, k_lex + dense_k)
    q_dev = torch.as_tensor(qv).to(eng.device)
    cos, meta = eng.rerank_gather(q_dev, cd, cn, max_chunks=10)
    fused = eng.rerank_fuse(cd, cs, cn, cos, meta, smoothing=cfg["smoothing"], max_chunks=10)
    fin = eng.diversify(fused, top_k=int(cfg["top_k"]), diversification=bool(cfg.get("diversification", False)))
    doc, score, _, chunk, n = _cpu(*fin)
    return (doc, score, chunk, n), (cd, cs, csrc, cn)


def _same_lists(got, want):
    doc, score, chunk, n = got[:4]
    wd, ws, wc, wn = want
    assert n.tolist() == wn.tolist()
    for q in range(len(n)):
        k = int(n[q])
        assert doc[q, :k].tolist() == wd[q, :k].tolist(), q
        assert score[q, :k].tobytes() == ws[q, :k].tobytes(), q
        assert chunk[q, :k].tolist() == wc[q, :k].tolist(), q


def test_hybrid_step_equals_its_parts_bit_for_bit(hyb):
    ix, terms, qv, planted, r = hyb
    for top_k, dense_k in ((1000, DENSE_K), (1000, 100), (200, 7)):
        got = r.final_lists(terms, qv, top_k, mode="hybrid", dense_k=dense_k, with_source=True)
        want, (cd, cs, csrc, cn) = _compose(r, terms, qv, top_k, dense_k)
        _same_lists(got, want)
        assert got[3].max() > 0 and got[3][3] > 0                 # the unknown-words query has results too
        for q in range(len(terms)):                               # the source of every final row
            look = dict(zip(cd[q, :cn[q]].tolist(), csrc[q, :cn[q]].tolist()))
            assert got[4][q, :got[3][q]].tolist() == [look[d] for d in got[0][q, :got[3][q]].tolist()]
    # the device union inside the step is the numpy union
    eng = r.engine
    _, (cd, cs, csrc, cn) = _compose(r, terms, qv, 1000, DENSE_K)
    k_lex = hybrid_k_lex(1000, eng.rerank_max_docs, DENSE_K)
    lex = eng.bm25_topk(terms, k=k_lex)
    dd, _, _, dn = eng.dense_topk(qv, k=DENSE_K, want_chunk=False)
    u = _cpu(*eng.union_candidates(lex, dd, eng.bm25_score_docs(terms, dd, dn)[0], dn))
    assert np.array_equal(u[0], cd) and np.array_equal(u[1].view(np.int64), cs.view(np.int64)) and np.array_equal(u[2], csrc)
    assert u[3].tolist() == cn.tolist()


def test_hybrid_step_against_the_cpu_chain(hyb):
    ix, terms, qv, planted, r = hyb
    eng, cfg = r.engine, r.reranker.cfg
    z, emb, off = _z(ix), _np(ix.emb), _np(ix.doc_off).astype(np.int64)
    # the dense stage may swap documents whose cosines lie within 1e-5 at the dense_k-th place: here, in float64, the gap
    # between the dense_k-th and the next document's cosine exceeds 2e-5 for EVERY query
    e64 = emb.astype(np.float64)
    e64 /= np.linalg.norm(e64, axis=1, keepdims=True)
    for i in range(QH):
        q64 = qv[i].astype(np.float64); q64 /= np.linalg.norm(q64)
        best = np.maximum.reduceat(e64 @ q64, off[:-1])
        top = np.sort(best)[::-1]
        assert top[DENSE_K - 1] - top[DENSE_K] > 2 * DENSE_TOL, i
        assert len(set(np.argsort(-best)[:DENSE_K].tolist()) & set(planted[i].tolist())) >= DENSE_K - 1
    got = r.final_lists(terms, qv, 1000, mode="hybrid", dense_k=DENSE_K)
    oe = OracleEngine(ix)
    lists = [H.candidates(z, emb, off, terms[q], qv[q], 1000, eng.rerank_max_docs, DENSE_K) for q in range(QH)]
    cd, cs, _, cn = H.pad_lists(lists, hybrid_k_lex(1000, eng.rerank_max_docs, DENSE_K) + DENSE_K)
    fused = H.fused(oe, cd, cs, cn, qv, smoothing=cfg["smoothing"])
    dts = (torch.int32, torch.float64, torch.float64, torch.int32, torch.int32)
    fused = tuple(x.to(device=eng.device, dtype=dt).contiguous() for x, dt in zip(fused, dts))
    fin = eng.diversify(fused, top_k=int(cfg["top_k"]), diversification=bool(cfg.get("diversification", False)))
    wd, ws, _, _, wn = _cpu(*fin)
    doc, score, _, n = got
    assert n.tolist() == wn.tolist()
    worst = 0.0
    for q in range(QH):
        k = int(n[q])
        assert doc[q, :k].tolist() == wd[q, :k].tolist(), q
        worst = max(worst, float(np.abs(score[q, :k] - ws[q, :k]).max()) if k else 0.0)
    print(f"hybrid step vs CPU chain: largest |score difference| = {worst:.3e} (bar {RERANK_BAR})")
    assert worst <= RERANK_BAR


def test_a_document_without_a_query_term_is_found(hyb):
    ix, terms, qv, planted, r = hyb
    z = _z(ix)
    ids = _np(ix.doc_ids)
    Q = 8
    # plant: for query i a document that shares no term with it and whose first chunk row IS the query vector
    emb, off = _np(ix.emb).copy(), _np(ix.doc_off).astype(np.int64)
    qs, star = [list(t) for t in terms[:Q]], []
    for i in range(Q):
        _, touched = H.point_scores(z, qs[i], np.arange(ix.n_docs))
        free = [d for d in np.nonzero(~touched)[0] if ix.urls[d] is not None and d not in planted and d not in star]
        assert free or i == 3
        d = free[i] if free else None
        star.append(d)
    qs[3] = [-1, -2]
    _, touched3 = H.point_scores(z, qs[3], np.arange(ix.n_docs))
    assert not touched3.any()
    star[3] = next(d for d in range(200, ix.n_docs) if ix.urls[d] is not None and d not in planted and d not in star)
    for i in range(Q):
        emb[off[star[i]]] = qv[i]
    ix2 = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                      "total_docs", "doc_off", "chunk_ids")}, emb=torch.as_tensor(emb))
    ix2.urls, ix2.titles, ix2.texts = ix.urls, ix.titles, ix.texts
    r2 = Retriever(indexer=DeviceEngine(ix2, max_queries=64, max_k=1000, rerank_max_docs=1000))
    try:
        kw = dict(query_embeddings=qv[:Q], term_lists=[[str(t) for t in q] for q in qs])
        ix2.vocab = {str(t): int(t) for q in qs for t in q if t >= 0}
        lexical = r2.search_batch(["q"] * Q, **kw)
        hybrid = r2.search_batch(["q"] * Q, mode="hybrid", dense_k=DENSE_K, **kw)
        saw_both = False
        for i in range(Q):
            want = str(int(ids[star[i]]))
            assert all(d["doc_id"] != want for d in lexical[i]), i          # the lexical stage is blind to it
            assert all("matched_by" not in d for d in lexical[i])
            hit = [d for d in hybrid[i] if d["doc_id"] == want]
            assert len(hit) == 1 and hit[0]["matched_by"] == "dense" and hit[0]["rank"] <= 3, (i, hit)
            assert all(d["matched_by"] in ("lexical", "dense", "both") for d in hybrid[i])
            saw_both |= any(d["matched_by"] == "both" for d in hybrid[i])
        assert lexical[3] == [] and 0 < len(hybrid[3]) <= DENSE_K
        assert all(d["matched_by"] == "dense" for d in hybrid[3])
        # a document of both lists says "both": make the dense top hit of query 0 one of its BM25 hits
        top_lex = lexical[0][0]["doc_id"]
        d_lex = int(np.searchsorted(ids, int(top_lex)))
        emb[off[d_lex]] = qv[0]
        ix3 = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                          "total_docs", "doc_off", "chunk_ids")}, emb=torch.as_tensor(emb))
        ix3.urls, ix3.titles, ix3.texts, ix3.vocab = ix.urls, ix.titles, ix.texts, ix2.vocab
        r2.update_index(ix3)
        rows = r2.search("q", query_embedding=qv[0], terms=[str(t) for t in qs[0]], mode="hybrid", dense_k=DENSE_K)
        assert [d["matched_by"] for d in rows if d["doc_id"] == top_lex] == ["both"]
    finally:
        r2.engine.close()


def test_default_mode_did_not_move_and_bad_modes_are_refused(hyb):
    ix, _, _, _, r = hyb
    terms, qv = synthetic_queries(ix, 64, seed=41, lo_rank=5, hi_rank=3000)
    qv = qv.numpy()
    a = r.final_lists(terms, qv, 1000)
    b = r.final_lists(terms, qv, 1000, mode="lexical")
    assert len(a) == len(b) == 4 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    ix.vocab = {str(t): int(t) for q in terms for t in q}
    kw = dict(query_embeddings=qv[:8], term_lists=[[str(t) for t in q] for q in terms[:8]])
    assert r.search_batch(["q"] * 8, **kw) == r.search_batch(["q"] * 8, mode="lexical", **kw)
    assert list(r.batch_search([(str(i), "q") for i in range(8)], **kw)) == \
        list(r.batch_search([(str(i), "q") for i in range(8)], mode="lexical", **kw))
    for call in (lambda: r.final_lists(terms[:2], qv[:2], 1000, mode="dense"),
                 lambda: r.search("q", query_embedding=qv[0], terms=["1"], mode="HYBRID"),
                 lambda: r.search_batch(["q"], mode=None, query_embeddings=qv[:1], term_lists=[["1"]]),
                 lambda: r.batch_search([("1", "q")], mode="rrf", query_embeddings=qv[:1], term_lists=[["1"]]),
                 lambda: r.final_lists(terms[:2], qv[:2], 1000, mode="hybrid", dense_k=0),
                 lambda: r.final_lists(terms[:2], qv[:2], 1000, mode="hybrid", dense_k=1000),
                 lambda: list(r.final_list_chunks(terms[:2], qv[:2], 1000, mode="x"))):
        with pytest.raises(ValueError):
            call()


def test_hybrid_within_a_document_set(hyb):
    ix, terms, qv, planted, r = hyb
    mask = np.zeros(ix.n_docs, bool)
    mask[::2] = True
    mask[planted[0, :5]] = True
    ds = DocSet.from_mask(ix, mask)
    got = r.final_lists(terms, qv, 1000, within=ds, mode="hybrid", dense_k=DENSE_K)
    want, _ = _compose(r, terms, qv, 1000, DENSE_K, within=ds)
    _same_lists(got, want)
    for q in range(QH):
        assert mask[got[0][q, :got[3][q]]].all()
    assert got[3].min() > 0


def test_hybrid_follows_update_index():
    from test_gpu_index_remove import chunks, corpus, meta, removal, subset, token_batch
    from msretr.chunk_index import attach_chunks
    from msretr.index_build import bm25_add_token_ids
    rng, b0, t0, m0, base = corpus(57)
    r = Retriever(indexer=base, max_queries=64, max_k=1000, rerank_max_docs=1000)
    try:
        R = removal(rng, np.asarray(base.doc_ids), "scattered", 0.05)
        new_ids = np.arange(400_000, 400_200, dtype=np.int64)
        nb = token_batch(rng, new_ids, 6500)
        nb = subset(nb, np.diff(nb[1]) > 0)
        t1 = chunks(rng, nb[0], int(t0.chunk_ids.max()) + 1)
        grown = bm25_add_token_ids(remove_documents(base, R), *nb, 6500, docs_meta=meta(nb[0], "new/"))
        r.update_index(attach_chunks(grown, t1))
        ix = r.index
        z = _z(ix)
        ids = _np(ix.doc_ids)
        df = np.diff(z["term_off"])
        pool = np.nonzero((df > 3) & (df < 2000))[0]
        Q = 6
        terms = [[int(t) for t in rng.choice(pool, 4, replace=False)] + [int(pool[0])] for _ in range(Q)]
        # BM25.score_docs on the rebuilt tables: new documents, kept documents; a removed one is unknown
        some = np.concatenate([nb[0][:20], ids[:20], ids[-20:]])
        got = r.bm25.score_terms(terms[0], some)
        ws, wt = H.point_scores(z, terms[0], np.searchsorted(ids, some))
        assert [g[0] for g in got] == some.tolist() and [g[1] for g in got] == ws.tolist() and [g[2] for g in got] == wt.tolist()
        with pytest.raises(KeyError):
            r.bm25.score_terms(terms[0], [int(R[0])])
        # hybrid search on the new index: the new documents' chunk rows as queries
        rows = _np(t1.emb)[:Q]
        qv = rows + 0.05 * rng.standard_normal(rows.shape).astype(np.float32)
        got = r.final_lists(terms, qv, 1000, mode="hybrid", dense_k=20, with_source=True)
        want, _ = _compose(r, terms, qv, 1000, 20)
        _same_lists(got, want)
        gone = set(np.searchsorted(_np(base.doc_ids), R).tolist())
        for q in range(Q):
            top = int(ids[got[0][q, 0]])
            assert top == int(t1.doc_ids[q]) and got[4][q, 0] in (2, 3)      # found by its new text
        assert not set(ids.tolist()) & set(R.tolist())
    finally:
        r.engine.close()


def test_http_search_hybrid_mode(hyb):
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, terms, qv, planted, r = hyb
    vocab_terms = [str(t) for t in terms[0]]
    ix.vocab = {s: int(s) for s in vocab_terms}
    client = TestClient(create_app(r))
    body = {"query": "tuebingen", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist(), "terms": vocab_terms}
    plain = client.post("/api/search", json=body)
    assert plain.status_code == 200
    assert plain.json()["documents"] == r.search("tuebingen", top_k=1000, query_embedding=qv[0], terms=vocab_terms, query_id="q1")
    assert client.post("/api/search", json=dict(body, mode="lexical")).json() == plain.json()
    hy = client.post("/api/search", json=dict(body, mode="hybrid", dense_k=DENSE_K))
    assert hy.status_code == 200
    docs = hy.json()["documents"]
    assert docs == r.search("tuebingen", top_k=1000, query_embedding=qv[0], terms=vocab_terms, query_id="q1", mode="hybrid",
                            dense_k=DENSE_K)
    assert docs and all(d["matched_by"] in ("lexical", "dense", "both") for d in docs)
    assert any(d["matched_by"] == "dense" for d in docs)
    for bad in ({"mode": "dense"}, {"mode": ""}, {"mode": "hybrid", "dense_k": 0}, {"mode": "hybrid", "dense_k": 5000}):
        assert client.post("/api/search", json=dict(body, **bad)).status_code in (400, 422), bad
    assert client.post("/api/search", json=dict(body, mode=7)).status_code in (400, 422)

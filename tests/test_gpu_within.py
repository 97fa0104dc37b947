"""Document sets on the GPU (msr_bm25_topk_within / msr_dense_topk_within, DocSet, within= of the facades, /api/search sites):
the restricted BM25 lists against the oracle's full lists filtered and cut (bit for bit), the restricted dense lists against
the unrestricted call on the index without the documents outside the set (bit for bit, same sweep kernel) and against the
oracle, the hybrid chain, the HTTP route, the ABI refusals and the index binding of a DocSet."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr.docset import DocSet
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import remove_documents
from msretr.retriever import Retriever
from msretr.synthetic import synthetic_corpus, synthetic_queries
from oracle import dense_ref, rerank_ref
from oracle_engine import OracleEngine
from within_ref import bm25_full, restrict_list

pytestmark = pytest.mark.gpu
N = 20_013                                                   # 20 BM25 tiles of 1024 documents, a last partial bitset word


def _z(ix):
    z = {k: _np(getattr(ix, k)) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")}
    z["avgdl"] = ix.avgdl
    return z


def _chunkless(ix):
    """The same corpus with chunk-less documents at the front, the back and inside (their rows go to a neighbour)."""
    cnt = np.diff(_np(ix.doc_off).astype(np.int64))
    for d in (0, 1, 2, 777, 778, 5000, 12345):
        cnt[d + 1] += cnt[d]; cnt[d] = 0
    for d in (N - 1, N - 2):
        cnt[d - 1] += cnt[d]; cnt[d] = 0
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    out = CorpusIndex(doc_ids=ix.doc_ids, doc_len=ix.doc_len, term_off=ix.term_off, post_doc=ix.post_doc, post_tf=ix.post_tf,
                      idf=ix.idf, avgdl=ix.avgdl, total_docs=ix.total_docs, doc_off=off, chunk_ids=ix.chunk_ids, emb=ix.emb)
    out.n_docs_global = out.n_docs
    return out


@pytest.fixture(scope="module")
def corp():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = _chunkless(synthetic_corpus(N, n_chunks=60_000, n_terms=6000, seed=11))
    terms, qv = synthetic_queries(ix, 120, seed=12, lo_rank=5, hi_rank=3000)
    return ix, terms, qv.numpy()


def _sets(N, seed=0):
    rng = np.random.default_rng(seed)
    m = lambda: np.zeros(N, bool)
    one, other, rnd, block, tail = m(), m(), rng.random(N) < 0.01, m(), m()
    one[4242] = True
    other[::2] = True
    block[1000:3100] = True                                  # crosses the 1024-document tiles at 1024, 2048 and 3072
    tail[N - 5:] = True; tail[(N // 32) * 32 - 3:(N // 32) * 32 + 2] = True; tail[-1] = True   # the last, partial word
    return {"all": np.ones(N, bool), "empty": m(), "one": one, "every_other": other, "random_1pct": rnd, "block": block,
            "tail_word": tail}


SETS = list(_sets(N).keys())


@pytest.fixture(scope="module")
def eng(corp):
    e = DeviceEngine(corp[0], max_queries=16, max_k=1000, rerank_max_docs=1000)
    yield e
    e.close()


def _bm25_check(eng, ix, terms, within_masks, k, min_score, got):
    doc, score, n = [x.cpu().numpy() for x in got]
    z = _z(ix)
    for q, t in enumerate(terms):
        fd, fs = bm25_full(z, t, min_score)
        if within_masks[q] is None:
            wd, ws = fd[:k], fs[:k]
        else:
            wd, ws = restrict_list(fd, fs, len(fd), within_masks[q], k)
        assert n[q] == len(wd), (q, n[q], len(wd))
        assert doc[q, :n[q]].tolist() == wd.tolist()
        assert score[q, :n[q]].tobytes() == ws.tobytes()     # the unrestricted scores, bit for bit
        assert (doc[q, n[q]:] == -1).all() and np.isneginf(score[q, n[q]:]).all()


@pytest.mark.parametrize("name", SETS)
def test_bm25_within_vs_oracle_full_list(corp, eng, name):
    ix, terms, _ = corp
    mask = _sets(N, 8)[name]
    ds = DocSet.from_mask(ix, mask)
    t = terms[:12]
    for k, min_score in ((100, 0.0), (1000, 0.0), (50, -1e9)):
        got = eng.bm25_topk(t, k=k, min_score=min_score, within=ds)
        _bm25_check(eng, ix, t, [mask] * len(t), k, min_score, got)
        if name == "all":                                      # the whole corpus: the unrestricted call, bit for bit
            ref = eng.bm25_topk(t, k=k, min_score=min_score)
            assert all(torch.equal(a, b) for a, b in zip(got, ref))
        if name == "empty":
            assert int(got[2].max()) == 0


def test_bm25_mixed_sets_more_queries_than_max_queries(corp, eng):
    ix, terms, _ = corp
    sets = _sets(N, 9)
    pool = [None, sets["random_1pct"], sets["block"], None, sets["empty"], sets["every_other"]]
    t = terms[:40]                                               # 40 > max_queries = 16: three slices
    masks = [pool[i % len(pool)] for i in range(len(t))]
    within = [None if m is None else DocSet.from_mask(ix, m) for m in masks]
    for min_score in (0.0, -1e9):
        got = eng.bm25_topk(t, k=300, min_score=min_score, within=within)
        _bm25_check(eng, ix, t, masks, 300, min_score, got)
    # k above the number of allowed matches: every match, out_n < k
    small = DocSet.from_mask(ix, sets["random_1pct"])
    got = eng.bm25_topk(t[:4], k=1000, within=small)
    _bm25_check(eng, ix, t[:4], [sets["random_1pct"]] * 4, 1000, 0.0, got)
    assert int(got[2].max()) < 1000


# ------------------------------------------------------------------------------------------------ dense
def _sub(ix, mask):
    """The index without the documents outside `mask`, and the maps of its document / row numbers back to ix's."""
    ids = _np(ix.doc_ids)
    sub = remove_documents(ix, ids[~mask])
    cnt = np.diff(_np(ix.doc_off).astype(np.int64))
    return sub, np.nonzero(mask)[0], np.nonzero(np.repeat(mask, cnt))[0]


def _dense_oracle(ix, mask, q, k, mc, got):
    """Against dense_ref.quick_search on the sub-index (mapped back): same documents up to swaps inside the tolerance, scores
    within 1e-5, chunk rows of the document whose cosine is the document's score."""
    sub, dmap, rmap = _sub(ix, mask)
    emb, off = _np(sub.emb), _np(sub.doc_off).astype(np.int64)
    doc, score, chunk, n = [x.cpu().numpy() for x in got]
    for i in range(len(q)):
        best, _ = dense_ref.doc_scores(emb, off, q[i], mc)
        oi, os_, _ = dense_ref.quick_search(emb, off, q[i], k, mc)
        assert n[i] == len(oi)
        assert np.isin(doc[i, :n[i]], dmap).all()
        sd = np.searchsorted(dmap, doc[i, :n[i]])
        np.testing.assert_allclose(score[i, :n[i]], os_, rtol=0, atol=1e-5)
        np.testing.assert_allclose(score[i, :n[i]], best[sd], rtol=0, atol=1e-5)
        for d in set(sd.tolist()) ^ set(oi.tolist()):
            assert abs(best[d] - os_[-1]) <= 2e-5
        for j in range(n[i]):
            r = np.searchsorted(rmap, chunk[i, j])
            assert rmap[r] == chunk[i, j] and off[sd[j]] <= r < off[sd[j] + 1]
            if mc:
                assert r < off[sd[j]] + mc
            assert abs(float(rerank_ref.cosine_f32(q[i], emb[r:r + 1])[0]) - best[sd[j]]) <= 2e-5
        assert (doc[i, n[i]:] == -1).all()


@pytest.mark.parametrize("layout,mc", [(0, 0), (0, 3), (1, 0)])
def test_dense_within_vs_sub_index_and_oracle(corp, layout, mc):
    ix, _, qv = corp
    sets = _sets(N, 10)
    e = DeviceEngine(ix, max_queries=256, max_k=1000, scan_layout=layout)
    same_kernel = 0
    try:
        for name in ("all", "one", "every_other", "random_1pct", "block", "tail_word"):
            mask = sets[name]
            ds = DocSet.from_mask(ix, mask)
            sub, dmap, rmap = _sub(ix, mask)
            es = DeviceEngine(sub, max_queries=256, max_k=1000, scan_layout=layout)
            try:
                for Q in (1, 33, 64):
                    q = qv[:Q]
                    got = e.dense_topk(q, k=100, max_chunks_per_doc=mc, within=ds)
                    path = e.dense_path()
                    assert path in (32, 64)
                    _dense_oracle(ix, mask, q, 100, mc, got)
                    ref = es.dense_topk(q, k=100, max_chunks_per_doc=mc)
                    if es.dense_path() != path:
                        continue
                    same_kernel += 1
                    doc, score, chunk, n = [x.cpu().numpy() for x in got]
                    rd, rs, rc, rn = [x.cpu().numpy() for x in ref]
                    assert n.tolist() == rn.tolist()
                    for i in range(Q):
                        assert doc[i, :n[i]].tolist() == dmap[rd[i, :n[i]]].tolist()
                        assert score[i].tobytes() == rs[i].tobytes()
                        assert chunk[i, :n[i]].tolist() == rmap[rc[i, :n[i]]].tolist()
            finally:
                es.close()
        assert same_kernel > 0, "no case ran the same sweep kernel restricted and on the sub-index"
        # more than 64 queries: an unrestricted call would take the streaming pass; restricted it is split into sweeps
        mask = sets["random_1pct"]
        got = e.dense_topk(qv[:100], k=100, max_chunks_per_doc=mc, within=DocSet.from_mask(ix, mask))
        assert e.dense_path() in (32, 64)
        _dense_oracle(ix, mask, qv[:100], 100, mc, got)
        # empty set
        d, s, c, n = e.dense_topk(qv[:3], k=10, within=DocSet.from_mask(ix, sets["empty"]))
        assert n.tolist() == [0, 0, 0] and (d == -1).all().item()
    finally:
        e.close()


def test_quick_search_within_unique_and_chunks(corp):
    ix, _, qv = corp
    mask = _sets(N, 11)["block"]
    r = Retriever(indexer=DeviceEngine(ix, max_queries=64, max_k=1000))
    sub = _sub(ix, mask)[0]
    rs = Retriever(indexer=DeviceEngine(sub, max_queries=64, max_k=1000))
    ds = DocSet.from_mask(ix, mask)
    for unique in (True, False):
        got = r.quick_search_batch(query_embeddings=qv[:6], top_k=20, return_unique_docs=unique, within=ds)
        want = rs.quick_search_batch(query_embeddings=qv[:6], top_k=20, return_unique_docs=unique)
        assert got == want
    one = r.quick_search(query_embedding=qv[0], top_k=5, within=ds)
    assert one == rs.quick_search(query_embedding=qv[0], top_k=5)


# ------------------------------------------------------------------------------------------------ hybrid, HTTP
def test_hybrid_search_batch_within_vs_oracle_chain(corp):
    ix, terms, qv = corp
    sets = _sets(N, 12)
    eng = DeviceEngine(ix, max_queries=64, max_k=1000, rerank_max_docs=1000)
    r = Retriever(indexer=eng)
    oe = OracleEngine(ix)
    z = _z(ix)
    masks = [sets["every_other"], None, sets["random_1pct"], sets["block"], sets["empty"], sets["every_other"]]
    within = [None if m is None else DocSet.from_mask(ix, m) for m in masks]
    Q, K = len(masks), 1000
    doc, score, _, n = r.final_lists(terms[:Q], qv[:Q], K, within=within)
    cd = np.full((Q, K), -1, np.int32); cs = np.full((Q, K), -np.inf); cn = np.zeros(Q, np.int32)
    for q in range(Q):
        fd, fs = bm25_full(z, terms[q])
        wd, ws = (fd[:K], fs[:K]) if masks[q] is None else restrict_list(fd, fs, len(fd), masks[q], K)
        cd[q, :len(wd)], cs[q, :len(wd)], cn[q] = wd, ws, len(wd)
    cos, meta = oe.rerank_gather(torch.as_tensor(qv[:Q]), cd, cn)
    fused = oe.rerank_fuse(cd, cs, cn, cos, meta, smoothing=r.reranker.cfg["smoothing"])
    dts = (torch.int32, torch.float64, torch.float64, torch.int32, torch.int32)
    fused = tuple(x.to(device=eng.device, dtype=dt).contiguous() for x, dt in zip(fused, dts))
    fin = eng.diversify(fused, top_k=int(r.reranker.cfg["top_k"]),
                        diversification=bool(r.reranker.cfg.get("diversification", False)))
    fd_, fs_, _, _, fn_ = [x.cpu().numpy() for x in fin]
    assert n.tolist() == fn_.tolist()
    assert n[4] == 0
    for q in range(Q):
        assert doc[q, :n[q]].tolist() == fd_[q, :n[q]].tolist()
        np.testing.assert_allclose(score[q, :n[q]], fs_[q, :n[q]], rtol=0, atol=5e-6)     # bench.py's rerank parity bar
        if masks[q] is not None:
            assert masks[q][doc[q, :n[q]]].all()
    assert r.search("q", terms=terms[4], query_embedding=qv[4], within=within[4]) == []


def _with_urls(ix):
    N_ = ix.n_docs
    ids = _np(ix.doc_ids)
    hosts = ["uni-tuebingen.de", "www.uni-tuebingen.de", "CS.Uni-Tuebingen.DE", "tuebingen.de", "notuni-tuebingen.de",
             "example.org"]
    ix.urls = [None if d % 97 == 0 else f"https://{hosts[d % len(hosts)]}/doc{int(ids[d])}" for d in range(N_)]
    ix.titles = [f"title {d}" for d in range(N_)]
    ix.texts = [f"text of document {d} " * 3 for d in range(N_)]
    ix._url_group = None
    return ix


def test_http_search_with_sites(corp):
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix0, terms, qv = corp
    ix = _with_urls(CorpusIndex(**{k: getattr(ix0, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf",
                                                                  "idf", "avgdl", "total_docs", "doc_off", "chunk_ids", "emb")}))
    vocab_terms = [str(t) for t in terms[0]]
    ix.vocab = {s: int(s) for s in vocab_terms}
    r = Retriever(indexer=DeviceEngine(ix, max_queries=64, max_k=1000, rerank_max_docs=1000))
    client = TestClient(create_app(r))
    body = {"query": "tuebingen", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist(), "terms": vocab_terms}
    plain = client.post("/api/search", json=body)
    assert plain.status_code == 200
    assert plain.json()["documents"] == r.search("tuebingen", top_k=1000, query_embedding=qv[0], terms=vocab_terms, query_id="q1")
    site = client.post("/api/search", json=dict(body, sites=["uni-tuebingen.de"]))
    assert site.status_code == 200
    docs = site.json()["documents"]
    ds = DocSet.from_sites(ix, ["uni-tuebingen.de"])
    assert docs == r.search("tuebingen", top_k=1000, query_embedding=qv[0], terms=vocab_terms, query_id="q1", within=ds)
    assert docs and set(site.json()) == set(plain.json())
    for d in docs:
        host = d["url"].split("/")[2].lower()
        assert host == "uni-tuebingen.de" or host.endswith(".uni-tuebingen.de")


# ------------------------------------------------------------------------------------------------ guards
def test_abi_refusals_out_of_range_sets_and_no_leaks(corp, eng):
    ix, terms, qv = corp
    lib, h, st = eng.lib, eng.handle, eng._stream()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    q_off, q_terms, q_qtf, Q = eng.pack_queries(terms[:3])
    dev = eng.device
    W = (N + 31) // 32
    bits = torch.full((2, W), -1, dtype=torch.int32, device=dev)
    q_set = torch.tensor([0, 1, -1], dtype=torch.int32, device=dev)
    before = eng.bm25_topk(terms[:3], k=50), eng.dense_topk(qv[:3], k=50)

    def outs(fill_score):
        return (torch.full((Q, 50), 7, dtype=torch.int32, device=dev), torch.full((Q, 50), fill_score, device=dev),
                torch.full((Q,), 9, dtype=torch.int32, device=dev))
    for n_sets, b, stride, qs in ((-1, bits, W, q_set), (2, None, W, q_set), (2, bits, W - 1, q_set), (2, bits, W, None)):
        od, osc, on = outs(3.0)
        osc = osc.double()
        rc = lib.msr_bm25_topk_within(h, P(q_off), P(q_terms), P(q_qtf), Q, 50, C.c_double(0.0), P(b), n_sets, stride, P(qs),
                                      P(od), P(osc), P(on), st)
        assert rc == -1
        assert b"msr_bm25_topk_within" in lib.msr_last_error(h)
        od2, osc2, on2 = outs(3.0)
        ch = torch.full((Q, 50), 5, dtype=torch.int32, device=dev)
        qd = torch.as_tensor(qv[:3]).to(dev)
        rc = lib.msr_dense_topk_within(h, P(qd), Q, 50, 0, P(b), n_sets, stride, P(qs), P(od2), P(osc2), P(ch), P(on2), st)
        assert rc == -1 and b"msr_dense_topk_within" in lib.msr_last_error(h)
        torch.cuda.synchronize(dev)
        assert (od == 7).all() and (osc == 3.0).all() and (on == 9).all()
        assert (od2 == 7).all() and (osc2 == 3.0).all() and (on2 == 9).all() and (ch == 5).all()
    # q_set outside [-1, n_sets): the empty set; n_sets = 0: unrestricted
    bad = torch.tensor([2, -2, 1000], dtype=torch.int32, device=dev)
    od, osc, on = outs(3.0)
    osc = osc.double()
    assert lib.msr_bm25_topk_within(h, P(q_off), P(q_terms), P(q_qtf), Q, 50, C.c_double(0.0), P(bits), 2, W, P(bad),
                                    P(od), P(osc), P(on), st) == 0
    qd = torch.as_tensor(qv[:3]).to(dev)
    od2, osc2, on2 = outs(3.0)
    assert lib.msr_dense_topk_within(h, P(qd), Q, 50, 0, P(bits), 2, W, P(bad), P(od2), P(osc2), P(None), P(on2), st) == 0
    torch.cuda.synchronize(dev)
    assert on.tolist() == [0, 0, 0] and (od == -1).all() and on2.tolist() == [0, 0, 0] and (od2 == -1).all()
    od, osc, on = outs(3.0)
    osc = osc.double()
    assert lib.msr_bm25_topk_within(h, P(q_off), P(q_terms), P(q_qtf), Q, 50, C.c_double(0.0), P(None), 0, 0, P(None),
                                    P(od), P(osc), P(on), st) == 0
    assert torch.equal(od, before[0][0]) and torch.equal(osc, before[0][1]) and torch.equal(on, before[0][2])
    # a set with every bit up (bits past n_docs included) is the unrestricted call; nothing leaks into later calls
    d2 = eng.dense_topk(qv[:3], k=50, within=DocSet.from_mask(ix, np.ones(N, bool)))
    assert all(torch.equal(a, b) for a, b in zip(d2, before[1]))
    full = torch.full((1, W), -1, dtype=torch.int32, device=dev)
    od, osc, on = outs(3.0)
    osc = osc.double()
    assert lib.msr_bm25_topk_within(h, P(q_off), P(q_terms), P(q_qtf), Q, 50, C.c_double(0.0), P(full), 1, W,
                                    P(torch.zeros(3, dtype=torch.int32, device=dev)), P(od), P(osc), P(on), st) == 0
    assert torch.equal(od, before[0][0]) and torch.equal(osc, before[0][1]) and torch.equal(on, before[0][2])
    after = eng.bm25_topk(terms[:3], k=50), eng.dense_topk(qv[:3], k=50)
    for a, b in zip(before, after):
        assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)


def test_docset_does_not_survive_update_index(corp):
    ix, terms, qv = corp
    r = Retriever(indexer=DeviceEngine(ix, max_queries=64, max_k=1000, rerank_max_docs=1000))
    mask = _sets(N, 13)["block"]
    ds = DocSet.from_mask(ix, mask)
    a = r.search("q", terms=terms[0], query_embedding=qv[0], within=ds)
    ids = _np(ix.doc_ids)
    r.update_index(remove_documents(ix, ids[[1500, 1501]]))
    with pytest.raises(ValueError):
        r.search("q", terms=terms[0], query_embedding=qv[0], within=ds)
    with pytest.raises(ValueError):
        r.bm25.search_terms(terms[0], within=ds)
    keep = np.delete(mask, [1500, 1501])
    ds2 = DocSet.from_mask(r.index, keep)
    b = r.search("q", terms=terms[0], query_embedding=qv[0], within=ds2)
    assert b and all(d["doc_id"] not in (str(ids[1500]), str(ids[1501])) for d in b)
    assert {d["doc_id"] for d in b} <= {str(i) for i in ids[mask]}
    assert len(a) > 0


def test_tuples_of_sets_and_chunk_sets_live_with_their_docset(corp, eng):
    import gc
    import weakref
    ix, terms, qv = corp
    mask = _sets(N, 14)["block"]
    ds = DocSet.from_mask(ix, mask)
    t = terms[:2]
    ref = eng.bm25_topk(t, k=200, within=[ds, ds])
    for w in ((ds, ds), (ds, None)):                           # tuples as lists
        got = eng.bm25_topk(t, k=200, within=w)
        assert torch.equal(got[0][0], ref[0][0]) and torch.equal(got[2][0], ref[2][0])
    assert all(torch.equal(a, b) for a, b in zip(eng.bm25_topk(t, k=200, within=ds), ref))
    d1 = eng.dense_topk(qv[:2], k=20, within=(ds, ds))
    d2 = eng.dense_topk(qv[:2], k=20, within=ds)
    assert all(torch.equal(a, b) for a, b in zip(d1, d2))
    # return_unique_docs=False: the chunk view's set is cached on the DocSet and goes with it
    r = Retriever(indexer=DeviceEngine(ix, max_queries=64, max_k=1000))
    first = r.quick_search(query_embedding=qv[0], top_k=10, return_unique_docs=False, within=ds)
    tmp = DocSet.from_mask(ix, mask)
    assert r.quick_search(query_embedding=qv[0], top_k=10, return_unique_docs=False, within=tmp) == first
    chunk_set = weakref.ref(tmp._chunk_view[1])
    del tmp
    gc.collect()
    assert chunk_set() is None
    assert r.quick_search(query_embedding=qv[0], top_k=10, return_unique_docs=False, within=ds) == first

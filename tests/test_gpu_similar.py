"""Similar documents on the GPU (msr_gather_rows / msr_dense_topk_grouped, DeviceEngine.gather_rows / dense_topk_grouped,
Retriever.similar, POST /api/similar): the gathered rows against the index bit for bit in both layouts, the grouped lists
against one msr_dense_topk call followed by the numpy merge (bit for bit) and against float64 cosines, planted
near-duplicates, the merge's global-memory path, document sets, the refusals, index updates and the HTTP route."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr.docset import DocSet
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from msretr.index_build import remove_documents
from msretr.retriever import Retriever
from similar_ref import brute_force, dense_scores, merge_lists

pytestmark = pytest.mark.gpu
N = 7001
PLANT = {11: [4321], 2500: [17, 6999], 300: [301]}        # source document -> its planted copies (same rows, other ids)


def _corpus(seed=5):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 9, size=N)
    cnt[rng.random(N) < 0.05] = 0                            # chunk-less documents, including at both ends
    cnt[[0, 1, 5000, N - 1]] = 0
    for a, bs in PLANT.items():
        cnt[a] = max(cnt[a], 2)
        for b in bs:
            cnt[b] = cnt[a]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    emb = rng.standard_normal((int(off[-1]), 768)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    for a, bs in PLANT.items():
        for b in bs:
            emb[off[b]:off[b + 1]] = emb[off[a]:off[a + 1]]
    ids = (np.arange(N, dtype=np.int64) * 3 + 100)
    ix = CorpusIndex(doc_ids=ids, doc_off=off, chunk_ids=np.arange(int(off[-1]), dtype=np.int64) + 50_000, emb=emb,
                     total_docs=N)
    hosts = ["uni-tuebingen.de", "www.uni-tuebingen.de", "example.org", "tuebingen.de"]
    ix.urls = [f"https://{hosts[d % len(hosts)]}/doc{int(ids[d])}" for d in range(N)]
    ix.titles = [f"title {d}" for d in range(N)]
    ix.texts = [f"text of document {d} " * 20 for d in range(N)]
    return ix


@pytest.fixture(scope="module")
def corp():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _corpus()


@pytest.fixture(scope="module")
def eng(corp):
    e = DeviceEngine(corp, max_queries=256, max_k=1024, rerank_max_docs=0)
    yield e
    e.close()


def _np(t):
    return [x.cpu().numpy() for x in t]


def _as_tuples(doc, score, chunk, src, n):
    return [[(int(doc[g, j]), score[g, j], int(chunk[g, j]), int(src[g, j])) for j in range(int(n[g]))] for g in range(len(n))]


def _composed(eng, q, goff, excl, k, min_score=-np.inf, within_rows=None):
    """What the contract says: ONE dense_topk call of depth k + max |excl_g| over all rows, then the host merge."""
    kk = k + max(len(e) for e in excl)
    d, s, c, n = _np(eng.dense_topk(q, k=kk, within=within_rows))
    return merge_lists(d, s, c, n, goff, excl, k, min_score)


def _random_groups(rng, n_rows, n_groups):
    cut = np.sort(rng.integers(0, n_rows + 1, size=n_groups - 1))
    return np.concatenate([[0], cut, [n_rows]]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("layout,row_copy", [(0, True), (1, True), (0, False)])
def test_gather_rows_bit_for_bit(corp, layout, row_copy):
    e = DeviceEngine(corp, max_queries=256, max_k=100, rerank_max_docs=0, scan_layout=layout, row_copy=row_copy)
    try:
        n_chunks = int(corp.doc_off[-1])
        rows = np.concatenate([[0, 1, 15, 16, 17, n_chunks - 1], np.random.default_rng(1).integers(0, n_chunks, 500)])
        got = e.gather_rows(rows).cpu().numpy()
        assert got.tobytes() == np.asarray(corp.emb)[rows].tobytes()
        out = torch.full((2, 768), 7.0, device=e.device)
        for bad in ([0, n_chunks], [-1, 3]):
            r = torch.tensor(bad, dtype=torch.int32, device=e.device)
            rc = e.lib.msr_gather_rows(e.handle, C.c_void_p(r.data_ptr()), 2, C.c_void_p(out.data_ptr()), e._stream())
            assert rc == -1
        torch.cuda.synchronize()
        assert (out == 7.0).all()                            # refused: out untouched
        assert e.gather_rows([]).shape == (0, 768)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. composition, bit for bit
@pytest.mark.parametrize("n_rows", [1, 60, 64, 65, 128, 200, 256])
def test_grouped_equals_one_dense_call_and_host_merge(corp, eng, n_rows):
    rng = np.random.default_rng(n_rows)
    n_chunks = int(corp.doc_off[-1])
    rows = rng.integers(0, n_chunks, size=n_rows)
    if n_rows > 4:
        rows[3] = rows[2]                                    # a duplicate row inside a group
    q = eng.gather_rows(rows)
    G = max(1, min(9, n_rows // 7))
    goff = _random_groups(rng, n_rows, G)
    excl = [rng.choice(N, size=int(rng.integers(0, 5)), replace=False).tolist() for _ in range(G)]
    for k in (10, 100):
        got = _as_tuples(*_np(eng.dense_topk_grouped(q, goff, excl, k=k)))
        assert got == _composed(eng, q, goff, excl, k)
        ms = 0.05
        got = _as_tuples(*_np(eng.dense_topk_grouped(q, goff, excl, k=k, min_score=ms)))
        assert got == _composed(eng, q, goff, excl, k, ms)


# ------------------------------------------------------------------------------------------------ 3. float64
def _check_f64(corp, q_np, goff, excl, k, got, min_score=-np.inf):
    S, A = dense_scores(corp.emb, corp.doc_off, q_np)
    want = brute_force(S, A, goff, excl, k, min_score)
    doc, score, chunk, src, n = got
    for g in range(len(goff) - 1):
        r0, r1 = int(goff[g]), int(goff[g + 1])
        Sg = S[r0:r1].max(axis=0) if r1 > r0 else None
        assert int(n[g]) == len(want[g]), (g, int(n[g]), len(want[g]))
        for j, (wd, ws, _, _) in enumerate(want[g]):
            d = int(doc[g, j])
            assert abs(float(score[g, j]) - Sg[d]) <= 1e-5
            assert d == wd or abs(Sg[d] - ws) <= 2e-5, (g, j, d, wd)
            assert d not in excl[g]
            r = int(src[g, j])
            assert r0 <= r < r1 and abs(S[r, d] - Sg[d]) <= 2e-5          # the source row reaches the maximum
        assert (doc[g, int(n[g]):] == -1).all() and np.isneginf(score[g, int(n[g]):]).all()


@pytest.mark.parametrize("k", [10, 100, "max"])
def test_grouped_against_float64_multi_slice_and_big_groups(corp, k):
    e = DeviceEngine(corp, max_queries=64, max_k=1024, rerank_max_docs=0)     # 300 rows: five dense calls
    try:
        rng = np.random.default_rng(3)
        n_chunks = int(corp.doc_off[-1])
        rows = rng.integers(0, n_chunks, size=300)
        goff = np.array([0, 150, 151, 151, 240, 300])                         # a group of 150 rows > max_queries, an empty one
        excl = [[1, 2, 3], [], [4], [7, 8], [9]]
        kk = 1024 - 3 if k == "max" else k
        q = e.gather_rows(rows)
        got = _np(e.dense_topk_grouped(q, goff, excl, k=kk))
        _check_f64(corp, np.asarray(corp.emb)[rows], goff, excl, kk, got)
        assert int(got[4][2]) == 0
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. near-duplicates
def test_planted_copies_come_first_and_min_score_finds_exactly_them(corp, eng):
    r = Retriever(indexer=eng)
    ids = np.asarray(corp.doc_ids)
    for a, bs in PLANT.items():
        res = r.similar(int(ids[a]), top_k=10)
        assert res[0]["doc_id"] in {int(ids[b]) for b in bs} and res[0]["score"] >= 1 - 1e-5
        assert all(x["doc_id"] != int(ids[a]) for x in res)
        assert res[0]["source_doc_id"] == int(ids[a])
        assert set(res[0]) >= {"rank", "doc_id", "score", "best_chunk_id", "url", "title", "source_doc_id", "source_chunk_id"}
        dup = r.similar(int(ids[a]), top_k=10, min_score=0.95)
        assert sorted(x["doc_id"] for x in dup) == sorted(int(ids[b]) for b in bs)
    batch = r.similar_batch([int(ids[a]) for a in PLANT], top_k=5)
    assert batch == [r.similar(int(ids[a]), top_k=5) for a in PLANT]
    with pytest.raises(LookupError):
        r.similar(int(ids[-1]) + 1)
    assert r.similar(int(ids[0])) == []                      # a chunk-less source: an empty group, no error


# ------------------------------------------------------------------------------------------------ 5. global-memory path
def test_identical_rows_at_max_k_take_the_global_path_exactly(corp, eng):
    one = np.asarray(corp.emb)[np.full(45, 1234)]
    q = torch.from_numpy(one).to(eng.device)
    goff = np.array([0, 40, 45])
    excl = [[], [5]]
    got = _np(eng.dense_topk_grouped(q, goff, excl, k=1023))    # 40 x 1023 and 5 x 1024 entries: past the LDS image
    assert _as_tuples(*got) == _composed(eng, q, goff, excl, 1023)
    assert int(got[4][0]) == 1023 and (got[3][0, :1023] == 0).all()   # equal maxima in every row: row 0 wins
    _check_f64(corp, one, goff, excl, 1023, got)


# ------------------------------------------------------------------------------------------------ 6. sets
def test_within_one_set_and_per_group_sets(corp, eng):
    rng = np.random.default_rng(9)
    n_chunks = int(corp.doc_off[-1])
    rows = rng.integers(0, n_chunks, size=90)
    q = eng.gather_rows(rows)
    goff = np.array([0, 30, 31, 90])
    excl = [[1], [], [2, 3]]
    ds = DocSet.from_mask(corp, rng.random(N) < 0.3)
    other = DocSet.from_sites(corp, ["example.org"])
    for within in (ds, [ds, None, other]):
        got = _np(eng.dense_topk_grouped(q, goff, excl, k=50, within=within))
        per_g = [within] * 3 if isinstance(within, DocSet) else within
        per_row = [per_g[g] for g in range(3) for _ in range(int(goff[g + 1] - goff[g]))]
        assert _as_tuples(*got) == _composed(eng, q, goff, excl, 50, within_rows=per_row)
        for g in range(3):
            if per_g[g] is not None:
                assert all(per_g[g].mask[int(d)] for d in got[0][g, :int(got[4][g])])
    r = Retriever(indexer=eng)
    res = r.similar(int(corp.doc_ids[2500]), within=other, top_k=20)
    assert res and all("example.org" in x["url"] for x in res)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_outputs_untouched_and_pending_begin_refuses(corp, eng):
    dev, lib, h, st = eng.device, eng.lib, eng.handle, eng._stream()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    q = eng.gather_rows(np.arange(10))
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    goff, eoff, edoc = i32([0, 4, 10]), i32([0, 1, 2]), i32([5, 6])
    G, k = 2, 10
    outs = [torch.full((G, k), 77, dtype=torch.int32, device=dev), torch.full((G, k), 7.0, device=dev),
            torch.full((G, k), 77, dtype=torch.int32, device=dev), torch.full((G, k), 77, dtype=torch.int32, device=dev),
            torch.full((G,), 77, dtype=torch.int32, device=dev)]
    bits = torch.full((1, (N + 31) // 32), -1, dtype=torch.int32, device=dev)
    gset = i32([0, 0])

    def call(qq=q, n_rows=10, go=goff, eo=eoff, ed=edoc, kk=k, ms=float("-inf"), b=None, ns=0, stride=0, gs=None):
        return lib.msr_dense_topk_grouped(h, P(qq), n_rows, P(go), G, P(eo), P(ed), kk, C.c_float(ms), P(b), ns, stride, P(gs),
                                          *[P(o) for o in outs], st)

    assert call() == 0
    torch.cuda.synchronize()
    ok = [o.clone() for o in outs]
    for o in outs:
        o.fill_(77)
    bad = [dict(kk=0), dict(kk=1024), dict(go=i32([0, 5, 4])), dict(go=i32([0, 4, 9])), dict(go=i32([1, 4, 10])),
           dict(eo=i32([0, 2, 1])), dict(ed=i32([5, N])), dict(ed=i32([-1, 6])), dict(qq=None), dict(ms=float("nan")),
           dict(ns=-1), dict(b=None, ns=1, stride=(N + 31) // 32, gs=gset), dict(b=bits, ns=1, stride=1, gs=gset),
           dict(b=bits, ns=1, stride=(N + 31) // 32, gs=None), dict(eo=i32([0, 1, 2]), ed=None)]
    for args in bad:
        assert call(**args) == -1, args
    torch.cuda.synchronize()
    assert all((o == 77).all() for o in outs)
    assert eng.dense_split_max(10) > 0
    qv = eng.gather_rows(np.arange(100))
    eng.dense_begin(qv, k=10)
    assert call() == -1 and b"pending" in lib.msr_last_error(h)
    eng.dense_end(100, k=10)
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, ok))


# ------------------------------------------------------------------------------------------------ 8. index updates
def test_similar_after_update_index(corp):
    ids = np.asarray(corp.doc_ids)
    r = Retriever(indexer=DeviceEngine(corp, max_queries=256, max_k=1024, rerank_max_docs=0))
    try:
        src, copy = int(ids[300]), int(ids[301])
        assert r.similar(src, top_k=3)[0]["doc_id"] == copy
        removed = remove_documents(corp, [copy, int(ids[2500])])
        r.update_index(removed)
        fresh = Retriever(indexer=DeviceEngine(removed, max_queries=256, max_k=1024, rerank_max_docs=0))
        got = r.similar(src, top_k=20)
        assert got == fresh.similar(src, top_k=20) and all(x["doc_id"] != copy for x in got)
        assert r.similar(src, top_k=5, min_score=0.95) == []
        with pytest.raises(LookupError):
            r.similar(int(ids[2500]))
        assert [x["doc_id"] for x in r.similar(int(ids[11]), min_score=0.95)] == [int(ids[4321])]
        fresh.engine.close()
    finally:
        r.engine.close()


# ------------------------------------------------------------------------------------------------ 9. HTTP
def test_http_similar(corp, eng):
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    r = Retriever(indexer=eng)
    client = TestClient(create_app(r))
    ids = np.asarray(corp.doc_ids)
    res = client.post("/api/similar", json={"doc_id": int(ids[2500]), "top_k": 5})
    assert res.status_code == 200
    docs = res.json()["documents"]
    want = r.similar(int(ids[2500]), top_k=5)
    assert [d["doc_id"] for d in docs] == [str(x["doc_id"]) for x in want] and len(docs) == 5
    assert set(docs[0]) >= {"query_id", "rank", "url", "score", "title", "snippet", "domain", "doc_id"}
    assert client.post("/api/similar", json={"doc_ids": [str(int(ids[11])), int(ids[300])], "top_k": 3}).status_code == 200
    assert client.post("/api/similar", json={"top_k": 3}).status_code == 400
    assert client.post("/api/similar", json={"doc_ids": [int(ids[-1]) + 7]}).status_code == 404
    site = client.post("/api/similar", json={"doc_id": int(ids[2500]), "top_k": 10, "sites": ["example.org"]})
    assert site.status_code == 200 and site.json()["documents"]
    assert all(d["url"].split("/")[2] == "example.org" for d in site.json()["documents"])
    near = client.post("/api/similar", json={"doc_id": int(ids[2500]), "min_score": 0.95}).json()["documents"]
    assert sorted(d["doc_id"] for d in near) == sorted(str(int(ids[b])) for b in PLANT[2500])

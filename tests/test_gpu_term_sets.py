"""Document sets built on the GPU from posting lists (msr_term_sets, DeviceEngine.term_sets, the operators of the facades):
the kernel against the numpy reference of term_set_ref.py on every hand-made corpus, word for word; rows of mixed operators in
one call; bases; determinism; the ABI refusals; and the consumers -- BM25, dense, the rerank chain in both modes, the
Retriever / BM25 facades and /api/search -- bit for bit against the same call with a host-built DocSet of the reference mask."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr.docset import DeviceSets, DocSet, pack_bits
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import remove_documents
from msretr.retriever import Retriever
from msretr.synthetic import synthetic_corpus, synthetic_queries
from term_set_ref import BIG, S, SIZES, RowCase, base_mask, corpus, random_rows, row_cases, term_set_mask

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
PAD = 3                                                      # words of a row behind ceil(N / 32) that must keep the fill


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a if len(a) else [0], np.int32)).to(dev)


def _pack_rows(rows, dev):
    m_off, m, x_off, x = [0], [], [0], []
    for r in rows:
        m += list(r.must); m_off.append(len(m))
        x += list(r.must_not); x_off.append(len(x))
    return _i32(m_off, dev), _i32(m, dev), _i32(x_off, dev), _i32(x, dev), _i32([r.base for r in rows], dev)


def _base_rows(c, dev, extra=2):
    """The corpus's base rows on the device, `extra` words of all-ones padding per row (base_stride > ceil(N / 32))."""
    W = (c.n_docs + 31) // 32
    b = np.full((len(c.bases), W + extra), 0xFFFFFFFF, np.uint32)
    for i, (_, m) in enumerate(c.bases):
        b[i, :W] = pack_bits(m)
    return torch.from_numpy(b.view(np.int32)).to(dev), W + extra


def _run(eng, c, rows, with_bases=True):
    """One msr_term_sets call into a pre-filled buffer of stride W + PAD -> uint32 [R, W + PAD] (host)."""
    dev = eng.device
    W = (c.n_docs + 31) // 32
    out = torch.from_numpy(np.full((len(rows), W + PAD), FILL, np.uint32).view(np.int32)).to(dev)
    m_off, m, x_off, x, rb = _pack_rows(rows, dev)
    if with_bases:
        bb, bs = _base_rows(c, dev)
        rc = eng.lib.msr_term_sets(eng.handle, len(rows), _P(m_off), _P(m), _P(x_off), _P(x), _P(bb), len(c.bases), bs, _P(rb),
                                   _P(out), W + PAD, eng._stream())
    else:
        rc = eng.lib.msr_term_sets(eng.handle, len(rows), _P(m_off), _P(m), _P(x_off), _P(x), _P(None), 0, 0, _P(None),
                                   _P(out), W + PAD, eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint32)


def _check(c, rows, got, with_bases=True):
    N, W = c.n_docs, (c.n_docs + 31) // 32
    assert got.shape == (len(rows), W + PAD)
    assert (got[:, W:] == FILL).all(), "words behind ceil(N / 32) were touched"
    for i, r in enumerate(rows):
        want = pack_bits(term_set_mask(c.z, r.must, r.must_not, base_mask(c, r.base) if with_bases else None))
        assert (got[i, :W] == want).all(), (N, i, r.claim)
    if N % 32:
        assert (got[:, W - 1] >> np.uint32(N % 32) == 0).all(), "bits at or above N"


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    made = {}

    def get(N):
        if N not in made:
            c = corpus(N)
            made[N] = (c, DeviceEngine(c.ix, max_queries=4, max_k=16, rerank_max_docs=0))
        return made[N]
    yield get
    for _, e in made.values():
        e.close()


@pytest.mark.parametrize("N", SIZES)
def test_kernel_against_reference_every_case_twice(engines, N):
    c, eng = engines(N)
    rows = row_cases(c)
    a = _run(eng, c, rows)
    _check(c, rows, a)
    b = _run(eng, c, rows)                                   # a second buffer: the same bytes
    assert a.tobytes() == b.tobytes()
    # one row per call gives the same words as the row inside the batch
    for i in (1, 5, len(rows) - 4):
        assert (_run(eng, c, rows[i:i + 1])[0] == a[i]).all(), rows[i].claim


@pytest.mark.parametrize("N", [33, 1025, BIG])
@pytest.mark.parametrize("n_rows", [1, 3, 300])
def test_row_mixes_in_one_call(engines, N, n_rows):
    c, eng = engines(N)
    rows = random_rows(c, n_rows, seed=n_rows)
    got = _run(eng, c, rows)
    _check(c, rows, got)
    assert _run(eng, c, rows).tobytes() == got.tobytes()
    if n_rows == 300:
        nz = sum(int(g[:-PAD].any()) for g in got)
        assert 30 <= nz < 300, nz                            # the mix holds empty rows and non-empty ones


@pytest.mark.parametrize("N", [31, BIG])
def test_no_bases_null_pointers(engines, N):
    c, eng = engines(N)
    rows = [RowCase(r.must, r.must_not, b, r.claim) for r in row_cases(c)[:20] for b in (-1, 0, 7)]   # row_base is not read
    got = _run(eng, c, rows, with_bases=False)
    _check(c, rows, got, with_bases=False)


def test_refusals_leave_the_output_untouched(engines):
    c, eng = engines(1025)
    lib, h, st, dev = eng.lib, eng.handle, eng._stream(), eng.device
    W = (c.n_docs + 31) // 32
    rows = row_cases(c)[:4]
    m_off, m, x_off, x, rb = _pack_rows(rows, dev)
    bb, bs = _base_rows(c, dev)
    nb = len(c.bases)
    out = torch.from_numpy(np.full((4, W), FILL, np.uint32).view(np.int32)).to(dev)
    good = dict(n=4, m_off=m_off, x_off=x_off, bb=bb, nb=nb, bs=bs, rb=rb, out=out, os=W)
    bad = [dict(n=-1), dict(out=None), dict(m_off=None), dict(x_off=None), dict(os=W - 1), dict(bs=W - 1), dict(nb=-1),
           dict(bb=None), dict(rb=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.msr_term_sets(h, a["n"], _P(a["m_off"]), _P(m), _P(a["x_off"]), _P(x), _P(a["bb"]), a["nb"], a["bs"], _P(a["rb"]),
                               _P(a["out"]), a["os"], st)
        assert rc == -1, change
        assert b"msr_term_sets" in lib.msr_last_error(h)
        torch.cuda.synchronize(dev)
        assert (out.cpu().numpy().view(np.uint32) == FILL).all(), change
    # n_rows == 0 succeeds (whatever the pointers) and launches nothing; base_stride is not looked at without bases
    assert lib.msr_term_sets(h, 0, _P(None), _P(None), _P(None), _P(None), _P(None), 0, 0, _P(None), _P(None), W, st) == 0
    assert lib.msr_term_sets(h, 0, _P(m_off), _P(m), _P(x_off), _P(x), _P(bb), nb, bs, _P(rb), _P(out), W, st) == 0
    torch.cuda.synchronize(dev)
    assert (out.cpu().numpy().view(np.uint32) == FILL).all()
    assert lib.msr_term_sets(h, 4, _P(m_off), _P(m), _P(x_off), _P(x), _P(None), 0, 0, _P(None), _P(out), W, st) == 0
    torch.cuda.synchronize(dev)
    assert not (out.cpu().numpy().view(np.uint32) == FILL).all()
    # without postings: not bound
    bare = DeviceEngine(CorpusIndex(doc_ids=np.arange(5, dtype=np.int64)), max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        assert bare.lib.msr_term_sets(bare.handle, 4, _P(m_off), _P(m), _P(x_off), _P(x), _P(None), 0, 0, _P(None), _P(out), W,
                                      bare._stream()) == -2
    finally:
        bare.close()


def test_engine_term_sets_dedup_and_docset(engines):
    c, eng = engines(BIG)
    t = c.term
    a, b, V = t["rnd30"], t["even"], len(t)
    odd = DocSet.from_mask(c.ix, c.bases[0][1])
    must = [[a], [a], [a, b], [b, a, a], [], [], [a], [-1], [V + 3], [t["empty"]], [a]]
    not_ = [[], [-1], [], [], [], [-1, t["empty"]], [a], [], [], [], [b]]
    within = [None, None, None, None, None, odd, None, None, odd, None, odd]
    ds = eng.term_sets(must, not_, within=within)
    assert isinstance(ds, DeviceSets) and len(ds) == len(must)
    bits, q_set, n_sets, stride = eng.pack_within(ds, len(must))                  # handed on unchanged
    assert bits is ds.bits and q_set is ds.q_set and (n_sets, stride) == (ds.n_sets, ds.stride)
    q = ds.q_set.cpu().tolist()
    assert q[0] == q[1] and q[2] == q[3] and q[4] == -1                           # same id lists: one row; no operators: -1
    assert q[6] == q[7] == q[8] == q[9]                                           # every empty row is the same row
    assert ds.n_sets == len(set(v for v in q if v >= 0)) and stride == (BIG + 31) // 32
    assert ds.docset(5) == odd                                                    # no operators: its base's row, no kernel row
    for i in range(len(must)):
        bm = None if within[i] is None else within[i].mask
        assert ds.docset(i) == DocSet.from_mask(c.ix, term_set_mask(c.z, must[i], not_[i], bm)), i
    with pytest.raises(ValueError):
        eng.pack_within(ds, len(must) + 1)
    with pytest.raises(ValueError):
        eng.term_sets([[a]], [[], []])
    # must_not only, one DocSet for every query
    ds2 = eng.term_sets(None, [[b], [a, b]], within=odd)
    assert ds2.docset(0) == odd and ds2.docset(1) == DocSet.from_mask(c.ix, term_set_mask(c.z, [], [a, b], odd.mask))


# ------------------------------------------------------------------------------------------------ consumers
N_DOCS = 20_013


def _word(t):
    s = ""
    t = int(t)
    while True:
        s = chr(ord("a") + t % 26) + s
        t //= 26
        if t == 0:
            return "w" + s


@pytest.fixture(scope="module")
def corp():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = synthetic_corpus(N_DOCS, n_chunks=60_000, n_terms=6000, seed=11)
    terms, qv = synthetic_queries(ix, 12, seed=12, lo_rank=5, hi_rank=3000)
    N = ix.n_docs
    ids = _np(ix.doc_ids)
    hosts = ["uni-tuebingen.de", "tuebingen.de", "example.org"]
    ix.urls = [f"https://{hosts[d % 3]}/doc{int(ids[d])}" for d in range(N)]
    ix.titles = [f"title {d}" for d in range(N)]
    ix.texts = [f"text of document {d} " * 3 for d in range(N)]
    ix._url_group = None
    z = {"term_off": _np(ix.term_off).astype(np.int64), "post_doc": _np(ix.post_doc), "n_docs": N}
    df = np.diff(z["term_off"])
    by_df = np.argsort(-df, kind="stable")
    mid = [int(t) for t in by_df[100:140]]                   # mid-frequency terms: in about a quarter of the documents, so
    assert 0 not in mid and df[mid[0]] < N // 2              # their idf is positive (term 0, the city, has a negative one)
    ix.vocab = {_word(t): t for t in range(ix.n_terms)}
    ix.vocab["tübingen"] = 0
    ix.vocab["mensa"] = mid[20]
    return ix, terms, qv.numpy(), z, mid


@pytest.fixture(scope="module")
def eng(corp):
    e = DeviceEngine(corp[0], max_queries=16, max_k=1000, rerank_max_docs=1000)
    yield e
    e.close()


def _ops(corp):
    """12 queries: must only, not only, both, both inside a site set, no operators, no operators inside a site set."""
    ix, _, _, z, mid = corp
    site = DocSet.from_sites(ix, ["uni-tuebingen.de"])
    rnd = DocSet.from_mask(ix, np.random.default_rng(3).random(ix.n_docs) < 0.5)
    must, not_, within = [], [], []
    for q in range(12):
        a, a2, b = mid[q % 3], mid[5 + q % 2], mid[8 + q % 4]
        kind = q % 6
        must.append([a] if kind in (0, 2) else [a, a2] if kind == 3 else [])
        not_.append([b] if kind in (1, 2) else [b, -1, mid[12]] if kind == 3 else [])
        within.append(site if kind in (3, 5) else rnd if q == 8 else None)
    masks = [term_set_mask(z, must[q], not_[q], None if within[q] is None else within[q].mask)
             if must[q] or not_[q] or within[q] is not None else None for q in range(12)]
    ref = [None if m is None else DocSet.from_mask(ix, m) for m in masks]
    return must, not_, within, masks, ref


def _same(got, want):
    for a, b in zip(got, want):
        a, b = (a.cpu().numpy(), b.cpu().numpy()) if torch.is_tensor(a) else (a, b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_bm25_and_dense_topk_equal_the_host_built_sets(corp, eng):
    ix, terms, qv, z, _ = corp
    must, not_, within, masks, ref = _ops(corp)
    ds = eng.term_sets(must, not_, within=within)
    for q in range(12):
        want = DocSet.from_mask(ix, np.ones(ix.n_docs, bool)) if ref[q] is None else ref[q]
        assert ds.docset(q) == want, q
    assert sum(1 for m in masks if m is not None and m.any()) >= 8
    for k in (100, 1000):
        got = eng.bm25_topk(terms, k=k, within=ds)
        _same(got, eng.bm25_topk(terms, k=k, within=ref))
        assert int(got[2].max()) > 0
    got = eng.dense_topk(qv, k=100, within=ds)
    _same(got, eng.dense_topk(qv, k=100, within=ref))
    doc, n = got[0].cpu().numpy(), got[3].cpu().numpy()
    for q in range(12):
        if masks[q] is not None:
            assert masks[q][doc[q, :n[q]]].all()


def test_dense_topk_grouped_equals_the_host_built_sets(corp, eng):
    ix, terms, qv, z, _ = corp
    must, not_, within, masks, ref = _ops(corp)
    goff = [0, 1, 3, 6, 7, 9, 12]                            # 6 groups of 1 .. 3 query rows; group g takes query g's operators
    ds = eng.term_sets(must[:6], not_[:6], within=within[:6])
    excl = [[], [5, 6], [], [], [], [17]]
    got = eng.dense_topk_grouped(qv, goff, exclude=excl, k=50, within=ds)
    _same(got, eng.dense_topk_grouped(qv, goff, exclude=excl, k=50, within=ref[:6]))
    doc, n = got[0].cpu().numpy(), got[4].cpu().numpy()
    assert int(n.min()) > 0
    for g in range(6):
        if masks[g] is not None:
            assert masks[g][doc[g, :n[g]]].all()


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_final_lists_equal_the_host_built_sets(corp, eng, mode):
    ix, terms, qv, z, _ = corp
    must, not_, within, masks, ref = _ops(corp)
    r = Retriever(indexer=eng)
    kw = dict(mode=mode, with_source=True) if mode == "hybrid" else {}
    got = r.final_lists(terms, qv, 1000, within=within, must=must, must_not=not_, **kw)
    want = r.final_lists(terms, qv, 1000, within=ref, **kw)
    _same(got, want)
    assert len(got) == (5 if mode == "hybrid" else 4) and int(got[3].max()) > 0
    for q in range(12):
        if masks[q] is not None:
            assert masks[q][got[0][q, :got[3][q]]].all()
    # term strings instead of ids, and chunks of 5 queries: one term_sets call per chunk
    words = lambda lists: [[_word(t) if t >= 0 else "notaword" for t in tl] for tl in lists]
    _same(r.final_lists(terms, qv, 1000, chunk=5, within=within, must=words(must), must_not=words(not_), **kw), want)
    # sets built beforehand for all 12 queries: every chunk takes its queries' part of q_set
    ds = eng.term_sets(must, not_, within=within)
    _same(r.final_lists(terms, qv, 1000, chunk=5, within=ds, **kw), want)
    _same(r.final_lists(terms, qv, 1000, within=ds, **kw), want)
    with pytest.raises(ValueError):
        r.final_lists(terms[:5], qv[:5], 1000, within=ds)
    with pytest.raises(ValueError):
        r.final_lists(terms, qv, 1000, operators=True)
    with pytest.raises(ValueError):
        r.final_lists(terms, qv, 1000, must=must[:3])


def _holds(z, t, rows, ix):
    """Do any of the result rows' documents hold term t?"""
    pos = {str(int(d)): i for i, d in enumerate(_np(ix.doc_ids))}
    docs = set(z["post_doc"][z["term_off"][t]:z["term_off"][t + 1]].tolist())
    return any(pos[row["doc_id"]] in docs for row in rows)


def test_retriever_and_bm25_facades(corp, eng):
    ix, terms, qv, z, mid = corp
    r = Retriever(indexer=eng)
    A, B = mid[1], mid[9]
    wa, wb = _word(A), _word(B)
    ref = DocSet.from_mask(ix, term_set_mask(z, [A], [B]))
    e0 = qv[0]
    for mode in ("lexical", "hybrid"):
        got = r.search(f"mensa +{wa} -{wb}", operators=True, query_embedding=e0, mode=mode)
        assert got and got == r.search(f"mensa {wa}", within=ref, query_embedding=e0, mode=mode)
        assert got == r.search(f"mensa {wa}", must=[wa], must_not=[wb], query_embedding=e0, mode=mode)   # explicit lists
        neg = r.search(f"mensa -{wb}", operators=True, query_embedding=e0, mode=mode)
        assert neg and not _holds(z, B, neg, ix)
        assert _holds(z, B, r.search(f"mensa {wb}", query_embedding=e0, mode=mode), ix)      # (the plain query does return them)
        assert r.search("mensa +unknownword", operators=True, query_embedding=e0, mode=mode) == []
        assert r.search("mensa", must=["unknownword"], query_embedding=e0, mode=mode) == []
        # operators off: the signs are what they were -- punctuation
        text = f"mensa +{wa} -{wb}"
        assert r.search(text, operators=False, query_embedding=e0, mode=mode) == r.search(text, query_embedding=e0, mode=mode)
        # operators and a site set
        site = DocSet.from_sites(ix, ["uni-tuebingen.de"])
        both = r.search(f"mensa +{wa} -{wb}", operators=True, within=site, query_embedding=e0, mode=mode)
        assert both == r.search(f"mensa {wa}", within=ref & site, query_embedding=e0, mode=mode)
        assert both and all("//uni-tuebingen.de/" in d["url"] for d in both)
    # -tuebingen excludes the city's pages and does not score the city
    no_city = r.search("mensa -tuebingen", operators=True, query_embedding=e0)
    assert no_city and not _holds(z, 0, no_city, ix)
    assert no_city == r.search("x", terms=["mensa"], within=DocSet.from_mask(ix, term_set_mask(z, [], [0])), query_embedding=e0)
    # batch: per-query operators, one of them without
    qs = [f"mensa +{wa}", "mensa", f"mensa -{wb}"]
    got = r.search_batch(qs, query_embeddings=qv[:3], operators=True)
    assert got[0] == r.search(f"mensa {wa}", within=DocSet.from_mask(ix, term_set_mask(z, [A], [])), query_embedding=qv[0])
    assert got[1] == r.search("mensa", query_embedding=qv[1])
    lines = r.batch_search(list(zip("123", qs)), query_embeddings=qv[:3], operators=True)
    assert [e["url"] for e in lines if e["query_num"] == "3"][:100] == [d["url"] for d in got[2]]
    # the BM25 facade (its query is taken as it is: no city)
    bm = r.bm25.search(f"mensa +{wa} -{wb}", top_k=50, operators=True)
    assert bm and bm == r.bm25.search(f"mensa {wa}", top_k=50, within=ref)
    assert bm == r.bm25.search(f"mensa {wa}", top_k=50, must=[wa], must_not=[wb])
    assert r.bm25.search("mensa +unknownword", operators=True) == []


def test_http_search_with_operators(corp, eng):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, terms, qv, z, mid = corp
    r = Retriever(indexer=eng)
    wa, wb = _word(mid[1]), _word(mid[9])
    client = TestClient(create_app(r))
    body = {"query": f"mensa +{wa} -{wb}", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    ops = client.post("/api/search", json=dict(body, operators=True))
    assert plain.status_code == 200 and ops.status_code == 200
    want = r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", operators=True)
    assert ops.json()["documents"] == want and want
    assert plain.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1")
    assert plain.json()["documents"] != want
    lists = client.post("/api/search", json=dict(body, query=f"mensa {wa}", must=[wa], must_not=[wb], mode="hybrid"))
    assert lists.status_code == 200
    assert lists.json()["documents"] == r.search(f"mensa {wa}", top_k=1000, query_embedding=qv[0], query_id="q1", must=[wa],
                                                 must_not=[wb], mode="hybrid")


def test_device_sets_do_not_survive_update_index(corp):
    ix, terms, qv, z, mid = corp
    r = Retriever(indexer=DeviceEngine(ix, max_queries=16, max_k=1000, rerank_max_docs=1000))
    try:
        ds = r.engine.term_sets([[mid[1]]], [[mid[9]]])
        assert int(r.engine.bm25_topk(terms[:1], k=10, within=ds)[2][0]) > 0
        ids = _np(ix.doc_ids)
        r.update_index(remove_documents(ix, ids[[1500, 1501]]))
        with pytest.raises(ValueError, match="built for another index"):
            r.engine.bm25_topk(terms[:1], k=10, within=ds)
        with pytest.raises(ValueError, match="built for another index"):
            r.engine.dense_topk(qv[:1], k=10, within=ds)
        with pytest.raises(ValueError, match="built for another index"):
            r.final_lists(terms[:1], qv[:1], 1000, within=ds)
        again = r.engine.term_sets([[mid[1]]], [[mid[9]]])
        assert int(r.engine.bm25_topk(terms[:1], k=10, within=again)[2][0]) > 0
        assert again.n_docs == ix.n_docs - 2
    finally:
        r.engine.close()

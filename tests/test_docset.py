"""Document sets on the host (msretr.docset, no GPU): the bit layout, the constructors, the set algebra, the binding to one
index, the packing of per-query sets for msr_*_topk_within, and the restricted-BM25 contract stated on the oracle's lists."""
import numpy as np
import pytest

from msretr.docset import DocSet, pack_bits, pack_within
from msretr.index import CorpusIndex
from msretr.index_build import bm25_add_token_ids, bm25_index_from_token_ids, remove_documents
from within_ref import bm25_full, restrict_list


def _ix(n, urls=None):
    ix = CorpusIndex(doc_ids=np.arange(10, 10 + 3 * n, 3, dtype=np.int64)[:n])
    ix.urls = urls
    return ix


def _unpack(words, n):
    w = np.asarray(words, np.uint32)
    return np.array([(int(w[d >> 5]) >> (d & 31)) & 1 for d in range(n)], bool)


@pytest.mark.parametrize("n", [0, 1, 5, 31, 32, 33, 64, 100, 1000, 1027])
def test_bit_layout(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.4
    if n:
        mask[-1] = True
    w = pack_bits(mask)
    assert w.dtype == np.uint32 and len(w) == (n + 31) // 32
    assert np.array_equal(_unpack(w, n), mask)
    if n % 32:                                               # bits at or above n are 0
        assert int(w[-1]) >> (n % 32) == 0
    ds = DocSet.from_mask(_ix(n), mask)
    assert np.array_equal(ds.words(), w) and len(ds) == int(mask.sum())
    for d in np.nonzero(mask)[0]:
        assert (int(w[d >> 5]) >> (d & 31)) & 1 == 1


def test_from_sites_subdomains_case_and_missing_urls():
    urls = ["https://uni-tuebingen.de/a", "http://www.Uni-Tuebingen.de/b?x=1", "https://CS.UNI-TUEBINGEN.DE:8080/c",
            "https://notuni-tuebingen.de/d", "https://tuebingen.de/e", None, "", "not a url", "https://uni-tuebingen.de.evil.com/",
            "https://example.org/uni-tuebingen.de"]
    ix = _ix(len(urls), urls)
    ds = DocSet.from_sites(ix, ["Uni-Tuebingen.DE"])
    assert ds.indices().tolist() == [0, 1, 2]                # (a port does not hide the host)
    assert DocSet.from_sites(ix, "uni-tuebingen.de").indices().tolist() == [0, 1, 2]
    assert DocSet.from_sites(ix, ["tuebingen.de"]).indices().tolist() == [4]    # the site itself: uni-tuebingen.de is another domain
    assert DocSet.from_sites(ix, ["example.org", "cs.uni-tuebingen.de"]).indices().tolist() == [2, 9]
    assert DocSet.from_sites(ix, ["cs.uni-tuebingen.de:8080"]).indices().tolist() == []     # a site is a host name, no port
    assert len(DocSet.from_sites(ix, [])) == 0
    assert len(DocSet.from_sites(_ix(4, None), ["uni-tuebingen.de"])) == 0                  # no URLs: nothing matches


def test_operators():
    ix = _ix(70)
    rng = np.random.default_rng(1)
    a, b = rng.random(70) < 0.5, rng.random(70) < 0.3
    A, B = DocSet.from_mask(ix, a), DocSet.from_mask(ix, b)
    assert np.array_equal((A & B).mask, a & b)
    assert np.array_equal((A | B).mask, a | b)
    assert np.array_equal((A - B).mask, a & ~b)
    assert np.array_equal((~A).mask, ~a) and len(~A) == 70 - len(A)
    assert len(~DocSet.from_mask(ix, np.zeros(70, bool))) == 70
    assert A == DocSet.from_mask(ix, a.copy()) and A != B
    assert 69 not in DocSet.from_mask(ix, np.zeros(70, bool)) and -1 not in A and 70 not in ~A
    w = (~A).words()
    assert int(w[-1]) >> (70 % 32) == 0                       # the complement stays within [0, N)
    with pytest.raises(ValueError):
        A & DocSet.from_mask(_ix(70), b)                      # another index
    with pytest.raises(ValueError):
        DocSet.from_mask(ix, np.ones(69, bool))


def test_from_doc_ids_counts_unknown_ids():
    ix = _ix(50)
    ids = ix.doc_ids
    ds = DocSet.from_doc_ids(ix, [ids[3], ids[49], 11, 10_000, ids[0], -5])
    assert ds.indices().tolist() == [0, 3, 49] and ds.not_found == 3
    assert len(DocSet.from_doc_ids(ix, [])) == 0
    e = DocSet.from_doc_ids(_ix(0), [1, 2])
    assert len(e) == 0 and e.not_found == 2


def _tok_index(n_docs, seed=0):
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n_docs + 1, dtype=np.int64) * 7
    lens = rng.integers(1, 30, n_docs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = rng.zipf(1.5, int(off[-1])) % 300
    return bm25_index_from_token_ids(ids, off, tok.astype(np.int32), 300), ids, off, tok


def test_stale_docset_is_refused_after_remove_and_add():
    ix, ids, off, tok = _tok_index(200)
    ds = DocSet.from_mask(ix, np.ones(200, bool))
    ds.check(ix)
    pack_within(ds, 3, ix)
    smaller = remove_documents(ix, ids[:5])
    with pytest.raises(ValueError):
        ds.check(smaller)
    with pytest.raises(ValueError):
        pack_within([None, ds], 2, smaller)
    grown = bm25_add_token_ids(ix, np.array([99_999], np.int64), np.array([0, 3], np.int64), np.array([1, 2, 3], np.int32), 300)
    with pytest.raises(ValueError):
        pack_within(ds, 1, grown)
    same_size = CorpusIndex(doc_ids=ix.doc_ids)               # another index of the same size is another index
    with pytest.raises(ValueError):
        ds.check(same_size)
    DocSet.from_mask(smaller, np.ones(smaller.n_docs, bool)).check(smaller)


def test_pack_within_dedup_none_and_stride():
    for n in (0, 5, 32, 33, 100):
        ix = _ix(n)
        rng = np.random.default_rng(n)
        a = DocSet.from_mask(ix, rng.random(n) < 0.5)
        a2 = DocSet.from_mask(ix, a.mask.copy())             # equal content, another object: one row
        b = ~a
        words, q_set, n_sets, stride = pack_within([a, None, b, a2, None, a], 6, ix)
        assert stride == max(1, (n + 31) // 32) and words.shape == (n_sets, stride) and words.dtype == np.uint32
        assert n_sets == (1 if n == 0 else 2)
        assert q_set.dtype == np.int32 and q_set[1] == -1 and q_set[4] == -1
        assert q_set[0] == q_set[3] == q_set[5]
        assert np.array_equal(_unpack(words[q_set[0]], n), a.mask)
        assert np.array_equal(_unpack(words[q_set[2]], n), b.mask)
        w1, q1, n1, s1 = pack_within(a, 4, ix)
        assert n1 == 1 and q1.tolist() == [0, 0, 0, 0]
        w0, q0, n0, s0 = pack_within(None, 3, ix)
        assert n0 == 0 and q0.tolist() == [-1, -1, -1]
        w0, q0, n0, _ = pack_within([None, None], 2, ix)
        assert n0 == 0
    with pytest.raises(ValueError):
        pack_within([None], 2, _ix(3))
    with pytest.raises(TypeError):
        pack_within([np.ones(3, bool)], 1, _ix(3))


def test_restricted_bm25_contract_on_the_oracle_lists():
    """The contract msr_bm25_topk_within is tested against on the GPU, stated with numpy: the restricted top k = the first k
    entries of the full unrestricted list whose documents are in R -- which is the top k of R's documents by the unrestricted
    scores (idf and avgdl of the whole index), ties by ascending index, only documents that are touched and >= min_score."""
    from oracle import bm25_ref
    ix, ids, off, tok = _tok_index(3000, seed=4)
    z = {k: np.asarray(getattr(ix, k)) if not hasattr(getattr(ix, k), "numpy") else getattr(ix, k).numpy()
         for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")}
    z["avgdl"] = ix.avgdl
    rng = np.random.default_rng(5)
    for t in range(12):
        terms = rng.integers(0, 300, rng.integers(1, 6)).tolist()
        R = rng.random(3000) < [1.0, 0.5, 0.05, 0.001][t % 4]
        for min_score in (0.0, -1e9):
            fd, fs = bm25_full(z, terms, min_score)
            # the same from the per-document scores: R's touched documents with score >= min_score, by (score desc, index asc)
            acc, touched = bm25_ref.scores_dense(z, *bm25_ref.prepare_query(terms, z["term_off"]))
            ok = np.nonzero(touched & (acc >= min_score) & R)[0]
            direct = ok[np.lexsort((ok, -acc[ok]))]
            for k in (1, 10, 1000):
                wd, ws = restrict_list(fd, fs, len(fd), R, k)
                assert len(wd) <= k and R[wd].all()
                assert wd.tolist() == direct[:k].tolist()      # nothing of R ranked behind the whole corpus's top k is lost
                assert ws.tobytes() == acc[wd].tobytes()       # the unrestricted scores (idf, avgdl of the whole index)
            # with R = every document the restricted list is the unrestricted one
            ad, as_ = restrict_list(fd, fs, len(fd), np.ones(3000, bool), 50)
            assert ad.tolist() == fd[:50].tolist() and as_.tobytes() == fs[:50].tobytes()


def test_url_host_user_info_ports_and_unparsable_urls():
    from msretr.docset import url_host
    assert url_host("https://user:pw@CS.Uni-Tuebingen.DE:8443/x") == "cs.uni-tuebingen.de"
    assert url_host("http://uni-tuebingen.de:/y") == "uni-tuebingen.de"
    assert url_host("http://[::1]:8080/") == "[::1]"
    assert url_host("http://[::1/") is None                      # does not parse
    assert url_host("not a url") is None and url_host("") is None and url_host(None) is None
    urls = ["https://bob@uni-tuebingen.de/a", "http://[::1/", "not a url", "https://www.uni-tuebingen.de:8080/b"]
    ix = _ix(len(urls), urls)
    assert DocSet.from_sites(ix, ["uni-tuebingen.de"]).indices().tolist() == [0, 3]
    assert len(DocSet.from_sites(ix, ["defaultdomain"])) == 0     # an unparsable URL matches no site


def test_normalised_sites_and_host_table_built_once():
    from msretr.docset import normalise_sites
    assert normalise_sites(["Uni-Tuebingen.DE.", " example.org", "uni-tuebingen.de", "", "."]) == \
        ("example.org", "uni-tuebingen.de")
    assert normalise_sites("A.b") == ("a.b",)
    urls = [f"https://h{i % 7}.example.org/{i}" for i in range(500)]
    ix = _ix(500, urls)
    a = DocSet.from_sites(ix, ["h3.example.org"])
    table = ix._docset_hosts
    b = DocSet.from_sites(ix, ["H3.Example.org."])
    assert ix._docset_hosts is table                              # the URLs were parsed once
    assert a == b and a.indices().tolist() == list(range(3, 500, 7))
    assert len(DocSet.from_sites(ix, ["example.org"])) == 500
    ix.urls = urls[:499] + ["https://other.net/"]                 # another list: parsed again
    assert len(DocSet.from_sites(ix, ["example.org"])) == 499


class _FakeRetriever:
    """What /api/search needs of a Retriever, without a GPU: records the sets it is given."""

    def __init__(self, ix):
        self.index, self.seen = ix, []

    def search(self, query, top_k=1000, query_embedding=None, terms=None, query_id=None, **kw):
        self.seen.append(kw.get("within", "absent"))
        return []


def test_http_site_cache_is_bounded_and_keyed_on_normalised_sites():
    import gc
    import weakref
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    urls = [f"https://s{i % 50}.example.org/{i}" for i in range(1000)]
    ix = _ix(1000, urls)
    fake = _FakeRetriever(ix)
    app = create_app(fake, site_cache_size=4)
    client = TestClient(app)
    assert client.post("/api/search", json={"query": "q"}).status_code == 200
    assert fake.seen == ["absent"]                                # without sites: the call of before
    refs = []
    for i in range(20):
        assert client.post("/api/search", json={"query": "q", "sites": [f"s{i}.example.org"]}).status_code == 200
        refs.append(weakref.ref(fake.seen[-1]))
        assert len(fake.seen[-1]) == 20
    fake.seen.clear()
    gc.collect()
    cache = app.state.site_sets["sets"]
    assert len(cache) == 4 and sum(r() is not None for r in refs) == 4    # evicted sets are released
    client.post("/api/search", json={"query": "q", "sites": ["S19.Example.ORG.", "s19.example.org"]})
    client.post("/api/search", json={"query": "q", "sites": ["s18.example.org", "s19.example.org"]})
    client.post("/api/search", json={"query": "q", "sites": ["s19.example.org", "s18.example.org"]})
    assert fake.seen[0] is cache[("s19.example.org",)] and fake.seen[1] is fake.seen[2]
    assert len(cache) == 4 and len(fake.seen[1]) == 40
    fake.index = _ix(1000, urls)                                  # an update_index: the old sets go
    client.post("/api/search", json={"query": "q", "sites": ["s1.example.org"]})
    assert len(cache_now := app.state.site_sets["sets"]) == 1 and fake.seen[-1].index is fake.index
    assert cache_now is not cache

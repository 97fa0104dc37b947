"""Facet counts on the host (DESIGN K17): the numpy reference against a python-dict brute force on every corpus size, the
host function msr_facet_table against a numpy restatement on every size and value layout, facets.counting_terms and
facets.facet_values on hand-written inputs, the request parsing of /api/search, the C ABI's new signatures, and fuzzy.Results."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from facet_ref import (S, SIZES, base_mask, brute_force, corpus, facet_counts_ref, facet_rows, table_ref, top_ref,
                       value_layouts)
from msretr import _abi, facets, fuzzy
from msretr.index import CorpusIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", SIZES)
def test_reference_against_brute_force(N):
    c = corpus(N)
    rows = facet_rows(c)
    rows = rows if N <= 1025 else rows[::7]                  # (the python loops are slow on the large corpora)
    for name, value, n_values in value_layouts(N):
        if N > 1025 and name == "own value":
            rows_here = rows[::4]
        else:
            rows_here = rows
        for any_terms, b, claim in rows_here:
            base = base_mask(c, b)
            hits, counts = facet_counts_ref(c.z, value, n_values, any_terms, base)
            b_hits, b_cnt, b_top = brute_force(c.z, value, n_values, any_terms, base, limit=10)
            assert hits == b_hits, (N, name, claim)
            assert {v: int(n) for v, n in enumerate(counts) if n} == b_cnt, (N, name, claim)
            tv, tc, n_hit = top_ref(counts, 10)
            assert [(int(v), int(n)) for v, n in zip(tv, tc) if v >= 0] == b_top and n_hit == len(b_cnt), (N, name, claim)
            assert counts.sum() <= hits and (tv[len(b_top):] == -1).all() and (tc[len(b_top):] == 0).all()


def test_top_ref_breaks_ties_by_value():
    tv, tc, n = top_ref([0, 5, 7, 5, 0, 7], 3)
    assert tv.tolist() == [2, 5, 1] and tc.tolist() == [7, 7, 5] and n == 4
    assert top_ref([0, 0], 4)[0].tolist() == [-1] * 4 and top_ref([3], 0)[2] == 1


@pytest.mark.parametrize("N", SIZES)
def test_facet_table_against_numpy(N):
    lib = _abi.load()
    for name, value, n_values in value_layouts(N):
        want = table_ref(value, n_values)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        T = int(lib.msr_facet_table(p(value), N, n_values, None, None, None, None, None))      # the counting-only call
        assert T == len(want[2]) and T <= N, (N, name)
        got = facets.build_table(value, n_values)
        for g, w, what in zip(got, want, ("local", "span_off", "span_values", "value_off", "value_pos")):
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (N, name, what)
        local, span_off, span_values, value_off, value_pos = got
        # the contract, stated directly
        assert ((local == 0xFFFF) == (value < 0)).all() and (local[value >= 0] <= min(S, N) - 1).all()
        assert span_off[0] == 0 and span_off[-1] == T == value_off[-1] and value_off[0] == 0
        for s in range(len(span_off) - 1):
            sv = span_values[span_off[s]:span_off[s + 1]]
            assert (np.diff(sv) > 0).all()
            d = np.arange(s * S, min(N, (s + 1) * S))
            has = d[value[d] >= 0]
            assert (sv[local[has]] == value[has]).all()
        for v in set(value[value >= 0][:50].tolist()) | {0, n_values - 1}:
            pos = value_pos[value_off[v]:value_off[v + 1]]
            assert (np.diff(pos) > 0).all() and (span_values[pos] == v).all()
            assert len(pos) == len(np.unique(np.nonzero(value == v)[0] // S))


def test_facet_table_refusals():
    lib = _abi.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = np.array([0, 1, -1, 2], np.int32)
    assert lib.msr_facet_table(p(ok), 4, 3, None, None, None, None, None) == 3
    assert lib.msr_facet_table(p(np.array([0, 3], np.int32)), 2, 3, None, None, None, None, None) < 0      # value >= n_values
    assert lib.msr_facet_table(p(np.array([0, -2], np.int32)), 2, 3, None, None, None, None, None) < 0     # value < -1
    assert lib.msr_facet_table(None, 2, 3, None, None, None, None, None) < 0                                # NULL values
    local = np.zeros(4, np.uint16)
    assert lib.msr_facet_table(p(ok), 4, 3, p(local), None, None, None, None) < 0                           # NULL outputs
    with pytest.raises(ValueError):
        facets.build_table(np.array([0, 5], np.int32), 3)
    assert lib.msr_facet_table(None, 0, 0, None, None, None, None, None) == 0                               # an empty corpus


def _index(idf, urls=None):
    V = len(idf)
    N = 4 if urls is None else len(urls)
    ix = CorpusIndex(doc_ids=np.arange(N, dtype=np.int64), doc_len=np.full(N, 5, np.int32),
                     term_off=np.arange(V + 1, dtype=np.int64), post_doc=np.zeros(V, np.int32), post_tf=np.ones(V, np.int32),
                     idf=np.asarray(idf, np.float32), avgdl=5.0, total_docs=N)
    ix.urls = urls
    return ix


def test_counting_terms_drops_the_negative_idf_term():
    ix = _index([-0.4, 1.5, 0.0, 2.0])
    assert facets.counting_terms(ix, [0, 1, 3]) == [1, 3]                  # the city term does not count
    assert facets.counting_terms(ix, [3, 1, 3, 1, 0, -1, 4, 99]) == [3, 1]  # unique, valid, first occurrence first
    assert facets.counting_terms(ix, [0, 2]) == [0, 2]                     # no positive idf: all valid terms count
    assert facets.counting_terms(ix, [0]) == [0]
    assert facets.counting_terms(ix, [-1, 4]) == [] and facets.counting_terms(ix, []) == []


def test_facet_values_for_both_keys():
    urls = ["https://www.uni-tuebingen.de/a", "http://user:pw@Uni-Tuebingen.de:8080/b", "https://[2001:db8::1]:443/x", None,
            "", "/no/host", "https://tuebingen.de/", "https://www.uni-tuebingen.de/c", "not a url"]
    ix = _index([1.0], urls)
    value, names = facets.facet_values(ix)
    assert names == ["www.uni-tuebingen.de", "uni-tuebingen.de", "[2001:db8::1]", "tuebingen.de"]
    assert value.dtype == np.int32 and value.tolist() == [0, 1, 2, -1, -1, -1, 3, 0, -1]
    assert facets.facet_values(ix, "host")[0] is value                     # cached on the index
    dv, dn = facets.facet_values(ix, by="domain")
    # the rows' "domain" key as it is: www. goes, user info and port are NOT stripped (extract_domain_topic is the reference's)
    assert dn == ["uni-tuebingen", "userpwuni-tuebingen", "2001db81443", "tuebingen"]
    assert dv.tolist() == [0, 1, 2, -1, -1, -1, 3, 0, -1]
    assert facets.facet_values(ix, "domain")[0] is dv
    from msretr.text import extract_domain_topic
    assert all(dn[v] == extract_domain_topic(u) for v, u in zip(dv, urls) if v >= 0)
    with pytest.raises(ValueError):
        facets.facet_values(ix, by="tld")
    with pytest.raises(ValueError):
        facets.facet_values(_index([1.0]))                                 # no URLs
    for bad in (0, 65, True, 2.5, None):
        with pytest.raises(ValueError):
            facets.check_options("host", bad)
    with pytest.raises(ValueError):
        facets.check_options("tld", 10)
    facets.check_options("domain", 64)


class _FakeRetriever:
    """What create_app needs of a retriever, recording the keyword arguments of search."""
    index = None

    def __init__(self):
        self.calls = []

    def search(self, query, **kw):
        self.calls.append(kw)
        if kw.get("facets"):
            facets.check_options(kw["facet_by"], kw["facet_limit"])
            return fuzzy.Results([{"snippet": "s", "url": "u"}], hits=4312, facet_values=2,
                                 facets=[{"value": "uni-tuebingen.de", "count": 2104}, {"value": "tuebingen.de", "count": 611}])
        return [{"snippet": "s", "url": "u"}]


def test_http_request_parsing_and_400s():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    r = _FakeRetriever()
    client = TestClient(create_app(r))
    plain = client.post("/api/search", json={"query": "mensa"})
    assert plain.status_code == 200 and set(plain.json()) == {"llm_response", "documents"}
    assert not any(k.startswith("facet") for k in r.calls[-1])              # off by default: the call is what it was
    got = client.post("/api/search", json={"query": "mensa", "facets": True, "facet_by": "domain", "facet_limit": 5})
    assert got.status_code == 200
    assert r.calls[-1]["facets"] is True and r.calls[-1]["facet_by"] == "domain" and r.calls[-1]["facet_limit"] == 5
    body = got.json()
    assert body["hits"] == 4312 and body["facet_values"] == 2 and body["facets"][0] == {"value": "uni-tuebingen.de", "count": 2104}
    assert body["documents"] == [{"snippet": "s", "url": "u"}]
    dflt = client.post("/api/search", json={"query": "mensa", "facets": True})
    assert dflt.status_code == 200 and r.calls[-1]["facet_by"] == "host" and r.calls[-1]["facet_limit"] == 10
    for bad in ({"facet_limit": 0}, {"facet_limit": 65}, {"facet_by": "tld"}):
        resp = client.post("/api/search", json=dict({"query": "mensa", "facets": True}, **bad))
        assert resp.status_code == 400 and "facet" in resp.json()["error"], bad


def test_header_and_abi_agree():
    hdr = open(os.path.join(ROOT, "include", "msretr.h"), encoding="utf-8").read()
    assert int(re.search(r"#define MSR_FACET_MAX_LIMIT (\d+)", hdr).group(1)) == _abi.MSR_FACET_MAX_LIMIT == 64
    assert _abi.MSR_ABI_VERSION == 16
    for name, n_args in (("msr_facet_table", 8), ("msr_bind_facet", 9), ("msr_facet_scratch_bytes", 2), ("msr_facet_counts", 18)):
        m = re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(([^;]*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S),
                      flags=re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_abi._SIGNATURES[name][1]), name
    assert _abi._SIGNATURES["msr_facet_table"][0] is C.c_int64 and _abi._SIGNATURES["msr_facet_scratch_bytes"][0] is C.c_int64
    lib = _abi.load()
    assert all(hasattr(lib, n) for n in ("msr_facet_table", "msr_bind_facet", "msr_facet_scratch_bytes", "msr_facet_counts"))


def test_results_keeps_its_constructor_and_equals_its_list():
    rows = [{"rank": 1}, {"rank": 2}]
    old = fuzzy.Results(rows, {"tubingen": "tübingen"}, "mensa tübingen", {"bib*": {"terms": ["bibliothek"], "total": 1}})
    assert old == rows and list(old) == rows
    assert old.corrections == {"tubingen": "tübingen"} and old.corrected_query == "mensa tübingen" and "bib*" in old.expansions
    assert old.hits is None and old.facets == [] and old.facet_values == 0
    new = fuzzy.Results(rows, hits=12, facets=[{"value": "a.de", "count": 7}], facet_values=3)
    assert new == rows and new.hits == 12 and new.facets == [{"value": "a.de", "count": 7}] and new.facet_values == 3
    assert new.corrections == {} and new.corrected_query is None and new.expansions == {}
    assert fuzzy.Results() == []

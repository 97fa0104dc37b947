"""The near-duplicate collapse on the host (DESIGN K18): the oracle's plain loops against its vectorised form, the definition's
check constants, what signatures of equal and of disjoint streams look like, the greedy order, SearchOptions' new fields, the
C ABI's new signatures, fuzzy.Results, and the request parsing of /api/search."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dedup_ref as ref
from msretr import _abi, fuzzy
from msretr.query import SearchOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_constants():
    assert ref.A[0] == 0x514E28B7 and ref.B[0] == 0x30F4C306
    assert ref.A[63] == 0xE751D2A7 and ref.B[63] == 0x888A6A77
    assert all(a & 1 for a in ref.A)
    assert ref.fmix(0) == 0


@pytest.mark.parametrize("w", range(1, ref.MAX_SHINGLE + 1))
def test_signature_loops_against_numpy(w):
    rng = np.random.default_rng(100 + w)
    for n in [0, 1, max(w - 1, 0), w, w + 1, 63, 64, 65, 64 + w - 1, 130]:
        s = rng.integers(0, 50, n).astype(np.int32)          # few terms: repeated shingles
        a, b = ref.signature(s, w), ref.signature_fast(s, w)
        assert a.dtype == b.dtype == np.uint32 and (a == b).all(), (w, n)
        assert ref.is_empty(a) == (n == 0)
    big = np.array([2 ** 31 - 1, 0, 2 ** 31 - 1, 5], np.int32)      # token + 1 wraps into the sign bit, not past 2^32
    assert (ref.signature(big, w) == ref.signature_fast(big, w)).all()


def test_a_short_document_is_one_shingle_and_neighbours_do_not_leak():
    s = np.array([7, 8, 9], np.int32)
    assert len(ref.shingle_hashes(s, 8)) == 1 and len(ref.shingle_hashes(s, 3)) == 1 and len(ref.shingle_hashes(s, 2)) == 2
    assert ref.shingle_hashes(s, 8) == ref.shingle_hashes(s, 3)              # L = min(w, n) enters the hash, w does not
    assert ref.shingle_hashes(s, 8) != ref.shingle_hashes(np.array([7, 8, 9, 9], np.int32), 8)
    streams = ref.forward_index(n_terms=200, seed=2)
    assert len(streams[0]) == 0 and len(streams[-1]) == ref.LONG
    assert {len(s) for s in streams} >= {n for w in range(1, 9) for n in ref.stream_lengths(w)}
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    tok = np.concatenate(streams)
    sigs = ref.signatures_fast(off, tok, 4)
    cut = next(d for d in range(len(streams) - 2) if len(streams[d]) == 9 and len(streams[d + 2]) == 19)
    assert (np.concatenate(streams[cut:cut + 2]) == streams[cut + 2]).all() and ref.matches(sigs[cut], sigs[cut + 2]) < 64
    for d in range(len(off) - 1):                            # each document alone gives the row it has inside the buffer
        if off[d + 1] - off[d] <= 400:                       # (the plain loops are slow on the 5000-token document)
            assert (sigs[d] == ref.signature(tok[off[d]:off[d + 1]], 4)).all(), d
    assert (ref.signatures_fast(off, tok, 4, 3, 7) == sigs[3:7]).all() and ref.signatures_fast(off, tok, 4, 5, 5).shape == (0, 64)


def test_identical_streams_match_fully_and_disjoint_streams_not_at_all():
    rng = np.random.default_rng(11)
    zero = 0
    for _ in range(60):
        a = rng.integers(0, 1000, 80).astype(np.int32)
        b = rng.integers(1000, 2000, 80).astype(np.int32)    # no token in common, so no shingle in common
        sa, sb = ref.signature_fast(a, 4), ref.signature_fast(b, 4)
        assert ref.matches(sa, ref.signature_fast(a.copy(), 4)) == 64
        zero += ref.matches(sa, sb)
    assert zero == 0
    base = rng.integers(0, 5000, 200).astype(np.int32)
    near = base.copy()
    near[100] = 4999 - near[100]                              # one token of 200: 4 of ~197 shingles differ
    m = ref.matches(ref.signature_fast(base, 4), ref.signature_fast(near, 4))
    assert 55 <= m <= 64, m                                  # J = 193 / 201 = 0.96, 64 J = 61.4, sigma = 8 sqrt(J (1 - J)) = 1.6: 4 sigma


def _table(rows):
    t = np.zeros((len(rows), 64), np.uint32)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def test_greedy_chain_and_the_smaller_leader():
    a = np.arange(64, dtype=np.uint32)
    b = a.copy(); b[:3] += 1000                              # a ~ b: 61
    c = b.copy(); c[3:6] += 2000                             # b ~ c: 61, a ~ c: 58
    sig = _table([a, b, c])
    for fn in (ref.collapse, ref.collapse_fast):
        assert fn([0, 1, 2], sig, 60) == ([0, 2], [(1, 0, 61)])           # A ~ B ~ C, A !~ C: a dropped row leads nothing
        assert fn([0, 1, 2], sig, 58) == ([0], [(1, 0, 61), (2, 0, 58)])
        assert fn([2, 1, 0], sig, 60) == ([0, 2], [(1, 0, 61)])           # slots, not documents
        assert fn([0, 1, 2], sig, 64) == ([0, 1, 2], [])
        assert fn([], sig, 1) == ([], [])
    d = a.copy(); d[60:] += 7                                # d ~ a: 60, d ~ e: 60, a !~ e: 56
    e = d.copy(); e[56:60] += 9
    sig = _table([a, e, d])
    for fn in (ref.collapse, ref.collapse_fast):
        assert fn([0, 1, 2], sig, 60) == ([0, 1], [(2, 0, 60)])           # two leaders: the smaller slot
        assert fn([1, 0, 2], sig, 60) == ([0, 1], [(2, 0, 60)])


def test_passive_slots_stay_and_lead_nothing():
    a = np.arange(64, dtype=np.uint32)
    sig = _table([a, a, ref.EMPTY, ref.EMPTY, a])
    for fn in (ref.collapse, ref.collapse_fast):
        assert fn([2, 3, 0, 1], sig, 64) == ([0, 1, 2], [(3, 2, 64)])      # EMPTY rows equal each other and are no duplicates
        assert fn([9, 0, -1, 9, 1], sig, 64) == ([0, 1, 2, 3], [(4, 1, 64)])      # outside the table
        assert fn([0, 1, 4], sig, 64, passive=[True, False, False]) == ([0, 1], [(2, 1, 64)])      # a rejected page leads nothing
        assert fn([0, 1, 4], sig, 64, passive=[False, True, False]) == ([0, 1], [(2, 0, 64)])      # ... and is never dropped


def test_collapse_loops_against_numpy_on_random_lists():
    streams, _ = ref.near_copies(12, 3, length=60, edits=1, n_terms=300, seed=5)
    streams.append(np.zeros(0, np.int32))
    sig = np.stack([ref.signature_fast(s, 4) for s in streams])
    rng = np.random.default_rng(6)
    for mm in (1, 40, 58, 64):
        for _ in range(4):
            docs = rng.integers(-1, len(streams) + 2, 70)
            passive = rng.random(70) < 0.1
            assert ref.collapse(docs, sig, mm, passive) == ref.collapse_fast(docs, sig, mm, passive), mm
    out = ref.collapse_lists(np.array([[0, 1, 2, 5]]), np.array([[.9, .8, .7, .6]]), np.zeros((1, 4)), np.array([[3, 4, 5, 6]]),
                             [9], sig, 40)
    kept = int(out[4][0])
    assert kept + int(out[8][0]) == 4 and (out[0][0, kept:] == -1).all() and np.isneginf(out[1][0, kept:]).all()
    assert (out[3][0, kept:] == -1).all() and (out[5][0, int(out[8][0]):] == -1).all() and (out[7][0, int(out[8][0]):] == 0).all()


def test_search_options_threshold():
    assert SearchOptions().collapse_duplicates is False and SearchOptions().duplicate_threshold == 0.9
    mm = lambda t: SearchOptions(collapse_duplicates=True, duplicate_threshold=t).min_matches
    assert mm(0.9) == 58 and mm(1.0) == 64 and mm(1 / 64) == 1 and mm(0.5) == 32 and mm(0.001) == 1
    for ok in (0.9, 1, 1.0, 1 / 64, np.float32(0.5)):
        SearchOptions(collapse_duplicates=True, duplicate_threshold=ok).check()
    for bad in (0, 0.0, -0.1, 1.01, 2, None, "0.9", True, float("nan")):
        with pytest.raises(ValueError, match="duplicate_threshold"):
            SearchOptions(collapse_duplicates=True, duplicate_threshold=bad).check()
        SearchOptions(duplicate_threshold=bad).check()       # off: the value is not looked at
    # the positional order of the older fields is what it was
    o = SearchOptions("hybrid", 50, True, False, False, True, 20, False, True, 4, True, "domain", 7)
    assert (o.mode, o.dense_k, o.snippet_tokens, o.max_expansions, o.facet_by, o.facet_limit) == ("hybrid", 50, 20, 4, "domain", 7)
    assert o.collapse_duplicates is False


def test_header_and_abi_agree():
    hdr = open(os.path.join(ROOT, "include", "msretr.h"), encoding="utf-8").read()
    for name, value in (("MSR_SIG_WORDS", 64), ("MSR_SIG_MAX_SHINGLE", 8), ("MSR_COLLAPSE_MAX_CAND", 1024)):
        assert int(re.search(r"#define " + name + r" (\d+)", hdr).group(1)) == getattr(_abi, name) == value
    assert _abi.MSR_ABI_VERSION == 16 and int(re.search(r"#define MSR_ABI_VERSION (\d+)", hdr).group(1)) == 16
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("msr_doc_signatures", 6), ("msr_bind_signatures", 4), ("msr_collapse_scratch_bytes", 2),
                         ("msr_collapse_duplicates", 21)):
        m = re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(([^;]*?)\);", bare, flags=re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_abi._SIGNATURES[name][1]), name
    assert _abi._SIGNATURES["msr_collapse_scratch_bytes"][0] is C.c_int64
    lib = _abi.load()
    assert all(hasattr(lib, n) for n in ("msr_doc_signatures", "msr_bind_signatures", "msr_collapse_scratch_bytes",
                                         "msr_collapse_duplicates"))
    # the scratch size is a host function of the shape alone
    assert lib.msr_collapse_scratch_bytes(3, 300) == (3 * 300 * 10 * 4 + 15) // 16 * 16
    assert lib.msr_collapse_scratch_bytes(0, 1) == 0 and lib.msr_collapse_scratch_bytes(256, 1000) == 256 * 1000 * 32 * 4
    for bad in ((-1, 10), (1, 0), (1, 1025)):
        assert lib.msr_collapse_scratch_bytes(*bad) < 0


def test_results_keeps_its_constructor_and_gains_collapsed():
    rows = [{"rank": 1}, {"rank": 2}]
    old = fuzzy.Results(rows, {"tubingen": "tübingen"}, "mensa tübingen", {"bib*": {"terms": ["bibliothek"], "total": 1}}, 12,
                        [{"value": "a.de", "count": 7}], 3)
    assert old == rows and old.corrections == {"tubingen": "tübingen"} and old.corrected_query == "mensa tübingen"
    assert "bib*" in old.expansions and old.hits == 12 and old.facets == [{"value": "a.de", "count": 7}] and old.facet_values == 3
    assert old.collapsed == 0 and fuzzy.Results().collapsed == 0 and fuzzy.Results.collapsed == 0
    new = fuzzy.Results(rows, collapsed=5)
    assert new == rows and new.collapsed == 5 and new.hits is None and new.corrections == {}


def test_sharded_search_refuses_the_option():
    from msretr.distributed import ShardedEngine
    with pytest.raises(ValueError, match="collapse_duplicates"):
        ShardedEngine.search(object(), [[1]], None, collapse_duplicates=True)


class _FakeRetriever:
    """What create_app needs of a retriever, recording the keyword arguments of search."""
    index = None

    def __init__(self):
        self.calls = []

    def search(self, query, **kw):
        self.calls.append(kw)
        if kw.get("collapse_duplicates"):
            SearchOptions(collapse_duplicates=True, duplicate_threshold=kw["duplicate_threshold"]).check()
            dup = {"doc_id": "8", "url": "http://uni-tuebingen.de/a", "title": "A", "similarity": 1.0}
            return fuzzy.Results([{"snippet": "s", "url": "https://www.uni-tuebingen.de/a", "duplicates": [dup]}], collapsed=1)
        return [{"snippet": "s", "url": "u"}]


def test_http_request_parsing_and_400s():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    r = _FakeRetriever()
    client = TestClient(create_app(r))
    plain = client.post("/api/search", json={"query": "mensa"})
    assert plain.status_code == 200 and set(plain.json()) == {"llm_response", "documents"}
    assert not any("duplicate" in k for k in r.calls[-1])    # off by default: the call is what it was
    also = client.post("/api/search", json={"query": "mensa", "duplicate_threshold": 0.5})
    assert also.status_code == 200 and not any("duplicate" in k for k in r.calls[-1]) and "collapsed" not in also.json()
    got = client.post("/api/search", json={"query": "mensa", "collapse_duplicates": True, "duplicate_threshold": 0.75})
    assert got.status_code == 200
    assert r.calls[-1]["collapse_duplicates"] is True and r.calls[-1]["duplicate_threshold"] == 0.75
    body = got.json()
    assert body["collapsed"] == 1 and body["documents"][0]["duplicates"][0]["url"] == "http://uni-tuebingen.de/a"
    dflt = client.post("/api/search", json={"query": "mensa", "collapse_duplicates": True})
    assert dflt.status_code == 200 and r.calls[-1]["duplicate_threshold"] == 0.9
    for bad in (0, 1.5, -1):
        resp = client.post("/api/search", json={"query": "mensa", "collapse_duplicates": True, "duplicate_threshold": bad})
        assert resp.status_code == 400 and "duplicate_threshold" in resp.json()["error"], bad


# ---- planted tables and lists (tests/test_gpu_collapse_edges.py runs them on the GPU) --------------------------------------------
def test_planted_table_holds_the_counts_it_claims():
    sig, rows = ref.planted_table()
    assert sig.dtype == np.uint32 and sig.shape[1] == 64
    count = lambda a, b: int((sig[a] == sig[b]).sum())
    assert sorted(rows["pairs"]) == [(m, side) for m in range(65) for side in ("first", "last")]
    for (m, side), (a, b) in rows["pairs"].items():
        eq = sig[a] == sig[b]
        assert eq.sum() == m and (eq[:m].all() if side == "first" else eq[64 - m:].all()), (m, side)
        assert ref.matches(sig[a], sig[b]) == m
    assert ref.pair_matches(rows).tolist() == [m for m in range(65) for _ in range(2)]
    x, y, z = rows["ones"]
    assert sig[x][0] == ref.M32 and sig[z][63] == ref.M32 and count(x, y) == 64 and count(x, z) == 0
    assert not ref.is_empty(sig[x]) and not ref.is_empty(sig[z]) and all(ref.is_empty(sig[r]) for r in rows["empty"])
    a, b, c = rows["chain"]
    assert (count(a, b), count(b, c), count(a, c)) == (61, 61, 58)
    a, e, d = rows["two"]
    assert (count(d, a), count(d, e), count(a, e)) == (60, 60, 56)
    # nothing else matches: every row pair outside the planted ones (the EMPTY rows apart) has count 0
    m = (sig[:, None, :] == sig[None, :, :]).sum(axis=2)
    np.fill_diagonal(m, 0)
    planted = set(map(tuple, rows["pairs"].values())) | {(x, y), (a, d), (e, d), (a, e), rows["empty"]} | \
        {(rows["chain"][i], rows["chain"][j]) for i in range(3) for j in range(i + 1, 3)}
    for i, j in np.argwhere(np.triu(m) > 0).tolist():
        if i not in rows["empty"] and j not in rows["empty"]:                 # (an EMPTY row equals the 0xFFFFFFFF words of `ones`)
            assert (i, j) in planted or (j, i) in planted, (i, j, int(m[i, j]))
    assert len(rows["fill"]) >= 1024


def test_planted_pairs_drop_exactly_from_their_count_on():
    sig, rows = ref.planted_table()
    M = 272                                                  # 9 words per row: the last tile owns one word
    doc, n = ref.planted_pair_lists(rows, M)
    assert doc.shape == (3, M) and n.tolist() == [260, 260, 261] and (M + 31) // 32 % 2 == 1
    want = ref.pair_matches(rows)
    z = np.zeros((3, M))
    for mm in (1, 2, 33, 64):
        out = ref.collapse_lists(doc, z, z, doc, n, sig, mm)
        for q in range(3):
            dropped = {int(d): int(k) for d, k in zip(out[5][q, :out[8][q]], out[7][q, :out[8][q]])}
            for (a, b), m in zip((rows["pairs"][k] for k in sorted(rows["pairs"])), want):
                assert (b in dropped) == (m >= mm) and a not in dropped
                if b in dropped:
                    assert dropped[b] == m
            assert out[8][q] == 2 * (65 - mm)
    # the pairs of the second list stand in different tiles, some of the third straddle a tile edge
    assert all(abs(int(np.nonzero(doc[1] == a)[0][0]) // 64 - int(np.nonzero(doc[1] == b)[0][0]) // 64) >= 2 for a, b in rows["pairs"].values())
    assert any(int(np.nonzero(doc[2] == a)[0][0]) % 64 == 63 for a, _ in rows["pairs"].values())


def test_full_width_list_and_the_many_queries():
    sig, rows = ref.planted_table()
    doc = ref.full_width_list(rows, len(sig))[None, :]
    z = np.zeros((1, 1024))
    out = ref.collapse_lists(doc, z, z, doc, [1024], sig, 60)
    drops = [(int(np.nonzero(doc[0] == d)[0][0]), int(np.nonzero(doc[0] == l)[0][0]), int(m))
             for d, l, m in zip(out[5][0, :out[8][0]], out[6][0, :out[8][0]], out[7][0, :out[8][0]])]
    assert drops == [(100, 10, 61), (990, 20, 60), (1000, 600, 64)]          # (slot, leader slot, matches) in drop order
    assert {s // 64 for s in (10, 100, 700)} == {0, 1, 10} and 1000 // 64 == 15 and 600 >= 512
    assert all(int(doc[0, s]) in out[0][0, :out[4][0]] for s in (63, 64, 1023, 700, 530))      # passive slots and C stay
    out58 = ref.collapse_lists(doc, z, z, doc, [1024], sig, 58)
    assert out58[8][0] == 4 and int(doc[0, 700]) in out58[5][0, :4]          # at 58 the chain's C goes as well
    q = ref.many_pair_queries(rows, 32770)
    assert q.shape == (32770, 2) and len({tuple(r) for r in q[32767:32770].tolist()}) == 3
    out = ref.collapse_lists(q[32766:], np.zeros((4, 2)), np.zeros((4, 2)), q[32766:], [2] * 4, sig, 32)
    assert out[8].tolist() == [0, 0, 0, 1] and out[7][3, 0] == 33            # the rows on the slice's two sides differ in outcome

"""Host-side logic and the C-ABI surface, no GPU: text helpers and diversification against the goldens,
every symbol of include/msretr.h exported by libmsretr.so, error behaviour without a device."""
import ctypes as C
import json
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load(name):
    with open(os.path.join(G, name), encoding="utf-8") as f:
        return json.load(f)


def test_text_helpers_match_reference_outputs():
    from msretr.text import extract_domain, extract_domain_topic, preprocess_query
    s = _load("search_api.json")
    for q, exp in s["preprocess_query"]:
        assert preprocess_query(q) == exp
    for u, exp in s["extract_domain_topic"]:
        assert extract_domain_topic(u) == exp
    for u, exp in _load("diversification.json")["extract_domain"]:
        assert extract_domain(u) == exp


def test_queries_txt_shape(tmp_path):
    from msretr.text import format_result_line, read_queries_file
    p = tmp_path / "queries.txt"
    p.write_text("1\ttübingen attractions\n\n2\tfood and drinks\nbroken line\n", encoding="utf-8")
    assert read_queries_file(str(p)) == [("1", "tübingen attractions"), ("2", "food and drinks")]
    assert format_result_line("7", 3, "https://a.de/x", 0.123456) == "7\t3\thttps://a.de/x\t0.123"


def test_sliding_windows_match_reference_outputs():
    from msretr.text import create_sliding_windows
    for c in _load("windows.json"):
        wins = create_sliding_windows(list(range(c["n"])), c["window"], c["step"])
        assert [w[0] if w else -1 for w in wins] == c["starts"] and [len(w) for w in wins] == c["lens"]


def test_diversify_matches_reference_outputs():
    from msretr.reranker import diversify
    for c in _load("diversification.json")["cases"]:
        docs = [{"doc_id": str(i), "url": u, "similarity_score": s} for i, u, s in c["input"]]
        got = diversify(docs, top_k=c["top_k"])
        assert [[int(x["doc_id"]), x["similarity_score"]] for x in got] == c["expected"]


def test_library_exports_every_declared_symbol():
    from msretr import _abi
    hdr = "".join(open(os.path.join(ROOT, "include", h), encoding="utf-8").read() for h in ("msretr.h", "msretr_encoder.h"))
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(msr_\w+)\s*\(", hdr, flags=re.M))
    assert declared, "no prototypes found in msretr.h"
    lib = _abi.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in msretr.h but not exported"
    assert declared == set(_abi.EXPORTS), declared ^ set(_abi.EXPORTS)
    assert lib.msr_abi_version() == _abi.MSR_ABI_VERSION


def test_create_rejects_bad_config_and_reports_why():
    from msretr import _abi
    lib = _abi.load()
    h = C.c_void_p()
    cfg = _abi.MsrConfig(C.sizeof(_abi.MsrConfig), 0, 512, 8, 100, 100, 0, 0)       # wrong dim
    assert lib.msr_create(C.byref(cfg), C.byref(h)) == -1
    assert b"dim" in lib.msr_last_error(None)
    cfg = _abi.MsrConfig(4, 0, 768, 8, 100, 100, 0, 0)                               # wrong struct size
    assert lib.msr_create(C.byref(cfg), C.byref(h)) == -1
    cfg = _abi.MsrConfig(C.sizeof(_abi.MsrConfig), 0, 768, 8, 100, 100, 0, 0, 0x40)  # a flag bit this ABI does not know
    assert lib.msr_create(C.byref(cfg), C.byref(h)) == -1 and b"flag" in lib.msr_last_error(None)
    assert lib.msr_owned_bytes(None) == -1 and lib.msr_row_copy_state(None) == -1 and lib.msr_row_image_state(None) == -1
    assert lib.msr_destroy(None) == 0


def test_no_cpu_fallback():
    """Without a GPU the product path refuses to run (it must never route through the oracle)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from msretr._abi import MsrError
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    ix = CorpusIndex(doc_ids=np.arange(3, dtype=np.int64))
    with pytest.raises(MsrError):
        DeviceEngine(ix)
    src = ""
    pkg = os.path.join(ROOT, "modern-search-engines-project_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src += open(os.path.join(pkg, fn), encoding="utf-8").read()
    assert "import oracle" not in src and "from oracle" not in src


def test_index_roundtrip_and_url_groups(tmp_path):
    from msretr.index import CorpusIndex
    ix = CorpusIndex.from_tables({"a": [(5, 1), (9, 2)], "b": [(9, 1)]}, {5: 3, 9: 4, 12: 1}, {"a": 0.5, "b": None}, 3.0,
                                 chunks=[(100, 9), (101, 9), (50, 5)], emb={100: np.ones(768), 101: np.zeros(768), 50: np.ones(768) * 2},
                                 urls_db={5: ("http://x.de/a?q=1", "t5", "x"), 9: ("http://x.de/a", None, "y")})
    assert ix.doc_ids.tolist() == [5, 9, 12] and ix.doc_off.tolist() == [0, 1, 3, 3]
    assert ix.chunk_ids.tolist() == [50, 100, 101]
    assert ix.url_group().tolist() == [0, 0, -1]                 # same URL modulo query string; 12 not in urlsDB
    assert ix.idf.tolist() == [0.5, 0.0]                         # NULL idf -> 0.0
    p = str(tmp_path / "snap.npz")
    ix.save(p)
    jx = CorpusIndex.load(p)
    assert jx.post_doc.tolist() == ix.post_doc.tolist() and jx.vocab == ix.vocab and jx.avgdl == ix.avgdl
    assert np.array_equal(jx.emb, ix.emb)


def test_snapshot_directory_roundtrip_and_streaming_upload(tmp_path):
    """the export format (one .npy per array + meta.json + docs.jsonl) maps back without reading the files,
    and stream_to_device moves a mapped array block by block (here to the CPU device: same code, unpinned buffers)."""
    import torch
    from msretr.engine import stream_to_device
    from msretr.index import CorpusIndex
    from msretr.synthetic import synthetic_corpus
    ix = synthetic_corpus(300, n_chunks=1100, n_terms=500, device="cpu")
    ix.urls = [f"https://example.org/{i}?x=1" if i % 7 else None for i in range(ix.n_docs)]
    ix.titles = [f"t{i}" if i % 5 else None for i in range(ix.n_docs)]
    ix.texts = [("Tübingen " * (i % 3)) or None for i in range(ix.n_docs)]
    ix.vocab = {f"w{i}": i for i in range(ix.n_terms)}
    d = str(tmp_path / "snap")
    ix.save_dir(d, block_rows=128)                             # several blocks per array
    back = CorpusIndex.load_dir(d, mmap=True)
    assert isinstance(back.emb, np.memmap) and back.emb.dtype == np.float32 and back.emb.shape == (1100, 768)
    for name in CorpusIndex._ARRAYS:
        a, b = getattr(ix, name), getattr(back, name)
        assert np.array_equal(np.asarray(a.cpu() if hasattr(a, "cpu") else a), np.asarray(b)), name
    assert (back.avgdl, back.total_docs, back.k1, back.b) == (ix.avgdl, ix.total_docs, ix.k1, ix.b)
    assert back.urls == ix.urls and back.titles == ix.titles and back.texts == ix.texts and back.vocab == ix.vocab
    assert np.array_equal(back.url_group(), ix.url_group())
    for arr in (back.emb, back.post_doc, back.term_off):
        t = stream_to_device(arr, "cpu", block_bytes=100_000)  # forces many blocks, ragged last one
        assert t.shape == arr.shape and np.array_equal(t.numpy(), np.asarray(arr))
    assert stream_to_device(np.zeros((0, 768), np.float32), "cpu").shape == (0, 768)
    with pytest.raises(ValueError):
        (tmp_path / "bad").mkdir()
        (tmp_path / "bad" / "meta.json").write_text("{}")
        CorpusIndex.load_dir(str(tmp_path / "bad"))


def test_duckdb_loader_runs_against_the_reference_schema(tmp_path):
    """CorpusIndex.from_duckdb executes its SQL (duckdb itself is not installable here): a sqlite3 database with the
    reference's tables and column names (bm25_indexer.py:86-126, embedder.py:31-52, databaseManagement.py:18-51; the
    FLOAT[768] column held as a float32 blob) behind a DuckDB-shaped adapter must load into the same index as
    from_tables on the same rows."""
    import sqlite3
    from msretr.index import CorpusIndex
    rng = np.random.default_rng(12)
    postings = {"castle": [(7, 2), (3, 1)], "tübingen": [(3, 4), (7, 1), (11, 2), (40, 1)], "garden": [(40, 3)]}
    doc_len = {3: 10, 7: 12, 11: 5, 40: 9}
    idf = {"castle": 0.25, "tübingen": -0.56, "garden": None}
    chunks = [(100, 7), (101, 7), (55, 3), (300, 40), (301, 40), (302, 40)]
    emb = {c: rng.standard_normal(768).astype(np.float32) for c, _ in chunks}
    urls = {3: ("http://a.de/x?p=1", "t3", "text three"), 7: ("http://a.de/x", None, "text seven"), 40: ("http://b.de/", "t40", None)}
    db = str(tmp_path / "crawlerDb.sqlite")
    con = sqlite3.connect(db)
    con.executescript("""
        CREATE TABLE bm25_doc_stats (doc_id INTEGER PRIMARY KEY, doc_length INTEGER, processed_at TIMESTAMP DEFAULT CURRENT_TIMESTAMP);
        CREATE TABLE bm25_term_freq (doc_id INTEGER, term TEXT, freq INTEGER, PRIMARY KEY (doc_id, term));
        CREATE TABLE bm25_term_stats (term TEXT PRIMARY KEY, doc_freq INTEGER, total_freq INTEGER, idf_score REAL, last_updated TIMESTAMP DEFAULT CURRENT_TIMESTAMP);
        CREATE TABLE bm25_corpus_stats (stat_name TEXT PRIMARY KEY, stat_value REAL, last_updated TIMESTAMP DEFAULT CURRENT_TIMESTAMP);
        CREATE TABLE chunks_optimized (chunk_id BIGINT PRIMARY KEY, doc_id BIGINT, chunk_text TEXT);
        CREATE TABLE embeddings (chunk_id BIGINT PRIMARY KEY, embedding BLOB);
        CREATE TABLE urlsDB (id BIGINT PRIMARY KEY, url TEXT UNIQUE, title TEXT, text TEXT, lastFetch DOUBLE, incoming TEXT,
                             domainLinkingDepth TINYINT, linkingDepth TINYINT, tueEngScore DOUBLE);
    """)
    con.executemany("INSERT INTO bm25_doc_stats (doc_id, doc_length) VALUES (?, ?)", list(doc_len.items()))
    con.executemany("INSERT INTO bm25_term_freq VALUES (?, ?, ?)", [(d, t, f) for t, pl in postings.items() for d, f in pl])
    con.executemany("INSERT INTO bm25_term_stats (term, doc_freq, total_freq, idf_score) VALUES (?, ?, ?, ?)",
                    [(t, len(pl), sum(f for _, f in pl), idf[t]) for t, pl in postings.items()])
    con.executemany("INSERT INTO bm25_corpus_stats (stat_name, stat_value) VALUES (?, ?)",
                    [("avg_doc_length", 9.0), ("total_docs", 4.0)])
    con.executemany("INSERT INTO chunks_optimized VALUES (?, ?, ?)", [(c, d, f"chunk {c}") for c, d in chunks])
    con.executemany("INSERT INTO embeddings VALUES (?, ?)", [(c, emb[c].tobytes()) for c, _ in chunks])
    con.executemany("INSERT INTO urlsDB (id, url, title, text) VALUES (?, ?, ?, ?)", [(i, *u) for i, u in urls.items()])
    con.commit(); con.close()

    class Cur:
        def __init__(self, cur):
            self.cur = cur

        def fetchall(self):
            return self.cur.fetchall()

        def fetchnumpy(self):                                  # DuckDB: dict column name -> numpy array
            rows = self.cur.fetchall()
            out = {}
            for i, d in enumerate(self.cur.description):
                col = [r[i] for r in rows]
                if d[0] == "embedding":                        # FLOAT[768] comes back as one array per row
                    arr = np.empty(len(col), dtype=object)
                    arr[:] = [np.frombuffer(b, np.float32) for b in col]
                    out[d[0]] = arr
                else:
                    out[d[0]] = np.array(col)
            return out

    class Conn:
        def __init__(self, path):
            self.con = sqlite3.connect(path)

        def execute(self, sql, params=()):
            return Cur(self.con.execute(sql, params))

    got = CorpusIndex.from_duckdb(db, connect=Conn)
    ref = CorpusIndex.from_tables(postings, doc_len, idf, 9.0, chunks=chunks, emb=emb, urls_db=urls)
    assert got.doc_ids.tolist() == ref.doc_ids.tolist() == [3, 7, 11, 40]
    assert got.doc_len.tolist() == ref.doc_len.tolist() and got.avgdl == ref.avgdl == 9.0 and got.total_docs == 4
    assert set(got.vocab) == set(ref.vocab)
    for t in postings:                                          # same posting list and idf per term (term ids differ: ORDER BY term)
        a, b = got.vocab[t], ref.vocab[t]
        sl = lambda ix, i: (np.asarray(ix.post_doc)[ix.term_off[i]:ix.term_off[i + 1]].tolist(),
                            np.asarray(ix.post_tf)[ix.term_off[i]:ix.term_off[i + 1]].tolist())
        assert sl(got, a) == sl(ref, b) and np.float32(got.idf[a]) == np.float32(ref.idf[b])
    assert got.doc_off.tolist() == ref.doc_off.tolist() and got.chunk_ids.tolist() == ref.chunk_ids.tolist()
    assert np.array_equal(got.emb, ref.emb)
    assert got.urls == ref.urls and got.titles == ref.titles and got.texts == ref.texts
    assert got.url_group().tolist() == ref.url_group().tolist()


def test_bm25_index_build_matches_reference_tables():
    """Index build from tokens reproduces the tables the goldens' corpora were described with."""
    from msretr.index_build import bm25_index_from_tokens, normalise_document_text
    from oracle import bm25_ref
    case = next(c for c in _load("bm25_kat.json") if c["name"] == "null_idf_lengths")
    docs = {}
    for t, pl in case["postings"].items():
        if t == "nullidf":            # that fixture row is a hand-made NULL-idf case, not a tokenisable term
            continue
        for d, tf in pl:
            docs.setdefault(d, []).extend([t] * tf)
    doc_len = {int(d): l for d, l in case["doc_len"].items()}
    for d, l in doc_len.items():                                  # pad with filler terms up to doc_length
        docs.setdefault(d, [])
        docs[d] += [f"filler{d}_{i}" for i in range(l - len(docs[d]))]
    ix = bm25_index_from_tokens(list(docs), list(docs.values()))
    assert ix.doc_ids.tolist() == sorted(doc_len) and ix.doc_len.tolist() == [doc_len[d] for d in sorted(doc_len)]
    assert ix.avgdl == case["avgdl_f32"]
    for t in ("a", "b"):
        lo, hi = ix.term_off[ix.vocab[t]], ix.term_off[ix.vocab[t] + 1]
        got = [(int(ix.doc_ids[d]), int(tf)) for d, tf in zip(ix.post_doc[lo:hi], ix.post_tf[lo:hi])]
        assert got == [tuple(p) for p in case["postings"][t]]
    # idf follows the stored-REAL formula with N = number of indexed documents
    import math
    N = len(doc_len)
    for t in ("a", "b"):
        df = len(case["postings"][t])
        assert float(ix.idf[ix.vocab[t]]) == float(np.float32(math.log10((N - df + 0.5) / (df + 0.5))))
    assert normalise_document_text("Tuebingen", "TUBINGEN x") == "tübingen tübingen x"
    assert bm25_index_from_tokens([1, 2], [[], ["x"]]).doc_ids.tolist() == [2]     # empty documents get no row


def test_bm25_index_build_from_token_ids_equals_the_token_list_builder():
    """the sort-based builder (runs on the GPU at corpus scale; here on the CPU device) against the
    dict-based one that is pinned to the reference's tables: same postings, lengths, idf bits, avgdl."""
    from msretr.index_build import bm25_index_from_token_ids, bm25_index_from_tokens
    rng = np.random.default_rng(9)
    n = 400
    doc_ids = rng.permutation(np.arange(1000, 1000 + 3 * n, 3))[:n]      # unsorted, with gaps
    lens = rng.integers(0, 60, size=n); lens[[3, 77]] = 0                 # two token-less documents: no row
    toks = [rng.zipf(1.3, size=l).clip(1, 300).tolist() for l in lens]
    ref = bm25_index_from_tokens(doc_ids, [[f"w{t}" for t in tl] for tl in toks])
    ids_of = {f"w{t}": i for t, i in ((int(k[1:]), v) for k, v in ref.vocab.items())}    # the dict builder's numbering
    tok_off = np.zeros(n + 1, np.int64); tok_off[1:] = np.cumsum(lens)
    tok_ids = np.array([ids_of[f"w{t}"] for tl in toks for t in tl], np.int32)
    got = bm25_index_from_token_ids(doc_ids, tok_off, tok_ids, len(ref.vocab), device="cpu")
    assert got.total_docs == ref.total_docs == int((lens > 0).sum()) < n - 1 and got.avgdl == ref.avgdl
    for name in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf"):
        assert np.array_equal(np.asarray(getattr(got, name)), np.asarray(getattr(ref, name))), name
    assert np.array_equal(np.asarray(got.idf).view(np.uint32), ref.idf.view(np.uint32))
    with pytest.raises(ValueError):
        bm25_index_from_token_ids([1, 1], [0, 1, 2], [0, 0], 1)
    with pytest.raises(ValueError):
        bm25_index_from_token_ids([1, 2], [0, 1, 2], [0, 5], 2)


def test_http_facade_shapes_and_status_codes():
    from fastapi.testclient import TestClient
    from msretr.reranker import RerankNotFound
    from msretr.server import create_app

    class FakeReranker:
        def rerank(self, doc_ids, similarities, query=None, query_embedding=None):
            if doc_ids == ["404"]:
                raise RerankNotFound("No documents found for the provided doc_ids")
            if doc_ids == ["boom"]:
                raise RuntimeError("x")
            return {"document_scores": [], "top_windows": [], "total_documents": 0, "total_windows": 100}

    class FakeRetriever:
        reranker = FakeReranker()

        def search(self, query, top_k=1000, query_embedding=None, terms=None, query_id=None):
            return [{"query_id": query_id, "rank": 1, "url": "https://a.de", "score": 0.5, "title": "t",
                     "snippet": "s", "domain": "a", "doc_id": "7"}]

        def batch_search(self, queries):
            return [{"query_num": n, "rank": 1, "url": "u", "score": "0.500", "formatted_line": f"{n}\t1\tu\t0.500"}
                    for n, _ in queries]

    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False, encoding="utf-8") as f:
        f.write("1\tfood and drinks\n2\tcastle\n")
    c = TestClient(create_app(FakeRetriever(), llm=lambda q, w: "summary", queries_file=f.name))
    assert c.post("/rerank", json={"doc_ids": ["1"], "similarities": [1.0], "query": "q"}).status_code == 200
    assert c.post("/rerank", json={"doc_ids": ["404"], "similarities": [1.0], "query": "q"}).status_code == 401
    assert c.post("/rerank", json={"doc_ids": ["boom"], "similarities": [1.0], "query": "q"}).status_code == 500
    r = c.post("/api/search", json={"query": "Food", "query_id": "abc"})
    assert r.status_code == 200 and r.json()["llm_response"] == "summary"
    assert set(r.json()["documents"][0]) == {"query_id", "rank", "url", "score", "title", "snippet", "domain", "doc_id"}
    b = c.post("/api/batch_search").json()
    assert b["total_queries"] == 2 and b["results"][1]["formatted_line"] == "2\t1\tu\t0.500"
    assert c.get("/api/health").json()["status"] == "healthy"
    assert TestClient(create_app(FakeRetriever(), queries_file="/nonexistent")).post("/api/batch_search").status_code == 404
    # /api/batch_search_file (search_api.py:331-367): same run, lines written to a file, errors passed through
    out = f.name + ".results"
    c2 = TestClient(create_app(FakeRetriever(), queries_file=f.name, results_file=out))
    r = c2.post("/api/batch_search_file").json()
    assert r["total_queries"] == 2 and r["total_results"] == 2 and r["output_file"] == out
    assert r["format"] == "query_num<tab>rank<tab>url<tab>score per line"
    assert open(out, encoding="utf-8").read() == "1\t1\tu\t0.500\n2\t1\tu\t0.500\n"
    assert TestClient(create_app(FakeRetriever(), queries_file="/nonexistent")).post("/api/batch_search_file").status_code == 404
    assert "api/search" in c.get("/").text


def test_duckdb_loader_is_columnar_at_ten_million_postings(tmp_path):
    """CorpusIndex.from_duckdb at >= 1e7 postings (round-1 finding: per-posting Python loops and np.stack of
    every embedding cell could not stream the BASELINE shape).  The loader now pulls numeric columns only (the term -> id
    join and both sort orders happen in SQL), maps documents with one searchsorted, and writes the embeddings block by
    block straight into the snapshot's memory-mapped matrix; checked against the arrays the tables were generated from,
    then the snapshot is reloaded.  Through a sqlite3 adapter (duckdb is not installable here)."""
    import sqlite3
    import time
    from msretr.index import CorpusIndex
    rng = np.random.default_rng(5)
    N, V, per = 100_000, 50_000, 102
    db = str(tmp_path / "big.sqlite")
    con = sqlite3.connect(db)
    con.executescript("""
        PRAGMA journal_mode=OFF; PRAGMA synchronous=OFF;
        CREATE TABLE bm25_doc_stats (doc_id INTEGER PRIMARY KEY, doc_length INTEGER);
        CREATE TABLE bm25_term_freq (doc_id INTEGER, term TEXT, freq INTEGER, PRIMARY KEY (doc_id, term)) WITHOUT ROWID;
        CREATE TABLE bm25_term_stats (term TEXT PRIMARY KEY, doc_freq INTEGER, total_freq INTEGER, idf_score REAL);
        CREATE TABLE bm25_corpus_stats (stat_name TEXT PRIMARY KEY, stat_value REAL);
        CREATE TABLE chunks_optimized (chunk_id BIGINT PRIMARY KEY, doc_id BIGINT, chunk_text TEXT);
        CREATE TABLE embeddings (chunk_id BIGINT PRIMARY KEY, embedding BLOB);
        CREATE TABLE urlsDB (id BIGINT PRIMARY KEY, url TEXT UNIQUE, title TEXT, text TEXT);
    """)
    doc_ids = np.cumsum(rng.integers(1, 4, size=N)) + 10
    base, stride = rng.integers(0, V, size=N), rng.integers(1, 400, size=N) * 2 + 1
    terms = np.sort((base[:, None] + np.arange(per)[None, :] * stride[:, None]) % V, axis=1)
    keep = np.ones_like(terms, bool); keep[:, 1:] = terms[:, 1:] != terms[:, :-1]
    dd, tt = np.repeat(doc_ids, per)[keep.ravel()], terms.ravel()[keep.ravel()]
    ff = rng.integers(1, 5, size=len(dd))
    assert len(dd) >= 10_000_000
    names = np.array([f"t{v:05d}" for v in range(V)])
    con.executemany("INSERT INTO bm25_term_freq VALUES (?,?,?)", zip(dd.tolist(), names[tt].tolist(), ff.tolist()))
    dl = rng.integers(50, 500, size=N)
    con.executemany("INSERT INTO bm25_doc_stats VALUES (?,?)", zip(doc_ids.tolist(), dl.tolist()))
    df = np.bincount(tt, minlength=V)
    idf = np.log10((N - df + 0.5) / (df + 0.5)).astype(np.float32)
    con.executemany("INSERT INTO bm25_term_stats VALUES (?,?,?,?)",
                    [(names[v], int(df[v]), int(df[v]), None if v % 997 == 0 else float(idf[v])) for v in range(V) if df[v] > 0])
    con.executemany("INSERT INTO bm25_corpus_stats VALUES (?,?)", [("avg_doc_length", 275.5), ("total_docs", float(N))])
    C = 5000
    cd = np.sort(rng.choice(doc_ids, size=C))
    emb = rng.standard_normal((C, 768)).astype(np.float32)
    con.executemany("INSERT INTO chunks_optimized VALUES (?,?,?)", [(i, int(d), "") for i, d in enumerate(cd)])
    con.executemany("INSERT INTO embeddings VALUES (?,?)", [(i, emb[i].tobytes()) for i in range(C)])
    con.executemany("INSERT INTO urlsDB VALUES (?,?,?,?)", [(int(d), f"http://x/{int(d)}", "t", "x") for d in doc_ids[:2000]])
    con.commit(); con.close()

    class Cur:
        def __init__(self, cur):
            self.cur = cur

        def fetchall(self):
            return self.cur.fetchall()

        def fetchnumpy(self):
            rows = self.cur.fetchall()
            out = {}
            for i, d in enumerate(self.cur.description):
                col = [r[i] for r in rows]
                if d[0] == "embedding":
                    arr = np.empty(len(col), dtype=object)
                    arr[:] = [np.frombuffer(b, np.float32) for b in col]
                    out[d[0]] = arr
                else:
                    out[d[0]] = np.array(col)
            return out

    class Conn:
        def __init__(self, path):
            self.con = sqlite3.connect(path)

        def execute(self, sql, params=()):
            return Cur(self.con.execute(sql, params))

    snap = str(tmp_path / "snap")
    t0 = time.time()
    ix = CorpusIndex.from_duckdb(db, connect=Conn, snapshot_dir=snap, block_docs=20000)
    print(f"from_duckdb: {len(ix.post_doc)} postings in {time.time() - t0:.1f}s")
    present = np.nonzero(df > 0)[0]
    assert ix.n_terms == len(present) and list(ix.vocab) == names[present].tolist()
    order = np.lexsort((np.searchsorted(ix.doc_ids, dd), tt))
    assert np.array_equal(ix.post_doc, np.searchsorted(ix.doc_ids, dd)[order].astype(np.int32))
    assert np.array_equal(ix.post_tf, ff[order].astype(np.int32))
    assert np.array_equal(np.diff(ix.term_off), df[present])
    exp_idf = np.where(present % 997 == 0, 0.0, idf[present]).astype(np.float32)          # NULL -> 0.0 (:426)
    assert np.array_equal(ix.idf, exp_idf)
    assert np.array_equal(ix.doc_len, dl.astype(np.int32)) and ix.avgdl == float(np.float32(275.5))
    assert ix.n_chunks == C and np.array_equal(np.asarray(ix.emb), emb)                     # chunk ids ascend with (doc, chunk)
    assert ix.urls[0] == f"http://x/{int(doc_ids[0])}" and ix.urls[5000] is None
    back = CorpusIndex.load_dir(snap)
    assert np.array_equal(back.post_doc, ix.post_doc) and np.array_equal(np.asarray(back.emb), emb)
    assert back.url_group().tolist() == ix.url_group().tolist()


def test_streaming_kernels_keep_their_row_rings_in_place():
    """The streaming passes drive their row rings by hand (inline-asm loads + counted s_waitcnt).  The compiler must not spill
    inside that pipeline nor rename ring slots with moves of registers whose loads are in flight: tools/ring_check.py compiles
    msr_gemm_f32.hip to gfx950 assembly (no GPU needed) and checks spills, vmcnt(0) inside the pipeline and the load
    destinations of every streaming kernel."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ring_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok  ") == 12, r.stdout          # 10 instantiations of the 256-query kernel (2 with non-temporal row loads, 2 on the f16 image) + 2 of the 128-query kernel


# scores on the formatter's slow path (1e12 and above, infinities, NaNs of both signs) and around its threshold, in the order
# of tests/format_lines_check.cpp
HUGE_SCORES = [1e12, -1e12, 1e12 - 0.0005, 1e36, 1e308, -1e308, sys.float_info.max, -sys.float_info.max, float("inf"),
               -float("inf"), float("nan"), struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0], 999999999999.9994,
               4503599627370496.5, 9007199254740993.0]


def test_python_prints_a_nan_without_its_sign():
    """The decision msr_format_lines follows: format(x, ".3f") of a NaN is "nan" whatever its sign bit (C's printf prints
    "-nan"), an infinity keeps its sign, and the longest line is -DBL_MAX's 314 characters."""
    neg_nan = HUGE_SCORES[11]
    assert math.isnan(neg_nan) and math.copysign(1.0, neg_nan) == -1.0
    assert format(neg_nan, ".3f") == "nan" == format(float("nan"), ".3f")
    assert format(-float("inf"), ".3f") == "-inf" and format(float("inf"), ".3f") == "inf"
    assert len(format(1e36, ".3f")) == 41 and max(len(format(x, ".3f")) for x in HUGE_SCORES) == 314
    assert 1e12 - 0.0005 < 1e12 and format(1e12 - 0.0005, ".3f") == "1000000000000.000"       # the fast path's longest number


def test_line_formatter_on_huge_scores_under_the_host_sanitizers(tmp_path):
    """tests/format_lines_check.cpp with csrc/msr_format.cpp under the address and undefined-behaviour sanitizers (a program
    of its own: nothing is loaded into this process): every slow-path score as first and last result of the first and last
    query, into a buffer of exactly the bytes the sizing call asked for.  A score of 1e12 and above used to advance the
    output by what snprintf WOULD have written into its 40 bytes: 1e308 wrote 129 bytes past such a buffer, 1e36 left a
    NUL and a cut line.  The printed lines equal Python's."""
    from msretr.text import format_result_line
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "format_lines_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-pthread", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "format_lines_check.cpp"),
           os.path.join(ROOT, "modern-search-engines-project_amd", "csrc", "msr_format.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, timeout=60)
    out = r.stdout.decode("utf-8")
    assert r.returncode == 0, out[-3000:] + r.stderr.decode("utf-8", "replace")[-6000:]
    assert out.endswith("format lines ok\n") and "FAILED" not in out
    urls = ["https://a.de/x", "", "http://b.org/a/long/path?q=1"]
    url = lambda d: urls[d] if 0 <= d < 3 else ""
    qn, doc, n = ["7", "Q-otto", "42"], [[0, 1, 2], [2, -1, 0], [1, 3, 0]], [3, 2, 3]
    exp = []
    for x in HUGE_SCORES:
        exp.append("# %016x" % struct.unpack("<Q", struct.pack("<d", x))[0])
        score = [[x, 0.5, x], [0.5, 0.5, x], [x, 0.5, x]]
        exp += [format_result_line(qn[q], r + 1, url(doc[q][r]), score[q][r]) for q in range(3) for r in range(n[q])]
    exp.append("# all")
    NV = len(HUGE_SCORES)
    exp += [format_result_line("7", i + 1, url(i % 4 - 1), HUGE_SCORES[i % NV]) for i in range(3 * NV)]
    exp.append("format lines ok")
    got = out.split("\n")
    assert got[-1] == "" and len(got) - 1 == len(exp)
    for g, e in zip(got, exp):
        assert g == e
    assert format_result_line("7", 1, "", HUGE_SCORES[4]).endswith("\t" + format(1e308, ".3f")) and len(format(1e308, ".3f")) == 313


def test_native_line_formatter_equals_python_format():
    """msr_format_lines (host function of libmsretr: no GPU) writes byte for byte what the reference's f-string does
    (search_api.py:290 `f"{query_num}\\t{rank}\\t{url}\\t{score:.3f}"`), including the half-to-even rounding of the EXACT
    binary value at the third decimal, negative zero, documents without a URL and non-ASCII URLs."""
    import random
    from msretr.text import LineFormatter, format_result_line
    urls = [f"https://ex{i}.de/p?x={i}" if i % 7 else None for i in range(50)]
    urls[3] = "https://tübingen.de/ü"
    lf = LineFormatter(urls)
    rng = random.Random(1)
    vals = [0.0, -0.0, 0.0005, 0.0015, 0.0025, 0.5, 0.9995, 0.99949999999999994, 1.0, 0.1235, 0.1245, 2.675, 1e-9, 123456.7895,
            -0.0004, -1.2345, 0.3335, float(np.nextafter(0.0005, 1)), float(np.nextafter(0.0005, 0)), 5e-324, 1e11 + 0.0005,
            1e13, float("inf"), float("nan")]
    vals += HUGE_SCORES                                        # (all inside the first query, whose 100 results are all formatted)
    vals += [rng.random() for _ in range(20000)] + [round(rng.random(), 3) + 0.0005 for _ in range(20000)]
    Q = len(vals) // 100
    doc = np.array([rng.randrange(-1, 52) for _ in range(Q * 100)], np.int32).reshape(Q, 100)
    score = np.array(vals[:Q * 100]).reshape(Q, 100)
    n = np.array([rng.randrange(0, 101) for _ in range(Q)], np.int32)
    n[0] = 100
    qn = [str(i * 3) for i in range(Q)]
    got = lf.format(qn, doc, score, n)
    exp = "".join(format_result_line(qn[q], r + 1, (urls[doc[q, r]] or "") if 0 <= doc[q, r] < 50 else "", score[q, r]) + "\n"
                  for q in range(Q) for r in range(n[q])).encode()
    assert got == exp
    assert lf.format([], np.zeros((0, 0), np.int32), np.zeros((0, 0)), np.zeros(0, np.int32)) == b""


def test_emitted_rows_suffice_for_the_exact_top_k():
    """The invariant behind the streaming passes' finish (msr_batch_rescore_rows recomputes only the rows the
    pass emitted for a candidate document), checked on the CPU with the pass' own arithmetic restated in numpy: products of
    f16(e) and f16(q^) accumulated in f32, the measured margin 2 (dE (1 + dq) + dq) + 1e-4, the bucket's bound = (k-th largest
    TILE maximum) - margin.  For every document whose exact max-cosine reaches the exact k-th document score: its arg-max row
    -- every row tied with it -- is among the emitted rows, so the maximum over the emitted rows IS the document's score; for
    every other document the maximum over its emitted rows cannot lift it above the k-th."""
    rng = np.random.default_rng(5)
    n_docs, k = 14000, 100
    n = rng.integers(1, 9, size=n_docs)
    off = np.zeros(n_docs + 1, np.int64); off[1:] = np.cumsum(n)
    C = int(off[-1])
    chunk_doc = np.repeat(np.arange(n_docs), n)
    emb = rng.standard_normal((C, 768)).astype(np.float32)
    emb *= (rng.uniform(0.6, 1.8, size=(C, 1)) / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    emb[off[77] + 2] = emb[off[77]]                            # two identical rows inside one document
    inv = (1.0 / np.linalg.norm(emb.astype(np.float64), axis=1)).astype(np.float32)
    e16 = emb.astype(np.float16).astype(np.float32)
    dE = float(np.max(np.linalg.norm((emb - e16).astype(np.float64), axis=1) * inv))
    # row tiles of <= 256 rows cut at document boundaries (the k-th largest tile maximum is attained by k documents)
    tiles, start = [], 0
    for d in range(n_docs):
        if off[d + 1] - off[start] > 256:
            tiles.append((off[start], off[d])); start = d
    tiles.append((off[start], off[n_docs]))
    assert len(tiles) >= 2 * k
    for trial in range(6):
        q = rng.standard_normal(768).astype(np.float32)
        if trial == 0:
            q = emb[off[77]] * 3.0                             # the tied pair is the best document
        if trial == 1:
            q = emb[rng.integers(0, C)] + 0.5 * q / np.linalg.norm(q)
        qn = (q / np.linalg.norm(q.astype(np.float64))).astype(np.float32)
        q16 = qn.astype(np.float16).astype(np.float32)
        dq = float(np.linalg.norm((qn - q16).astype(np.float64)))
        margin = 2.0 * (dE * (1.0 + dq) + dq) + 1e-4
        approx = (e16 @ q16) * inv                             # the pass' scores (f32 accumulation of f16 products)
        exact = (emb @ qn) * inv                               # what the finish recomputes
        assert np.abs(approx - exact).max() <= 0.5 * margin    # the measured bound holds
        tmax = np.array([approx[a:b].max() for a, b in tiles])
        bound = np.sort(tmax)[-k] - margin                     # thr2
        emitted = approx >= bound
        doc_exact = np.maximum.reduceat(exact, off[:-1])
        doc_emit = np.full(n_docs, -np.inf, np.float32)
        np.maximum.at(doc_emit, chunk_doc[emitted], exact[emitted])
        sigma = np.sort(doc_exact)[-k]
        top = doc_exact >= sigma
        assert np.array_equal(doc_emit[top], doc_exact[top])                  # exact scores for everything that can be returned
        assert np.all(doc_emit[~top] <= doc_exact[~top]) and np.all(doc_emit[~top] < sigma)
        for d in np.nonzero(top)[0]:                           # ... and the FIRST arg-max row is among the emitted ones
            rows = np.arange(off[d], off[d + 1])
            first = rows[np.argmax(exact[rows])]
            assert emitted[first]
        assert emitted.sum() < 40 * k                          # (the filter filters: a few rows per candidate)


def test_bench_dump_writes_every_query_or_one_fixed_sample(tmp_path):
    """bench.py --dump-outputs: one float32 / float64 file per returned array, every value finite (the -inf scores of the
    slots past a query's count are written as 0); every query when the files fit in the limit, else the same seeded sample
    of queries in every array (a stage with fewer rows keeps the sampled queries it has)."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    idx = lambda q, k: torch.randint(-1, 1 << 30, (q, k), generator=g, dtype=torch.int32)
    cnt = lambda q, k: torch.randint(0, k + 1, (q,), generator=g, dtype=torch.int32)
    pad = lambda s, n: s.masked_fill(torch.arange(s.shape[1])[None, :] >= n[:, None], float("-inf"))   # as the engine pads
    nb, nd, nr = cnt(400, 10), cnt(400, 5), cnt(100, 10)
    out = {"bm25": (idx(400, 10), pad(torch.rand(400, 10, generator=g, dtype=torch.float64), nb), nb),
           "dense": (idx(400, 5), pad(torch.rand(400, 5, generator=g), nd), None, nd),
           "rerank": (idx(100, 10), pad(torch.rand(100, 10, generator=g, dtype=torch.float64), nr),
                      torch.rand(100, 10, generator=g, dtype=torch.float64), idx(100, 10), nr, cnt(100, 10))}
    arrays = bench.host_outputs(out)
    assert sorted(arrays) == sorted(["bm25_doc", "bm25_score", "bm25_n", "dense_doc", "dense_score", "dense_n", "rerank_doc",
                                     "rerank_score", "rerank_orig", "rerank_chunk", "rerank_n", "rerank_rows"])
    assert arrays["dense_score"].dtype == np.float32 and all(a.dtype == np.float64 for k, a in arrays.items() if k != "dense_score")
    assert np.array_equal(arrays["bm25_doc"], out["bm25"][0].numpy()) and np.array_equal(arrays["rerank_rows"], out["rerank"][5].numpy())
    assert all(np.isfinite(a).all() for a in arrays.values())
    for stage, n in (("bm25", nb), ("dense", nd), ("rerank", nr)):
        got, exp = arrays[f"{stage}_score"], out[stage][1].numpy()
        inside = np.arange(exp.shape[1])[None, :] < n.numpy()[:, None]
        assert np.array_equal(got[inside], exp[inside]) and np.all(got[~inside] == 0), stage

    assert bench.write_outputs(arrays, str(tmp_path / "all")) == 400
    assert np.array_equal(np.load(tmp_path / "all" / "query_index.npy"), np.arange(400))
    for name, a in arrays.items():
        got = np.load(tmp_path / "all" / f"{name}.npy")
        assert got.dtype == a.dtype and np.array_equal(got, a), name

    limit = 20000
    kept = [bench.write_outputs(arrays, str(tmp_path / d), limit=limit) for d in ("a", "b")]
    assert kept[0] == kept[1] and 1 <= kept[0] < 400
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= limit
    q = np.load(tmp_path / "a" / "query_index.npy")
    assert len(q) == kept[0] and np.all(np.diff(q) > 0) and np.array_equal(q, np.load(tmp_path / "b" / "query_index.npy"))
    q = q.astype(np.int64)
    for name, a in arrays.items():
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert np.array_equal(got, a[q[q < len(a)]]) and np.array_equal(got, np.load(tmp_path / "b" / f"{name}.npy")), name

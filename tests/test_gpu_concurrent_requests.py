"""Concurrent requests on ONE engine (msretr/serial.py): the facades take the engine's lock for a whole request, so threads that
come in together are served one after the other and each gets its own answer.

The fixture is the crawl and the 32 queries of options_cases.py behind one Retriever (forward index, vocabulary, URLs, bf16 off,
max_queries=64: a 300-query search_batch is two chunks and uses both pinned slots).  A concurrent answer must be BIT-EQUAL to
the same request issued alone on the same retriever beforehand (the same call shape, so the same kernels and the same bits), and
the answers issued alone agree with the composed CPU oracle (options_ref.py) under the comparison of test_gpu_options_oracle.py,
taken from that file: scores within its PARITY_BAR, everything else equal.

All threads live in this one process (one GPU client), at most 8 of them.  Every join has a limit: 20 x the time the thread's
own work took when it ran alone in the same test, at least 30 s (LIMIT_FACTOR, LIMIT_FLOOR).  A join that runs out is a hang:
the test fails at once and the remaining tests of this file are skipped (_HUNG).

The tests never run unlocked: what an absent lock looks like is shown on the CPU, over a stand-in (test_serial.py).  Here the
contract itself is pinned as well as its symptoms: a recorder around the bound methods of this DeviceEngine (Guard) notes thread
and enter / leave of every engine call and of every facade call; after the joins no two threads were inside the engine at
once, and between a request's first engine call and its last no other thread entered."""
import functools
import threading
import time
from dataclasses import replace

import numpy as np
import pytest
import torch

import options_ref as ref
from msretr.docset import DocSet
from msretr.fuzzy import Results
from msretr.retriever import Retriever
from msretr.text import Near
from options_cases import BATCHES, BIG_SITES, NAMED, N_FILL, TOPICS, call_kwargs, crawl, masks, vectors
from test_gpu_options_oracle import EXTRAS, _same        # the comparison of the oracle's own GPU test, its PARITY_BAR inside
from test_serial import LOCKED

pytestmark = pytest.mark.gpu
N_THREADS = 8                # a GPU command has 16 CPUs
ROUNDS = 3
LIMIT_FACTOR, LIMIT_FLOOR = 20.0, 30.0
_HUNG = []                   # set by a join that ran out: the remaining tests of the file are skipped


@pytest.fixture(autouse=True)
def _not_after_a_hang():
    if _HUNG:
        pytest.skip(f"an earlier test of this file hung: {_HUNG[0]}")


# ---------------------------------------------------------------------------------------------------- the recorder
class Guard:
    """Thread and enter / leave of every call of the wrapped bound methods, in one order.  It only records."""

    def __init__(self):
        self.meta, self.events = threading.Lock(), []

    def _log(self, kind, name):
        with self.meta:
            self.events.append((threading.get_ident(), kind, name))

    def wrap(self, obj, names, kind):
        for name in names:
            setattr(obj, name, self._wrapped(getattr(obj, name), kind, name))

    def _wrapped(self, fn, kind, name):
        @functools.wraps(fn)
        def run(*args, **kwargs):
            self._log(kind + "+", name)
            try:
                return fn(*args, **kwargs)
            finally:
                self._log(kind + "-", name)
        return run

    def threads(self):
        return {t for t, kind, _ in self.events if kind == "eng+"}


def violations(events):
    """events: (thread, "eng+" | "eng-" | "req+" | "req-", name) in the order they happened -> what breaks the contract:
    ("overlap", ...) an engine call entered while another thread was inside one; ("interleaved", ...) another thread's engine
    call between the first and the last engine call of one request (the outermost facade call of a thread)."""
    out, inside = [], {}
    for seq, (tid, kind, name) in enumerate(events):
        if kind == "eng+":
            others = [t for t, d in inside.items() if d > 0 and t != tid]
            if others:
                out.append(("overlap", seq, name, tid, others))
            inside[tid] = inside.get(tid, 0) + 1
        elif kind == "eng-":
            inside[tid] -= 1
    depth, start, spans = {}, {}, []
    for seq, (tid, kind, name) in enumerate(events):
        if kind == "req+":
            if depth.get(tid, 0) == 0:
                start[tid] = seq
            depth[tid] = depth.get(tid, 0) + 1
        elif kind == "req-":
            depth[tid] -= 1
            if depth[tid] == 0:
                spans.append((tid, start[tid], seq, name))
    eng_seq = np.asarray([seq for seq, (_, kind, _) in enumerate(events) if kind.startswith("eng")], np.int64)
    eng_tid = np.asarray([tid for tid, kind, _ in events if kind.startswith("eng")], np.int64)
    for tid, a, b, name in spans:
        mine = eng_seq[(eng_tid == tid) & (eng_seq > a) & (eng_seq < b)]
        if len(mine) and bool(((eng_tid != tid) & (eng_seq > mine[0]) & (eng_seq < mine[-1])).any()):
            out.append(("interleaved", name, tid, a, b))
    return out


def test_the_recorder_sees_an_overlap_and_an_interleaving():
    """The checker on written-out event lists (no thread, no GPU call): what tests 1 to 3 would report."""
    A, B = 1, 2
    clean = [(A, "req+", "search"), (A, "eng+", "x"), (A, "eng+", "nested"), (A, "eng-", "nested"), (A, "eng-", "x"), (B, "req+", "search"),
             (A, "eng+", "y"), (A, "eng-", "y"), (A, "req-", "search"), (B, "eng+", "x"), (B, "eng-", "x"), (B, "req-", "search")]
    assert violations(clean) == []
    overlap = [(A, "eng+", "x"), (B, "eng+", "y"), (B, "eng-", "y"), (A, "eng-", "x")]
    assert [v[0] for v in violations(overlap)] == ["overlap"]
    between = [(A, "req+", "search"), (A, "eng+", "x"), (A, "eng-", "x"), (B, "eng+", "rebind"), (B, "eng-", "rebind"), (A, "eng+", "y"),
               (A, "eng-", "y"), (A, "req-", "search")]
    assert [v[0] for v in violations(between)] == ["interleaved"]


# ---------------------------------------------------------------------------------------------------- the fixture
class Site:
    def __init__(self):
        from fastapi.testclient import TestClient
        from msretr.engine import DeviceEngine
        from msretr.server import create_app
        self.c = crawl()
        self.r = Retriever(indexer=self.c.ix, max_queries=64, max_k=1000)
        self.within = [[None if m is None else DocSet.from_mask(self.c.ix, m) for m in masks(self.c, b)] for b in BATCHES]
        self.guard = Guard()
        self.guard.wrap(self.r.engine, [k for k, v in vars(DeviceEngine).items() if not k.startswith("_") and callable(v)], "eng")
        for obj, name in ((self.r, "Retriever"), (self.r.bm25, "BM25"), (self.r.reranker, "Reranker")):
            self.guard.wrap(obj, sorted(LOCKED[name] - {"final_list_chunks"}), "req")     # (a generator's work is not inside its call)
        self.app = create_app(self.r)
        self.client = lambda: TestClient(self.app)
        self.oracle = {}

    def want(self, b, q, mode, collapse):
        """The oracle's answer to query q of batch b, with the collapse on (the table's setting) or off; once per module."""
        key = (b, q, mode, collapse)
        if key not in self.oracle:
            plan = ref.plans(self.c, BATCHES[b])[q]
            self.oracle[key] = ref.evaluate(self.c, plan if collapse else replace(plan, collapse=None), mode, True)
        return self.oracle[key]

    def clean(self):
        bad = violations(self.guard.events)
        assert not bad, bad[:5]


@pytest.fixture(scope="module")
def site():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    s = Site()
    yield s
    s.r.engine.close()


def run_workers(targets, alone_seconds, what):
    """One daemon thread per target, started together; thread i is joined with max(LIMIT_FLOOR, LIMIT_FACTOR x alone_seconds[i])
    seconds, alone_seconds[i] being what its work took alone.  A join that runs out is a hang."""
    errors, start = [], threading.Barrier(len(targets))
    assert len(targets) <= N_THREADS

    def guarded(fn):
        def go():
            try:
                start.wait(LIMIT_FLOOR)
                fn()
            except BaseException as e:                      # noqa: BLE001  (raised again by the main thread)
                errors.append(e)
        return go
    threads = [threading.Thread(target=guarded(t), daemon=True, name=f"{what}-{i}") for i, t in enumerate(targets)]
    for t in threads:
        t.start()
    return threads, errors, [max(LIMIT_FLOOR, LIMIT_FACTOR * s) for s in alone_seconds]


def join_workers(threads, errors, limits, what):
    for t, limit in zip(threads, limits):
        t.join(limit)
        if t.is_alive():
            _HUNG.append(f"{what}: {t.name} still alive after {limit:.0f} s")
            pytest.fail(_HUNG[-1])
    if errors:
        raise errors[0]


# ---------------------------------------------------------------------------------------------------- 1. many single searches
def _phrase(p):
    if isinstance(p, Near):
        return {"phrase": p.terms if isinstance(p.terms, str) else " ".join(p.terms), "slop": p.slop, "ordered": p.ordered}
    return p if isinstance(p, str) else " ".join(p)


def http_body(c, b, q, mode, collapse, query_id):
    """Query q of batch b as a POST /api/search body: the batch's switches (the collapse as given), its lists and its sites."""
    batch = BATCHES[b]
    body = {"query": batch.queries[q], "query_id": query_id, "query_embedding": vectors(c, batch)[q].tolist(), "mode": mode}
    body.update(batch.switches)
    body["collapse_duplicates"] = collapse
    if batch.term_lists is not None:
        body["terms"] = batch.term_lists[q]
    if batch.sites[q] is not None:
        body["sites"] = batch.sites[q]
    for k, v in batch.lists.items():
        if v[q] is not None:
            body[k] = [_phrase(p) for p in v[q]] if k in ("must_phrases", "must_not_phrases") else list(v[q])
    return body


class Answer(list):
    """A /api/search response as the oracle's comparison reads a result: the rows, and the extras as attributes."""

    def __init__(self, out):
        super().__init__(out["documents"])
        for name in EXTRAS:
            setattr(self, name, out.get(name, getattr(Results, name)))      # (a feature that is off: the value a Results has then)


def post(client, body):
    resp = client.post("/api/search", json=body)
    assert resp.status_code == 200, (body["query_id"], resp.status_code, resp.text)
    return resp.json()


def thread_cases(k):
    """The 4 of the 32 cases of thread k: query k of every batch; hybrid against lexical and the collapse on against off
    alternate between adjacent threads, and every thread has both of each."""
    return [(b, k, "hybrid" if (k + b) % 2 == 0 else "lexical", (k + b // 2) % 2 == 0) for b in range(len(BATCHES))]


def test_many_single_searches_at_once(site):
    c = site.c
    assert sorted((b, q) for k in range(N_THREADS) for b, q, _, _ in thread_cases(k)) == [(b, q) for b in range(4) for q in range(8)]
    bodies = [[http_body(c, b, q, mode, coll, f"t{k}-b{b}") for b, q, mode, coll in thread_cases(k)] for k in range(N_THREADS)]
    one = site.client()
    alone, seconds = [], []
    for k in range(N_THREADS):                               # every request alone, beforehand
        t0 = time.monotonic()
        alone.append([post(one, body) for body in bodies[k]])
        seconds.append(ROUNDS * (time.monotonic() - t0))
    for k in range(N_THREADS):                               # ... agrees with the oracle
        for (b, q, mode, coll), out in zip(thread_cases(k), alone[k]):
            assert ("collapsed" in out) == coll and all(row["query_id"] == f"t{k}-b{b}" for row in out["documents"])
            _same(Answer(out), site.want(b, q, mode, coll), ("alone", k, b, mode, coll))
    docs = lambda out: [row["doc_id"] for row in out["documents"]]
    print("rows per case", [[len(docs(out)) for out in alone[k]] for k in range(N_THREADS)], "alone, seconds", seconds)
    for k in range(N_THREADS - 1):                           # adjacent threads: other documents, other lengths, the other settings
        for j in range(4):
            assert docs(alone[k][j]) != docs(alone[k + 1][j]), (k, j)
            assert thread_cases(k)[j][2] != thread_cases(k + 1)[j][2] and thread_cases(k)[j][3] != thread_cases(k + 1)[j][3]
        assert any(len(docs(alone[k][j])) != len(docs(alone[k + 1][j])) for j in range(4)), k

    def worker(k):
        def go():
            client = site.client()
            for rnd in range(ROUNDS):
                for j, body in enumerate(bodies[k]):
                    assert post(client, body) == alone[k][j], ("thread", k, "round", rnd, "case", j)
        return go
    state = run_workers([worker(k) for k in range(N_THREADS)], seconds, "searches")
    join_workers(*state, "searches")
    site.clean()
    assert len(site.guard.threads()) >= 2


# ---------------------------------------------------------------------------------------------------- 2. mixed entry points
def snapshot(res):
    """A result with its extras (a fuzzy.Results' attributes), comparable bit for bit."""
    if isinstance(res, list) and res and isinstance(res[0], list):
        return [snapshot(x) for x in res]
    return (list(res), {name: getattr(res, name, None) for name in EXTRAS})


def test_mixed_entry_points_at_once(site):
    c, r = site.c, site.r
    A, B, C, D = range(4)
    tiled = lambda b, n: [q % 8 for q in range(n)]

    def batch_call(b, n, mode):
        """search_batch of n queries: the batch's eight, repeated."""
        batch, qs = BATCHES[b], tiled(b, n)
        rep = lambda xs: None if xs is None else [xs[q] for q in qs]
        kw = call_kwargs(c, batch, within=rep(site.within[b]))
        kw.update(query_embeddings=kw["query_embeddings"][qs], term_lists=rep(kw["term_lists"]))
        kw.update({k: rep(v) for k, v in batch.lists.items()})
        return lambda: r.search_batch(rep(batch.queries), mode=mode, **kw)
    sizes = [(D, 3, "lexical"), (A, 65, "hybrid"), (C, 300, "lexical")]
    calls = [batch_call(*s) for s in sizes]
    assert 300 > max(256, r.engine.max_queries) >= 65        # 300 queries: two chunks, both pinned slots; 65: more than max_queries
    single = lambda b, q, mode: lambda: r.search(BATCHES[b].queries[q], mode=mode, **call_kwargs(c, BATCHES[b], q, within=site.within[b][q]))
    source = int(np.asarray(c.ix.doc_ids)[c.pages["mensa"][0]])
    lex = r.bm25.search_terms(["mensa", "essen"], top_k=50)
    rerank_kw = dict(doc_ids=[str(d) for d, _ in lex], similarities=[s for _, s in lex], query_embedding=vectors(c, BATCHES[C])[0])
    sw = BATCHES[A].switches
    bm25_kw = {k: sw[k] for k in ("operators", "proximity", "fuzzy", "wildcards", "max_expansions")}
    bm25_kw.update({k: v[2] for k, v in BATCHES[A].lists.items()})
    work = {"facets by host": single(A, 1, "hybrid"),
            "facets by domain": single(B, 1, "lexical"),       # (the one facet table rebinds between these two)
            "collapse and snippets": single(C, 0, "hybrid"),
            "search_batch of 3, 65 and 300": lambda: [call() for call in calls],
            "similar": lambda: r.similar([source], top_k=10),
            "rerank": lambda: r.reranker.rerank(**rerank_kw),
            "bm25.search": lambda: r.bm25.search(BATCHES[A].queries[2], top_k=sw["top_k"], within=site.within[A][2], **bm25_kw),
            "quick_search": lambda: r.quick_search(query_embedding=vectors(c, BATCHES[B])[1], top_k=10)}
    assert len(work) == N_THREADS
    view = {"similar": list, "rerank": lambda x: x, "quick_search": list}
    alone, seconds = {}, []
    for name, call in work.items():
        t0 = time.monotonic()
        alone[name] = view.get(name, snapshot)(call())
        seconds.append(ROUNDS * (time.monotonic() - t0))
    # alone: the oracle where it has an answer, and the plain properties of the rest
    _same(work["facets by host"](), site.want(A, 1, "hybrid", True), "facets by host")
    _same(work["facets by domain"](), site.want(B, 1, "lexical", True), "facets by domain")
    _same(work["collapse and snippets"](), site.want(C, 0, "hybrid", True), "collapse and snippets")
    assert alone["facets by host"][1]["facets"] != alone["facets by domain"][1]["facets"]
    assert alone["collapse and snippets"][1]["collapsed"] > 0 and "highlights" in alone["collapse and snippets"][0][0]
    for (b, n, mode), got in zip(sizes, work["search_batch of 3, 65 and 300"]()):
        assert len(got) == n
        for i in range(n):
            if i < 8:
                _same(got[i], site.want(b, i, mode, True), ("search_batch", n, i))
            else:
                assert snapshot(got[i]) == snapshot(got[i % 8]), (n, i)
    rows, corrections, expansions = ref.bm25_search(c, BATCHES[A], 2)
    got = work["bm25.search"]()
    assert [(row["doc_id"], row["score"]) for row in got] == rows and len(rows) > 0
    assert got.corrections == corrections and got.expansions == expansions
    assert len(alone["similar"]) == 10 and all(row["source_doc_id"] == source for row in alone["similar"])
    assert len(alone["rerank"]["document_scores"]) > 0 and len(alone["quick_search"]) == 10
    print("alone, seconds", dict(zip(work, seconds)))

    def worker(name):
        def go():
            for rnd in range(ROUNDS):
                assert view.get(name, snapshot)(work[name]()) == alone[name], (name, "round", rnd)
        return go
    state = run_workers([worker(name) for name in work], seconds, "mixed")
    join_workers(*state, "mixed")
    site.clean()


# ---------------------------------------------------------------------------------------------------- 3. update_index under load
def grown_index(c):
    """The fixture's index plus one page per topic (index_build.bm25_add_token_ids + chunk_index.attach_chunks): each holds its
    topic word three times, lies on a host inside BIG_SITES and has an embedding row next to a page the query vectors lean
    towards -- and with five more documents every idf and the average length change, so every score does."""
    from msretr.chunk_index import ChunkTable, attach_chunks
    from msretr.index_build import bm25_add_token_ids
    ix, rng = c.ix, np.random.default_rng(5)
    ids = np.asarray(ix.doc_ids, np.int64)
    new_ids = int(ids.max()) + 10 + np.arange(len(TOPICS), dtype=np.int64)
    streams = [np.asarray([ix.vocab[w]] * 3 + [ix.vocab["tübingen"]] + (len(NAMED) + rng.choice(N_FILL, 50, replace=False)).tolist(),
                          np.int32) for w in TOPICS]
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    meta = {int(d): (f"https://example.org/new{int(d)}", "neu " + w, " ".join(c.names[int(t)] for t in s))
            for d, w, s in zip(new_ids, TOPICS, streams)}
    grown = bm25_add_token_ids(ix, new_ids, off, np.concatenate(streams), ix.n_terms, vocab=ix.vocab, docs_meta=meta)
    doc_off = np.asarray(ix.doc_off, np.int64)
    e = np.stack([ix.emb[doc_off[c.pages[w][11]]] for w in TOPICS]) + 0.02 * rng.standard_normal((len(TOPICS), 768)).astype(np.float32)
    e = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    table = ChunkTable(chunk_ids=len(ix.emb) + np.arange(len(TOPICS), dtype=np.int64), doc_ids=new_ids, seqs=[[1]] * len(TOPICS),
                       emb=torch.as_tensor(e))
    return attach_chunks(grown, table)


def test_update_index_under_load(site):
    c, r = site.c, site.r
    original, grown = c.ix, grown_index(c)
    assert grown.n_docs == original.n_docs + len(TOPICS) and r.index is original
    # (batch, query, mode) of the /api/search requests of each searcher; those with sites go through the server's site cache
    lists = [[(0, 0, "hybrid"), (1, 1, "lexical"), (2, 0, "hybrid"), "similar"],
             [(0, 4, "lexical"), (1, 2, "hybrid"), (2, 3, "lexical"), (3, 0, "hybrid")],
             [(0, 5, "hybrid"), (1, 4, "lexical"), (2, 5, "hybrid"), (3, 2, "lexical")],
             [(0, 1, "lexical"), (1, 0, "hybrid"), (2, 7, "lexical"), (3, 6, "hybrid")]]
    source = int(np.asarray(original.doc_ids)[c.pages["mensa"][0]])
    assert sum(req != "similar" and BATCHES[req[0]].sites[req[1]] is not None for reqs in lists for req in reqs) >= 6

    def send(client, s, j):
        req = lists[s][j]
        if req == "similar":
            resp = client.post("/api/similar", json={"doc_id": source, "top_k": 10, "sites": BIG_SITES})
        else:
            resp = client.post("/api/search", json=http_body(c, req[0], req[1], req[2], True, f"s{s}-{j}"))
        assert resp.status_code == 200, (s, j, resp.status_code, resp.text)      # never a 500
        return resp.json()
    one = site.client()

    def alone():
        out, seconds = [], []
        for s in range(len(lists)):
            t0 = time.monotonic()
            out.append([send(one, s, j) for j in range(len(lists[s]))])
            seconds.append(time.monotonic() - t0)
        return out, seconds
    first, seconds = alone()
    for s, reqs in enumerate(lists):                          # the answers on the original index agree with the oracle
        for j, req in enumerate(reqs):
            if req != "similar":
                _same(Answer(first[s][j]), site.want(req[0], req[1], req[2], True), ("original", s, j))
    r.update_index(grown)
    second, _ = alone()
    r.update_index(original)
    assert alone()[0] == first
    changed = [[first[s][j] != second[s][j] for j in range(len(lists[s]))] for s in range(len(lists))]
    assert all(any(row) for row in changed), changed         # the added pages change at least one answer of every searcher
    new_docs = {str(int(d)) for d in np.asarray(grown.doc_ids)[original.n_docs:]}
    assert any(row["doc_id"] in new_docs for out in sum(second, []) for row in out["documents"])     # ... and are served

    MAX_ROUNDS = 40
    progress, rounds, stop = threading.Condition(), [0] * len(lists), threading.Event()
    seen = [{"original": 0, "grown": 0} for _ in lists]

    def searcher(s):
        def go():
            client = site.client()
            try:
                while not stop.is_set() and rounds[s] < MAX_ROUNDS:
                    for j in range(len(lists[s])):
                        out = send(client, s, j)
                        which = "original" if out == first[s][j] else "grown" if out == second[s][j] else None
                        assert which is not None, ("searcher", s, "request", j, "round", rounds[s], "neither index's answer")
                        if changed[s][j]:
                            seen[s][which] += 1
                    with progress:
                        rounds[s] += 1
                        progress.notify_all()
            except BaseException as e:
                errors.append(e)                             # (seen by the main thread's wait at once)
                with progress:
                    progress.notify_all()
        return go
    limits = [max(LIMIT_FLOOR, LIMIT_FACTOR * MAX_ROUNDS * t) for t in seconds]

    def wait_for_rounds(n, what):
        """Until every searcher has finished n more rounds (or stopped at MAX_ROUNDS); running out of time is a hang."""
        with progress:
            target = [min(MAX_ROUNDS, x + n) for x in rounds]
            if not progress.wait_for(lambda: all(x >= t for x, t in zip(rounds, target)) or bool(errors), max(limits)):
                _HUNG.append(f"update: searchers made no progress {what}: rounds {rounds}")
                pytest.fail(_HUNG[-1])
    threads, errors, _ = run_workers([searcher(s) for s in range(len(lists))], seconds, "update")
    try:
        wait_for_rounds(1, "before the update")
        r.update_index(grown)
        wait_for_rounds(2, "on the grown index")             # (a round that began before the update, then a whole one after it)
        r.update_index(original)
        wait_for_rounds(1, "after the second update")
    finally:
        stop.set()
    join_workers(threads, errors, limits, "update")
    print("rounds", rounds, "answers by index", seen)
    assert all(n["original"] > 0 and n["grown"] > 0 for n in seen), seen
    assert r.index is original and alone()[0] == first
    site.clean()


# ---------------------------------------------------------------------------------------------------- the chunk generator
def test_a_search_waits_for_a_chunk_generator_to_finish(site):
    """final_list_chunks holds the lock from its first chunk to exhaustion: 150 queries in chunks of 64 are three chunks, and
    when the first one is handed out the second is enqueued and the third -- pinned slot 0 again, the slot of every single
    search -- is still to come.  A search of another thread that arrives now starts its engine work after the generator's
    last; the chunks equal final_lists' rows of the same call alone, the search its answer alone."""
    c, r = site.c, site.r
    b, n = 2, 150
    batch = BATCHES[b]
    ids = [c.ix.term_ids(batch.term_lists[q % 8]) for q in range(n)]
    qv = vectors(c, batch)[[q % 8 for q in range(n)]]
    t0 = time.monotonic()
    doc, score, row, cnt = r.final_lists(ids, qv, top_k=60, chunk=64)
    search = lambda: r.search(batch.queries[0], mode="hybrid", **call_kwargs(c, batch, 0, within=None))
    alone = snapshot(search())
    seconds = time.monotonic() - t0
    started, got, me = threading.Event(), [], threading.get_ident()
    seq0 = len(site.guard.events)

    def other():
        started.set()
        got.append((threading.get_ident(), snapshot(search())))
    gen = r.final_list_chunks(ids, qv, top_k=60, chunk=64)
    parts = [next(gen)]
    threads, errors, limits = run_workers([other], [seconds], "generator")
    assert started.wait(LIMIT_FLOOR)
    parts += list(gen)
    join_workers(threads, errors, limits, "generator")
    assert [p[0] for p in parts] == [0, 64, 128]
    for a, d, s, w, m in parts:
        k = len(m)
        assert np.array_equal(m, cnt[a:a + k])
        for i in range(k):
            j = int(m[i])
            assert np.array_equal(d[i, :j], doc[a + i, :j]) and np.array_equal(s[i, :j], score[a + i, :j]) and \
                np.array_equal(w[i, :j], row[a + i, :j]), (a, i)
    (tid, answer), = got
    assert answer == alone and len(alone[0]) > 0 and tid != me
    events = site.guard.events[seq0:]
    mine = [i for i, (t, kind, _) in enumerate(events) if t == me and kind.startswith("eng")]
    theirs = [i for i, (t, kind, _) in enumerate(events) if t == tid and kind.startswith("eng")]
    assert mine and theirs and min(theirs) > max(mine), (max(mine), min(theirs))
    site.clean()


# ---------------------------------------------------------------------------------------------------- 4. the engine entry guard
def test_engine_entry_guard_over_the_whole_file(site):
    """Everything the recorder saw in tests 1 to 3, once more in one piece: requests of many threads, engine calls of every
    kind, and no two threads inside the engine at once nor inside one request's span."""
    events = site.guard.events
    names = {name for _, kind, name in events if kind == "eng+"}
    assert {"bm25_topk", "dense_topk", "rerank_gather", "rerank_fuse", "diversify", "collapse_duplicates", "bind_facet",
            "facet_counts", "best_windows", "rebind", "dense_topk_grouped", "rerank", "union_candidates"} <= names, names
    assert {name for _, kind, name in events if kind == "req+"} >= {"search", "search_batch", "similar", "rerank", "quick_search",
                                                                    "update_index"}
    assert len(site.guard.threads()) >= 2 and sum(kind == "eng+" for _, kind, _ in events) > 1000
    assert all(sum(1 if kind == k + "+" else -1 for _, kind, _ in events if kind[:3] == k) == 0 for k in ("eng", "req"))
    site.clean()

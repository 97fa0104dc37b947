"""The near-duplicate collapse on the GPU (msr_doc_signatures, msr_bind_signatures, msr_collapse_duplicates, DeviceEngine and
Retriever(collapse_duplicates=True); DESIGN K18): everything exact against the oracle of dedup_ref.py -- the signatures of
hand-made streams at every shingle width, the collapse of hand-made lists, every refusal, and the search path end to end on a
small crawl with planted copies under other URLs and hosts."""
import ctypes as C

import numpy as np
import pytest
import torch

import dedup_ref as ref
from msretr import _abi, fuzzy
from msretr.chunk_index import ChunkTable, attach_chunks
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import bm25_add_token_ids
from msretr.retriever import Retriever

pytestmark = pytest.mark.gpu
FILL = -1515870811                                           # 0xA5A5A5A5 as int32
INVALID, NOT_BOUND = -1, -2
N_TERMS = 1000


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- signatures -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    streams = ref.forward_index(N_TERMS)
    ix, off, tok = ref.index_of(streams, N_TERMS)
    eng = DeviceEngine(ix, max_queries=4, max_k=16, rerank_max_docs=0)
    want = {}                                                # the reference, once per width
    yield eng, streams, off, tok, lambda w: want.setdefault(w, ref.signatures_fast(off, tok, w))
    eng.close()


@pytest.mark.parametrize("w", range(1, ref.MAX_SHINGLE + 1))
def test_signatures_every_width(fwd, w):
    eng, streams, off, tok, want = fwd
    N = len(streams)
    assert {len(s) for s in streams} >= set(ref.stream_lengths(w)) | {ref.LONGER} and int(tok.max()) == N_TERMS - 1
    assert len(streams[0]) == 0 and len(streams[-1]) == ref.LONG          # the buffer's first and last documents
    out = torch.full((N + 1, 64), FILL, dtype=torch.int32, device=eng.device)
    eng.doc_signatures(w, out=out)
    got = _u32(out)
    assert (got[N] == np.uint32(FILL & 0xFFFFFFFF)).all()    # nothing behind the rows
    bad = np.nonzero((got[:N] != want(w)).any(axis=1))[0]
    assert len(bad) == 0, (w, [(int(d), len(streams[d])) for d in bad[:5]])
    assert (got[0] == ref.EMPTY).all()
    short = next(d for d in range(N) if 1 <= len(streams[d]) <= 400)
    assert (got[short] == ref.signature(streams[short], w)).all()          # ... and one row against the plain loops
    again = eng.doc_signatures(w)
    assert again.shape == (N, 64) and torch.equal(again, out[:N])          # two calls, equal bytes


def test_signature_subranges_leave_the_other_rows(fwd):
    eng, streams, off, tok, want = fwd
    N, w = len(streams), 4
    for d0, d1 in ((0, 1), (3, 4), (1, 9), (5, 22), (N - 1, N), (N - 9, N), (2, N - 3), (7, 7)):
        out = torch.full((d1 - d0 + 2, 64), FILL, dtype=torch.int32, device=eng.device)
        rc = eng.lib.msr_doc_signatures(eng.handle, d0, d1, w, _P(out[1:]), eng._stream())
        assert rc == 0, eng.lib.msr_last_error(eng.handle)
        got = _u32(out)
        assert (got[1:1 + d1 - d0] == want(w)[d0:d1]).all(), (d0, d1)
        assert (got[0] == np.uint32(FILL & 0xFFFFFFFF)).all() and (got[1 + d1 - d0] == np.uint32(FILL & 0xFFFFFFFF)).all(), (d0, d1)


def test_signature_refusals(fwd):
    eng, streams, *_ = fwd
    N = len(streams)
    out = torch.full((N, 64), FILL, dtype=torch.int32, device=eng.device)
    call = lambda d0, d1, w, o=out: eng.lib.msr_doc_signatures(eng.handle, d0, d1, w, _P(o), eng._stream())
    for args in ((-1, 2, 4), (3, 2, 4), (0, N + 1, 4), (0, N, 0), (0, N, 9), (0, N, -1)):
        assert call(*args) == INVALID, args
    assert call(0, N, 4, None) == INVALID
    assert call(5, 5, 4, None) == 0 and call(N, N, 4, None) == 0           # an empty range needs no output
    torch.cuda.synchronize(eng.device)
    assert (out == FILL).all()
    with pytest.raises(_abi.MsrError):
        eng.doc_signatures(12)
    # without a forward index: NOT_BOUND
    z = eng.index
    bare = CorpusIndex(**{k: getattr(z, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                      "total_docs")})
    e2 = DeviceEngine(bare, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        assert not e2.has_tokens
        assert e2.lib.msr_doc_signatures(e2.handle, 0, 1, 4, _P(out), e2._stream()) == NOT_BOUND
        torch.cuda.synchronize(eng.device)
        assert (out == FILL).all()
    finally:
        e2.close()


# ---- collapse -------------------------------------------------------------------------------------------------------------------
M = 300
NS = [0, 1, 2, 63, 64, 65, 129, 300, 1000, -5]               # fused_n per query; above max_cand and below 0 are clamped


class Lists:
    """An engine over 40 pages with 5 near-copies each (1 .. 25 of 60 tokens replaced: match counts from 64 down to a few),
    some pages without tokens; the signature table from the oracle; and fused lists of every length of NS."""

    def __init__(self):
        streams, self.group = ref.near_copies(40, 5, length=60, edits=30, n_terms=N_TERMS, seed=9)
        for d in (7, 8, 100):
            streams[d] = np.zeros(0, np.int32)               # EMPTY signatures (two of them in one group)
        self.ix, off, tok = ref.index_of(streams, N_TERMS)
        self.N = len(streams)
        self.sig = ref.signatures_fast(off, tok, 4)
        self.eng = DeviceEngine(self.ix, max_queries=4, max_k=16, rerank_max_docs=0)
        self.eng.bind_signatures(torch.from_numpy(self.sig.view(np.int32)).to(self.eng.device))
        rng = np.random.default_rng(10)
        Q = len(NS)
        self.doc = rng.integers(0, self.N, (Q, M)).astype(np.int32)
        self.doc[3, :63] = np.arange(63) * 6 % self.N        # group leaders and copies apart
        self.doc[6, 10:20] = [-1, self.N, self.N + 5, -7, 2 ** 31 - 1, 7, 8, 100, 7, -1]      # outside the table; EMPTY ones
        self.doc[7, :] = np.arange(M) % 6                    # one group only: with min_matches 1 all but the first drop
        self.doc[5, :65] = np.arange(65) * 6                 # base pages only: nothing drops
        self.score = -np.sort(-rng.random((Q, M)), axis=1)
        self.orig = rng.random((Q, M))
        self.chunk = rng.integers(0, 10 ** 6, (Q, M)).astype(np.int32)
        self.n = np.asarray(NS, np.int32)
        self.domain = np.where(rng.random(self.N + 3) < 0.2, -1, rng.integers(0, 9, self.N + 3)).astype(np.int32)
        self.domain[:6] = [0, -1, 1, 2, -1, 3]               # in query 7 two of the six pages are rejected

    def run(self, mm, doc=None, n=None, fill=False):
        """One msr_collapse_duplicates call into buffers with one query row more than the call writes -> host arrays
        (doc, score, orig, chunk, n, drop_doc, drop_leader, drop_matches, drop_n), and the return code."""
        dev, eng = self.eng.device, self.eng
        doc = self.doc if doc is None else doc
        n = self.n if n is None else n
        Q = len(n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        i32 = lambda *s: torch.full(s, FILL, dtype=torch.int32, device=dev)
        f64 = lambda *s: torch.full(s, -7.5, dtype=torch.float64, device=dev)
        outs = [i32(Q + 1, M), f64(Q + 1, M), f64(Q + 1, M), i32(Q + 1, M), i32(Q + 1), i32(Q + 1, M), i32(Q + 1, M), i32(Q + 1, M),
                i32(Q + 1)]
        need = eng.lib.msr_collapse_scratch_bytes(Q, M)
        scratch = torch.full((need // 8 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)      # (no memset is needed)
        ins = [up(doc[:Q]), up(self.score[:Q]), up(self.orig[:Q]), up(self.chunk[:Q]), up(n)]
        rc = eng.lib.msr_collapse_duplicates(eng.handle, Q, *map(_P, ins), M, mm, *map(_P, outs), _P(scratch), need, eng._stream())
        torch.cuda.synchronize(dev)
        return [o.cpu().numpy() for o in outs], rc

    def want(self, mm, domain=None, doc=None, n=None):
        doc = self.doc if doc is None else doc
        n = self.n if n is None else n
        Q = len(n)
        return ref.collapse_lists(doc[:Q], self.score[:Q], self.orig[:Q], self.chunk[:Q], n, self.sig, mm, domain)


@pytest.fixture(scope="module")
def lists():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    c = Lists()
    yield c
    c.eng.close()


def _same(got, want, Q, what):
    names = ("doc", "score", "orig", "chunk", "n", "drop_doc", "drop_leader", "drop_matches", "drop_n")
    for g, w, name in zip(got, want, names):
        assert (g[:Q] == w).all(), (what, name, np.argwhere(g[:Q] != w)[:4].tolist())
        tail = g[Q]                                          # the row behind the call's queries keeps the fill
        assert (tail == (-7.5 if g.dtype == np.float64 else FILL)).all(), (what, name)


@pytest.mark.parametrize("mm", [1, 58, 64])
def test_collapse_against_the_oracle(lists, mm):
    Q = len(NS)
    got, rc = lists.run(mm)
    assert rc == 0, lists.eng.lib.msr_last_error(lists.eng.handle)
    want = lists.want(mm)
    _same(got, want, Q, mm)
    kept, dropped = want[4], want[8]
    assert (kept + dropped == np.clip(lists.n, 0, M)).all()
    assert kept[0] == 0 and kept[1] == 1 and dropped[9] == 0 and kept[8] + dropped[8] == M        # n = 0, 1, clamped from both sides
    assert dropped[5] == 0                                   # a list without duplicates
    if mm == 1:
        assert kept[7] <= 3 and dropped[7] >= M - 3          # the all-duplicate list: one group, EMPTY rows apart
    if mm == 64:
        assert dropped[7] == M - 6                           # the six pages differ; every repeat equals its first occurrence
    assert 0 < dropped[7] and 0 < dropped[6] < lists.n[6]
    # padding past out_n / out_drop_n (the oracle pads the same way; stated once more directly)
    q = 6
    assert (got[0][q, kept[q]:] == -1).all() and np.isneginf(got[1][q, kept[q]:]).all() and (got[2][q, kept[q]:] == 0).all()
    assert (got[3][q, kept[q]:] == -1).all() and (got[5][q, dropped[q]:] == -1).all() and (got[6][q, dropped[q]:] == -1).all()
    assert (got[7][q, dropped[q]:] == 0).all()
    # rows outside the table and EMPTY rows are kept
    for d in (-1, lists.N, lists.N + 5, -7, 2 ** 31 - 1, 100):
        assert d in got[0][q, :kept[q]] and d not in got[5][q, :dropped[q]]
    again, _ = lists.run(mm)
    assert all((a == b).all() for a, b in zip(again, got))   # repeated calls, equal bytes


def test_chain_and_two_leaders(lists):
    """A ~ B ~ C with A !~ C keeps A and C; a row that duplicates two leaders takes the smaller slot -- on pages found in the
    table by their match counts, so that the case is the kernel's own and not the oracle's."""
    sig, N = lists.sig, lists.N
    m = (sig[:, None, :] == sig[None, :, :]).sum(axis=2)
    live = ~(sig == 0xFFFFFFFF).all(axis=1)
    found = None
    for mm in range(20, 60):
        for b in range(N):
            near = [x for x in np.nonzero((m[b] >= mm) & live)[0] if x != b]
            pair = [(a, c) for a in near for c in near if a < c and m[a, c] < mm]
            if live[b] and pair:
                found = (mm, pair[0][0], b, pair[0][1])
                break
        if found:
            break
    assert found, "the corpus holds no chain"
    mm, a, b, c = found
    doc = np.full((2, M), -1, np.int32)
    doc[0, :3] = [a, b, c]                                   # the chain
    doc[1, :3] = [a, c, b]                                   # two leaders: b duplicates both, a stands first
    n = np.asarray([3, 3], np.int32)
    got, rc = lists.run(mm, doc, n)
    assert rc == 0
    _same(got, lists.want(mm, None, doc, n), 2, "chain")
    assert got[0][0, :2].tolist() == [a, c] and got[4].tolist()[:2] == [2, 2]
    assert (got[5][0, 0], got[6][0, 0], got[7][0, 0]) == (b, a, m[a, b])
    assert got[0][1, :2].tolist() == [a, c] and (got[5][1, 0], got[6][1, 0], got[7][1, 0]) == (b, a, m[a, b])


def test_rejected_pages_neither_drop_nor_lead(lists):
    eng = lists.eng
    plain, _ = lists.run(58)
    try:
        for table in (lists.domain, lists.domain[:lists.N - 30]):             # the second does not reach every document
            eng.bind_doc_domains(table)
            got, rc = lists.run(58)
            assert rc == 0
            _same(got, lists.want(58, table), len(NS), "domain table")
            assert not all((a == b).all() for a, b in zip(got, plain))       # the table changes the answer on these lists
            rejected = np.nonzero(table < 0)[0]
            assert not np.isin(got[5][got[5] >= 0], rejected).any() and not np.isin(got[6][got[6] >= 0], rejected).any()
    finally:
        eng.bind_doc_domains(None)
    got, _ = lists.run(58)
    assert all((a == b).all() for a, b in zip(got, plain))   # unbound again: what it was


def test_collapse_refusals_leave_the_outputs_untouched(lists):
    eng, dev = lists.eng, lists.eng.device
    Q = 3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [up(lists.doc[:Q]), up(lists.score[:Q]), up(lists.orig[:Q]), up(lists.chunk[:Q]), up(lists.n[:Q])]
    i32 = lambda *s: torch.full(s, FILL, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.full(s, -7.5, dtype=torch.float64, device=dev)
    outs = [i32(Q, M), f64(Q, M), f64(Q, M), i32(Q, M), i32(Q), i32(Q, M), i32(Q, M), i32(Q, M), i32(Q)]
    need = eng.lib.msr_collapse_scratch_bytes(Q, M)
    scratch = torch.zeros((need // 8 + 4,), dtype=torch.int64, device=dev)

    def call(q=Q, m=M, mm=58, ins=ins, outs=outs, sc=scratch, nbytes=need, e=eng):
        return e.lib.msr_collapse_duplicates(e.handle, q, *map(_P, ins), m, mm, *map(_P, outs), _P(sc), nbytes, e._stream())

    for kw in (dict(mm=0), dict(mm=65), dict(mm=-3), dict(m=0), dict(m=1025), dict(q=-1), dict(nbytes=need - 1), dict(sc=None),
               dict(sc=scratch.view(torch.int32)[1:])):
        assert call(**kw) == INVALID, kw
        assert eng.lib.msr_last_error(eng.handle)
    for k in range(5):
        assert call(ins=ins[:k] + [None] + ins[k + 1:]) == INVALID, k
    for k in range(9):
        assert call(outs=outs[:k] + [None] + outs[k + 1:]) == INVALID, k
    assert call(q=0, ins=[None] * 5, outs=[None] * 9, sc=None, nbytes=0) == 0            # nothing to do is a success
    # no signatures bound: NOT_BOUND, from the C call and from the engine method
    e2 = DeviceEngine(lists.ix, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        assert not e2.has_signatures and call(e=e2) == NOT_BOUND
        with pytest.raises(_abi.MsrError):
            e2.collapse_duplicates(tuple(ins), 58)
        sig = torch.from_numpy(lists.sig.view(np.int32)).to(dev)
        assert e2.lib.msr_bind_signatures(e2.handle, _P(sig[:-1]), lists.N - 1, e2._stream()) == INVALID      # not the postings' count
        e2.bind_signatures(sig)
        assert e2.has_signatures
        e2.rebind(lists.ix)                                  # a rebind drops the binding with the postings
        assert not e2.has_signatures and call(e=e2) == NOT_BOUND
        e2.bind_signatures(sig)
        e2.bind_signatures(None)
        assert not e2.has_signatures and call(e=e2) == NOT_BOUND
    finally:
        e2.close()
    torch.cuda.synchronize(dev)
    assert all((o == (-7.5 if o.dtype == torch.float64 else FILL)).all() for o in outs)
    assert call() == 0                                       # ... and the same buffers are fine for a good call
    torch.cuda.synchronize(dev)
    assert (outs[4].cpu().numpy() == lists.want(58)[4][:Q]).all()


def test_engine_method_feeds_diversify(lists):
    eng, dev = lists.eng, lists.eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = np.clip(lists.n, 0, M).astype(np.int32)
    fused = (up(lists.doc), up(lists.score), up(lists.orig), up(lists.chunk), up(n))
    kept, drops = eng.collapse_duplicates(fused, 58)
    want = lists.want(58)
    for g, w in zip(list(kept) + list(drops), want):
        assert (g.cpu().numpy() == w).all()
    a = [x.cpu().numpy() for x in eng.diversify(kept, top_k=100, diversification=False)]
    b = [x.cpu().numpy() for x in eng.diversify(tuple(up(w) for w in want[:5]), top_k=100, diversification=False)]
    assert all((x == y).all() for x, y in zip(a, b))
    with pytest.raises(_abi.MsrError):
        eng.collapse_duplicates(fused, 0)
    with pytest.raises(ValueError):
        eng.bind_signatures(torch.zeros((lists.N, 64), dtype=torch.int64, device=dev))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
N_DOCS, N_WORDS = 2400, 1500
PLANTED = ["mensa", "bibliothek", "semesterticket"]          # queries whose pages have copies under other URLs
CONTROL = ["hochschulsport", "wohnheim"]                     # ... and queries whose pages have none


def _crawl():
    """2400 pages of 40 .. 90 tokens over 1500 filler words, each query word on 40 pages of its own.  Of every planted word's
    pages the first 8 have two copies each further on in the index: the same stream but for one token (the print view) and
    the same stream (the mirror), under another scheme or host; the copies' embeddings are the page's plus a little noise."""
    rng = np.random.default_rng(77)
    words = PLANTED + CONTROL
    vocab = {w: i for i, w in enumerate(words)}
    vocab.update({f"w{i}": len(words) + i for i in range(N_WORDS)})
    n_terms = len(vocab)
    streams = [rng.integers(len(words), n_terms, int(rng.integers(40, 91))).astype(np.int32) for _ in range(N_DOCS)]
    urls = [f"https://www.site{d % 37}.de/page/{d}" for d in range(N_DOCS)]
    emb = rng.standard_normal((N_DOCS, 768)).astype(np.float32)
    free = list(rng.permutation(N_DOCS))
    copies = {}
    for t, w in enumerate(words):
        pages = [free.pop() for _ in range(40)]
        for p in pages:
            streams[p][rng.integers(0, len(streams[p]), 3)] = t
        if w in PLANTED:
            for p in pages[:8]:
                a, b = free.pop(), free.pop()
                streams[a] = streams[p].copy()
                streams[a][-1] = len(words) + (int(streams[a][-1]) + 1) % N_WORDS        # the print view: one token differs
                streams[b] = streams[p].copy()                                            # the mirror
                urls[a] = urls[p].replace("https://www.", "http://") + "?print=1"
                urls[b] = urls[p].replace("https://www.", "https://")
                emb[a] = emb[p] + 0.01 * rng.standard_normal(768)
                emb[b] = emb[p] + 0.01 * rng.standard_normal(768)
                copies[p] = (a, b)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    ix, off, tok = ref.index_of(streams, n_terms)
    ix.vocab = vocab
    ix.urls, ix.titles, ix.texts = urls, [f"Seite {d}" for d in range(N_DOCS)], [f"text {d}" for d in range(N_DOCS)]
    ix.titles[5] = None                                      # a page the response models reject
    ix.doc_off = np.arange(N_DOCS + 1, dtype=np.int32)
    ix.chunk_ids = np.arange(N_DOCS, dtype=np.int64)
    ix.emb = emb
    return ix, off, tok, copies


@pytest.fixture(scope="module")
def crawl():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix, off, tok, copies = _crawl()
    qv = torch.randn((8, 768), generator=torch.Generator().manual_seed(5)).numpy()
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    yield ix, off, tok, copies, qv, r
    r.engine.close()


def _oracle_rows(r, sig, ids, qv, mode, mm):
    """The oracle chain for one chunk: the engine's own fused lists, the oracle's collapse, the engine's diversify ->
    (final doc [Q, S], final score, n, per query the drops as (doc, leader, matches) rows)."""
    eng, cfg = r.engine, r.reranker.cfg
    dev = eng.device
    r._ensure_response_tables()
    fused, _ = r._fused_chunk(ids, eng._dev(qv, torch.float32), 1000, None, mode, 100)
    host = [x.cpu().numpy() for x in fused[:5]]
    want = ref.collapse_lists(*host, sig, mm, r._doc_domains())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fin = eng.diversify(tuple(up(w) for w in want[:5]), top_k=int(cfg["top_k"]), diversification=bool(cfg.get("diversification", False)))
    doc, score, _, _, n = [x.cpu().numpy() for x in fin]
    drops = [np.stack([want[5][q, :want[8][q]], want[6][q, :want[8][q]], want[7][q, :want[8][q]]], axis=1) for q in range(len(ids))]
    return doc, score, n, drops, host


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_search_collapses_planted_copies(crawl, mode):
    ix, off, tok, copies, qv, r = crawl
    sig = ref.signatures_fast(off, tok, 4)
    qs = PLANTED + CONTROL
    ids = [[ix.vocab[w]] for w in qs]
    plain = r.search_batch(qs, query_embeddings=qv[:5], term_lists=[[w] for w in qs], mode=mode)
    got = r.search_batch(qs, query_embeddings=qv[:5], term_lists=[[w] for w in qs], mode=mode, collapse_duplicates=True)
    assert r.engine.has_signatures and (_u32(r.engine._t["doc_sig"]) == sig).all()
    doc, score, n, drops, fused = _oracle_rows(r, sig, ids, qv[:5], mode, 58)
    ids_of = _np(ix.doc_ids)
    for q, w in enumerate(qs):
        res = got[q]
        assert isinstance(res, fuzzy.Results) and res.collapsed == len(drops[q])
        # the condition that keeps the test from passing vacuously
        assert (len(drops[q]) >= 1) == (w in PLANTED), (w, len(drops[q]))
        assert [row["doc_id"] for row in res] == [str(int(ids_of[d])) for d in doc[q, :n[q]]], w
        assert [row["score"] for row in res] == score[q, :n[q]].tolist(), w
        led = {}
        for d, lead, m in drops[q].tolist():
            led.setdefault(lead, []).append({"doc_id": str(int(ids_of[d])), "url": ix.urls[d], "title": ix.titles[d] or "No Title",
                                             "similarity": m / 64.0})
        for row, d in zip(res, doc[q, :n[q]]):
            assert row.get("duplicates") == led.get(int(d)), (w, int(d))
            assert ("duplicates" in row) == (int(d) in led)
            if mode == "hybrid":
                assert row["matched_by"] in ("lexical", "dense", "both")
        if w in PLANTED:                                     # a page and its two copies: one of the three is shown, with the others
            shown = {int(d) for d in doc[q, :n[q]]}
            hits = 0
            for p, (a, b) in copies.items():
                if ids[q][0] in tok[off[p]:off[p + 1]]:      # the word's own pages (hybrid: another word's may join by cosine)
                    assert p in fused[0][q, :fused[4][q]]
                    hits += 1
                    # (hybrid: the 100 dense candidates join the list, and the reranker's top_k may cut the one that stays)
                    assert len(shown & {p, a, b}) == 1 or (mode == "hybrid" and not shown & {p, a, b}), (w, p)
            assert hits == 8
            assert len(res) < len(plain[q]) if mode == "lexical" else len(res) <= len(plain[q])
            if mode == "lexical":
                assert any(dup["similarity"] == 1.0 for row in res for dup in row.get("duplicates", ()))
        else:
            assert list(res) == list(plain[q]) and res.collapsed == 0
    # one query at a time, and a threshold that only the mirrors pass
    one = r.search(qs[0], query_embedding=qv[0], terms=[qs[0]], mode=mode, collapse_duplicates=True)
    assert one == got[0] and one.collapsed == got[0].collapsed
    exact = r.search(qs[0], query_embedding=qv[0], terms=[qs[0]], mode=mode, collapse_duplicates=True, duplicate_threshold=1.0)
    _, _, _, d64, _ = _oracle_rows(r, sig, ids[:1], qv[:1], mode, 64)
    assert exact.collapsed == len(d64[0]) and 8 <= exact.collapsed <= one.collapsed
    with pytest.raises(ValueError, match="duplicate_threshold"):
        r.search(qs[0], query_embedding=qv[0], terms=[qs[0]], collapse_duplicates=True, duplicate_threshold=0)
    lines = r.batch_search(list(enumerate(qs)), query_embeddings=qv[:5], term_lists=[[w] for w in qs], mode=mode,
                           collapse_duplicates=True)
    assert lines.collapsed == [g.collapsed for g in got] and [e["url"] for e in lines] == [row["url"] for g in got for row in g]


def test_the_option_off_changes_nothing_and_needs_a_forward_index(crawl):
    ix, off, tok, copies, qv, r = crawl
    qs = PLANTED + CONTROL
    kw = dict(query_embeddings=qv[:5], term_lists=[[w] for w in qs])
    r.search_batch(qs, collapse_duplicates=True, **kw)
    assert r.engine.has_signatures
    after = r.search_batch(qs, **kw)
    fresh = Retriever(indexer=ix, max_queries=8, max_k=1000)                 # one that never built signatures
    try:
        never = fresh.search_batch(qs, **kw)
        assert not fresh.engine.has_signatures
        assert after == never and all(type(x) is list for x in after)
    finally:
        fresh.engine.close()
    bare = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                       "total_docs", "doc_off", "chunk_ids", "emb")})
    bare.vocab, bare.urls, bare.titles, bare.texts = ix.vocab, ix.urls, ix.titles, ix.texts
    r2 = Retriever(indexer=bare, max_queries=8, max_k=1000)
    try:
        with pytest.raises(_abi.MsrError, match="forward index") as e:
            r2.search("mensa", query_embedding=qv[0], terms=["mensa"], collapse_duplicates=True)
        assert e.value.code == -2
        assert r2.search("mensa", query_embedding=qv[0], terms=["mensa"]) == after[0]
    finally:
        r2.engine.close()


def test_a_copy_added_by_update_index_is_collapsed(crawl):
    ix, off, tok, copies, qv, _ = crawl
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    try:
        w = CONTROL[0]
        before = r.search(w, query_embedding=qv[3], terms=[w], collapse_duplicates=True)
        assert before.collapsed == 0 and len(before) >= 2
        top = int(before[0]["doc_id"])
        d = int(np.searchsorted(_np(ix.doc_ids), top))
        new_id = int(_np(ix.doc_ids).max()) + 4
        stream = tok[off[d]:off[d + 1]]
        meta = {new_id: (ix.urls[d].replace("https://www.", "http://"), "Kopie", "text")}
        grown = bm25_add_token_ids(ix, np.asarray([new_id], np.int64), np.asarray([0, len(stream)], np.int64), stream, ix.n_terms,
                                   vocab=ix.vocab, docs_meta=meta)
        assert grown.tok_off is not None
        e = torch.as_tensor(_np(ix.emb)[d:d + 1])
        grown = attach_chunks(grown, ChunkTable(chunk_ids=np.asarray([int(_np(ix.chunk_ids).max()) + 1], np.int64),
                                                doc_ids=np.asarray([new_id], np.int64), seqs=[[1]], emb=e))
        r.update_index(grown)
        assert not r.engine.has_signatures                   # the rebind dropped the table of the old index
        plain = r.search(w, query_embedding=qv[3], terms=[w])
        assert {str(top), str(new_id)} <= {row["doc_id"] for row in plain}
        after = r.search(w, query_embedding=qv[3], terms=[w], collapse_duplicates=True)
        assert r.engine.has_signatures and int(r.engine._t["doc_sig"].shape[0]) == grown.n_docs
        assert after.collapsed == 1 and len(after) == len(plain) - 1
        lead = [row for row in after if "duplicates" in row]
        assert len(lead) == 1 and {lead[0]["doc_id"], lead[0]["duplicates"][0]["doc_id"]} == {str(top), str(new_id)}
        assert lead[0]["duplicates"][0]["similarity"] == 1.0
    finally:
        r.engine.close()

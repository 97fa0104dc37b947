"""Query-biased snippets on the GPU (msr_best_windows, DeviceEngine.best_windows, the facades; DESIGN K14): the kernel against
the plain-loop oracle of snippet_ref.py, all five outputs, exactly -- the hand-made streams (chunk geometry, document ends,
neighbouring documents, every kind of row), proximity_ref's corpora, every pair count around the workgroup's four waves,
pairs out of range, padding, determinism, 300 random pairs against the numpy formulation; the ABI refusals; and the
consumers -- Retriever.search in both modes and /api/search return the same documents, ranks and scores with snippets=True,
and every row's snippet, highlights and missing terms are snippets.render of the oracle's window."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr._abi import MsrError
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import bm25_index_from_token_ids, normalise_document_text, tokens_from_texts
from msretr.retriever import Retriever
from msretr.snippets import query_row, render, term_weights
from msretr.text import preprocess_query, simple_tokenize, simple_tokenize_spans
from phrase_ref import BIG, N_RANDOM, N_TERMS
from snippet_ref import NONE, VARIANTS, best_window, best_windows_fast, corpus_cases, expected, hand

pytestmark = pytest.mark.gpu
PAD = 3                                                      # entries behind n_pairs that must keep the fill
FILLS = (0x5A5A5A5A, 0x3C3C3C3C, 0x77777777, 0x1234567890ABCDEF, 0xA5A5A5A5)
DTYPES = (np.int32, np.int32, np.int32, np.uint64, np.uint32)
MSR_ERR_INVALID, MSR_ERR_NOT_BOUND = -1, -2                # msretr.h


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a if len(a) else [0], np.int32)).to(dev)


def _filled(n, dev):
    """The five output buffers of n + PAD entries, each pre-filled with a pattern of its own."""
    out = []
    for fill, dt in zip(FILLS, DTYPES):
        host = np.full(n + PAD, fill, np.uint64 if dt == np.uint64 else np.uint32)
        out.append(torch.from_numpy(host.view(np.int64 if dt == np.uint64 else np.int32)).to(dev))
    return out


def _host(outs):
    return [t.cpu().numpy().view(dt) for t, dt in zip(outs, DTYPES)]


def _rows(c, dev):
    off, terms, wts = [0], [], []
    for p, w in zip(c.rows, c.weights):
        terms += list(p); wts += list(w); off.append(len(terms))
    return _i32(off, dev), _i32(terms, dev), _i32(wts, dev), _i32(c.spans, dev)


def _run(eng, c, pair_doc, pair_row, n_rows=None):
    """One msr_best_windows call into pre-filled buffers of n + PAD entries -> the five host arrays (padding included)."""
    dev, n = eng.device, len(pair_doc)
    outs = _filled(n, dev)
    off, terms, wts, spans = _rows(c, dev)
    d_doc, d_row = _i32(pair_doc, dev), _i32(pair_row, dev)  # (named: a temporary's memory would be reused by the next one)
    rc = eng.lib.msr_best_windows(eng.handle, n, _P(d_doc), _P(d_row),
                                  len(c.rows) if n_rows is None else n_rows, _P(off), _P(terms), _P(wts), _P(spans),
                                  *[_P(t) for t in outs], eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    return _host(outs)


def _check(got, want, pairs=None):
    """want: the oracle's 5-tuples; the PAD entries behind them keep the fill."""
    n = len(want)
    for x, fill, dt in zip(got, FILLS, DTYPES):
        assert x.shape == (n + PAD,) and x.dtype == dt
        assert (x[n:] == dt(fill & (2 ** (8 * np.dtype(dt).itemsize) - 1))).all(), "entries at or above n_pairs were touched"
    for i, w in enumerate(want):
        assert tuple(int(x[i]) for x in got) == w, (i, None if pairs is None else pairs[i], w)


def _bytes(got):
    return b"".join(x.tobytes() for x in got)


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    made = {}

    def get(key):
        if key not in made:
            c = hand() if key == "hand" else corpus_cases(*key)
            made[key] = (c, DeviceEngine(c.ix, max_queries=4, max_k=16, rerank_max_docs=0))
        return made[key]
    yield get
    for _, e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------------ the kernel
def test_hand_made_cases_every_pair_twice(engines):
    c, eng = engines("hand")
    assert eng.has_tokens and int(_np(c.ix.tok_ids).size) == int(c.tok_off[-1])      # tok_ids is sized exactly
    want = expected("hand")
    docs, rows = [p[0] for p in c.pairs], [p[1] for p in c.pairs]
    a = _run(eng, c, docs, rows)
    _check(a, want, c.pairs)
    assert _bytes(_run(eng, c, docs, rows)) == _bytes(a)     # a second set of buffers: the same bytes
    # every scan width and both kinds of answer are among them
    assert {len(c.rows[r]) for r in rows} >= {0, 1, 4, 5, 8, 9, 16, 17}
    assert {c.spans[r] for r in rows} >= {0, 1, 2, 63, 64, 65}
    assert 150 < sum(w != NONE for w in want) < len(want) - 50
    assert max(w[1] for w in want) == 1 << 24 and any(w[3] >> 63 for w in want)
    # a pair alone gives what it gives inside the batch
    for i in sorted({0, 7, len(want) // 2, len(want) - 1} | {i for i, p in enumerate(c.pairs) if "2^24" in p[2] or "tie" in p[2]}):
        _check(_run(eng, c, docs[i:i + 1], rows[i:i + 1]), want[i:i + 1], c.pairs[i:i + 1])


@pytest.mark.parametrize("key", VARIANTS, ids=str)
def test_kernel_against_the_oracle_on_the_proximity_corpora(engines, key):
    c, eng = engines(key)
    want = expected(key)
    got = _run(eng, c, [p[0] for p in c.pairs], [p[1] for p in c.pairs])
    _check(got, want, c.pairs)
    assert any(w != NONE for w in want) and any(w == NONE for w in want)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_pair_counts_around_the_four_waves_of_a_workgroup(engines, n):
    c, eng = engines("hand")
    want_all = expected("hand")
    hits = [i for i, w in enumerate(want_all) if w != NONE]
    pick = [hits[(7 * i) % len(hits)] if i % 3 else (11 * i) % len(want_all) for i in range(n)]
    got = _run(eng, c, [c.pairs[i][0] for i in pick], [c.pairs[i][1] for i in pick])
    _check(got, [want_all[i] for i in pick])                 # n == 0: nothing but the untouched padding


def test_pairs_out_of_range_and_the_same_pair_twice(engines):
    c, eng = engines("hand")
    want_all = expected("hand")
    i = next(k for k, w in enumerate(want_all) if w != NONE and w[2] > 1 and c.pairs[k][1] >= 1)
    d, r = c.pairs[i][:2]
    N, R = c.n_docs, len(c.rows)
    docs = [d, -1, N, d, d, d, N + 5, -2 ** 31, 2 ** 31 - 1, d, N - 1]
    rows = [r, r, r, -1, R, r, -1, r, r, 2 ** 31 - 1, r]
    want = [want_all[i], NONE, NONE, NONE, NONE, want_all[i], NONE, NONE, NONE, NONE,
            best_window(c.streams[N - 1], c.rows[r], c.weights[r], c.spans[r])]
    _check(_run(eng, c, docs, rows), want)
    # n_rows smaller than the row buffer: a row at or above it is out of range
    _check(_run(eng, c, [d, d], [r, 0], n_rows=r), [NONE, best_window(c.streams[d], c.rows[0], c.weights[0], c.spans[0])])


def _random_rows(rng, n):
    rows, weights, spans = [], [], []
    for i in range(n):
        L = (1, 2, 3, 4, 5, 8, 9, 16)[i % 8]
        rows.append(rng.integers(0, N_RANDOM, L).tolist())   # repeats happen
        weights.append(rng.choice([0, 1, 5, 900, 1 << 20], L).tolist() if i % 3 else rng.integers(0, 4, L).tolist())
        spans.append(int(rng.integers(1, 65)) if i % 4 else (1, 64, 30, 63)[(i // 4) % 4])
    rows.append([3, N_TERMS]); weights.append([1, 1]); spans.append(9)      # an invalid row among them
    return rows, weights, spans


def test_300_random_pairs_in_one_call(engines):
    """The oracle here is best_windows_fast, which test_snippet_cases.py holds against the plain loops."""
    c, eng = engines((BIG, False))
    assert c.n_docs == 16421
    rng = np.random.default_rng(14)
    rows, weights, spans = _random_rows(rng, 24)
    docs = rng.integers(0, c.n_docs, 300).tolist()
    prow = rng.integers(0, len(rows), 300).tolist()
    long = np.nonzero(np.diff(c.tok_off) > 200)[0].tolist()
    docs[:len(long)] = long                                  # the long planted documents too
    rc = type(c)(c.streams, c.ix, c.tok_off, c.tok_ids, rows, weights, spans)
    want = best_windows_fast(c.tok_off, c.tok_ids, docs, prow, rows, weights, spans)
    got = _run(eng, rc, docs, prow)
    _check(got, [tuple(int(x[i]) for x in want) for i in range(300)], list(zip(docs, prow)))
    assert _bytes(_run(eng, rc, docs, prow)) == _bytes(got)
    found = int((want[0] >= 0).sum())
    assert 150 < found < 300, found


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(engines):
    c, eng = engines("hand")
    dev = eng.device
    off, terms, wts, spans = _rows(c, dev)
    d, r = _i32([0, 1], dev), _i32([0, 0], dev)
    outs = _filled(2, dev)
    before = _bytes(_host(outs))
    args = [_P(d), _P(r), len(c.rows), _P(off), _P(terms), _P(wts), _P(spans)] + [_P(t) for t in outs]
    call = lambda n, a: eng.lib.msr_best_windows(eng.handle, n, *a, eng._stream())
    for k in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11):            # every pointer NULL in turn
        bad = list(args)
        bad[k] = C.c_void_p(0)
        assert call(2, bad) == MSR_ERR_INVALID, k
        assert b"msr_best_windows" in eng.lib.msr_last_error(eng.handle)
    zero_rows = list(args); zero_rows[2] = 0
    assert call(2, zero_rows) == MSR_ERR_INVALID
    neg_rows = list(args); neg_rows[2] = -1
    assert call(2, neg_rows) == MSR_ERR_INVALID and call(-1, args) == MSR_ERR_INVALID
    nulls = [C.c_void_p(0), C.c_void_p(0), 0] + [C.c_void_p(0)] * 9
    assert call(0, nulls) == 0 and call(0, args) == 0         # n_pairs == 0 succeeds and launches nothing
    torch.cuda.synchronize(dev)
    assert _bytes(_host(outs)) == before
    # no tokens bound
    ix = CorpusIndex(**{k: getattr(c.ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                       "total_docs")})
    bare = DeviceEngine(ix, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        assert not bare.has_tokens
        assert bare.lib.msr_best_windows(bare.handle, 2, *args, bare._stream()) == MSR_ERR_NOT_BOUND
        torch.cuda.synchronize(dev)
        assert _bytes(_host(outs)) == before
        with pytest.raises(MsrError, match="forward index"):
            bare.best_windows([0], [0], [[1]], [[1]], 5)
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------ DeviceEngine.best_windows
def test_engine_best_windows(engines):
    c, eng = engines("hand")
    want = expected("hand")
    docs, rows = np.array([p[0] for p in c.pairs]), np.array([p[1] for p in c.pairs])
    out = eng.best_windows(docs, rows, c.rows, c.weights, c.spans)
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int32, torch.int64, torch.int32]
    assert all(t.is_cuda and t.shape == (len(want),) for t in out)
    got = _host(out)
    for i, w in enumerate(want):
        assert tuple(int(x[i]) for x in got) == w, c.pairs[i]
    # device tensors for the pairs; python lists; one span for every row
    dev_out = eng.best_windows(torch.from_numpy(docs).to(eng.device), torch.from_numpy(rows).to(eng.device), c.rows, c.weights,
                               c.spans)
    assert _bytes(_host(dev_out)) == _bytes(got)
    same = [r for r in range(len(c.rows)) if c.spans[r] == 64]
    sel = [i for i, p in enumerate(c.pairs) if p[1] in same]
    one = eng.best_windows([c.pairs[i][0] for i in sel], [same.index(c.pairs[i][1]) for i in sel], [c.rows[r] for r in same],
                           [c.weights[r] for r in same], 64)
    assert [tuple(int(x[k]) for x in _host(one)) for k in range(len(sel))] == [want[i] for i in sel]
    empty = eng.best_windows([], [], c.rows, c.weights, c.spans)
    assert all(t.numel() == 0 for t in empty)
    with pytest.raises(ValueError):
        eng.best_windows([0], [0], [[1, 2]], [[1]], 5)
    with pytest.raises(ValueError):
        eng.best_windows([0], [0], [[1, 2]], [[1, 1]], [5, 6])


# ------------------------------------------------------------------------------------------------ the facades
N_DOCS, V = 1201, 150
PA, PB, PC = V, V + 1, V + 2                                 # "alpha", "beta", "gamma"


def _word(t):
    if t == 0:
        return "tübingen"
    if t >= V:
        return ("alpha", "beta", "gamma")[t - V]
    s, t = "", int(t)
    while True:
        s = chr(ord("a") + t % 26) + s
        t //= 26
        if t == 0:
            return "w" + s


# words of the Zipf tail: about a sixth of the pages hold each, so their idf is positive (the commonest words stand on nearly
# every page, their idf is negative, and a lexical query of them finds nothing, as in the reference)
RARER = " ".join(_word(t) for t in (60, 75, 90))


def _shown(d, k, t):
    """How token k of document d is written on the page: capitals, and for the city one of its ASCII spellings now and then."""
    w = _word(t)
    if t == 0 and d % 7 == 0:
        return ("Tuebingen", "TUBINGEN")[k % 2]
    return w.capitalize() if (d + k) % 5 == 0 else w


@pytest.fixture(scope="module")
def corp():
    """1201 pages of 8 .. 160 Zipf words behind a title of one or two words, built on the GPU with keep_tokens=True; the page
    texts carry capitals, commas and (every seventh page) ASCII spellings of the city.  Page d holds, by d % 10: 0 alpha beta
    gamma; 1 alpha .. beta far apart; 2 beta alone; else none of the three.  tokens_from_texts of the pages is the stream."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    rng = np.random.default_rng(23)
    w = 1.0 / np.arange(1, V) ** 1.07
    streams, titles, texts = [], [], []
    for d in range(N_DOCS):
        s = (1 + rng.choice(V - 1, int(rng.integers(8, 161)), p=w / w.sum())).tolist()
        if rng.random() < 0.3:
            s[int(rng.integers(0, len(s)))] = 0
        at = int(rng.integers(1, len(s) + 1))
        ins = {0: [PA, PB, PC], 2: [PB]}.get(d % 10, [])
        s = s[:at] + ins + s[at:]
        if d % 10 == 1:
            s = [PA] + s + [PB]
        nt = 1 + d % 2
        title = s[:nt] if d % 13 else []
        body = s[len(title):]
        streams.append(s)
        titles.append(" ".join(_shown(d, k, t) for k, t in enumerate(title)) if d % 13 else (None if d % 2 else ""))
        texts.append("".join(_shown(d, len(title) + k, t) + (", " if k % 7 == 6 else " ") for k, t in enumerate(body)).strip())
    off = np.zeros(N_DOCS + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    tok = np.asarray([t for s in streams for t in s], np.int32)
    ids = np.arange(N_DOCS, dtype=np.int64) * 2 + 100
    ix = bm25_index_from_token_ids(ids, off, tok, V + 3, device="cuda", keep_tokens=True)
    cnt = 1 + np.arange(N_DOCS) % 3
    ix.doc_off = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
    n_chunks = int(cnt.sum())
    ix.chunk_ids = torch.arange(n_chunks, dtype=torch.int64)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn((n_chunks, 768), generator=g)
    ix.emb = emb / emb.norm(dim=1, keepdim=True)
    hosts = ["uni-tuebingen.de", "tuebingen.de", "example.org"]
    ix.urls = [f"https://{hosts[d % 3]}/doc{d}" for d in range(N_DOCS)]
    ix.titles, ix.texts = titles, texts
    ix.vocab = {_word(t): t for t in range(V + 3)}
    t_off, t_ids = tokens_from_texts(ix)                     # the pages tokenise to the indexed streams
    assert t_off.tolist() == off.tolist() and t_ids.tobytes() == tok.tobytes()
    qv = (ix.emb[rng.integers(0, n_chunks, 6)] + 0.3 * torch.randn((6, 768), generator=g)).numpy() * 7.0
    # the star: a page without the city and without the planted words whose first chunk is query vector 1 -- the dense
    # stage's best hit for that vector, which the lexical stage cannot see
    star = next(d for d in range(50, N_DOCS) if d % 10 > 2 and 0 not in streams[d])
    ix.emb[int(ix.doc_off[star])] = torch.from_numpy(qv[1] / np.linalg.norm(qv[1]))
    ix.star = star
    return ix, streams, np.ascontiguousarray(qv, np.float32)


@pytest.fixture(scope="module")
def eng(corp):
    e = DeviceEngine(corp[0], max_queries=16, max_k=1000, rerank_max_docs=1000)
    yield e
    e.close()


def _reference_snippet(text):
    return (text[:200] + "..." if len(text) > 200 else text) or "No content available"


def _check_rows(ix, streams, query, got, plain, span, terms=None):
    """Every row of `got` against `plain` (the same call without snippets) and against render of the oracle's window."""
    strip = lambda row: {k: v for k, v in row.items() if k not in ("snippet", "highlights", "missing")}
    assert [strip(r) for r in got] == plain_stripped(plain) and len(got) == len(plain)
    ids = ix.term_ids(terms if terms is not None else simple_tokenize(preprocess_query(query)))
    row = query_row(ix, ids)
    names = [] if row is None else [next(w for w, t in ix.vocab.items() if t == i) for i in row]
    kinds = {"window": 0, "none": 0}
    for r_got, r_plain in zip(got, plain):
        d = (int(r_got["doc_id"]) - 100) // 2
        want = NONE if row is None else best_window(streams[d], row, term_weights(ix, row), span, ix.n_terms)
        if want == NONE:
            assert r_got["snippet"] == r_plain["snippet"] == _reference_snippet(ix.texts[d])
            assert r_got["highlights"] == [] and r_got["missing"] == names
            kinds["none"] += 1
            continue
        snippet, hl = render(ix.titles[d], ix.texts[d], want[0], want[3], span)
        assert (r_got["snippet"], r_got["highlights"]) == (snippet, hl), (d, want)
        assert r_got["missing"] == [w for j, w in enumerate(names) if not want[4] >> j & 1]
        for b, e in hl:                                      # the invariant: a highlighted slice is one token, a term of the row
            toks = simple_tokenize(normalise_document_text("", snippet[b:e]))
            assert len(toks) == 1 and toks[0] in names, (snippet, b, e)
        kinds["window"] += 1
    return kinds


def plain_stripped(rows):
    return [{k: v for k, v in r.items() if k != "snippet"} for r in rows]


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_search_with_snippets_returns_the_same_rows_and_the_oracles_passages(corp, eng, mode):
    ix, streams, qv = corp
    r = Retriever(indexer=eng)
    kw = dict(query_embedding=qv[0], mode=mode)
    for query, span in (("alpha beta gamma", 30), ("Beta alpha", 5), (f"alpha {RARER}", 64), ("gamma", 1)):
        plain = r.search(query, **kw)
        got = r.search(query, snippets=True, snippet_tokens=span, **kw)
        assert plain, query
        assert [row["score"] for row in got] == [row["score"] for row in plain], query          # bit for bit
        kinds = _check_rows(ix, streams, query, got, plain, span)
        assert kinds["window"] >= 10
        assert all(set(row) - set(p) == {"highlights", "missing"} for row, p in zip(got, plain))
    # the default window is 30 tokens
    assert r.search("alpha beta", snippets=True, **kw) == r.search("alpha beta", snippets=True, snippet_tokens=30, **kw)
    # pages with the three words next to each other show them, all highlighted, nothing but the city missing at most
    got = r.search("alpha beta gamma", snippets=True, snippet_tokens=3, **kw)
    full = [row for row in got if ((int(row["doc_id"]) - 100) // 2) % 10 == 0]
    assert len(full) >= 5
    for row in full:
        assert [row["snippet"][b:e].lower() for b, e in row["highlights"]] == ["alpha", "beta", "gamma"]
        assert row["missing"] == ["tübingen"]
    # off: the rows are what they were
    assert r.search("alpha beta", snippets=False, **kw) == r.search("alpha beta", **kw)
    assert "highlights" not in r.search("alpha beta", **kw)[0]


def test_a_dense_only_hit_and_a_query_without_a_row_keep_the_reference_snippet(corp, eng):
    ix, streams, qv = corp
    r = Retriever(indexer=eng)
    # a word no page holds: the city alone scores; the dense stage adds pages without it
    kw = dict(query_embedding=qv[1], mode="hybrid", dense_k=100)
    plain = r.search("unbekannteswort", **kw)
    got = r.search("unbekannteswort", snippets=True, **kw)
    kinds = _check_rows(ix, streams, "unbekannteswort", got, plain, 30)
    dense_only = [row for row in got if row["matched_by"] == "dense" and 0 not in streams[(int(row["doc_id"]) - 100) // 2]]
    assert dense_only and kinds["none"] >= len(dense_only) and kinds["window"] > 0
    assert str(ix.star * 2 + 100) in [row["doc_id"] for row in dense_only]
    for row in dense_only:
        assert row["highlights"] == [] and row["missing"] == ["tübingen"]
        assert row["snippet"] == _reference_snippet(ix.texts[(int(row["doc_id"]) - 100) // 2])
    # a query of unknown words only (caller-supplied terms: no city): no row, every result is the dense stage's
    plain = r.search("x", terms=["zzz", "yyy"], **kw)
    got = r.search("x", terms=["zzz", "yyy"], snippets=True, **kw)
    assert got and _check_rows(ix, streams, "x", got, plain, 30, terms=["zzz", "yyy"]) == {"window": 0, "none": len(got)}
    assert all(row["missing"] == [] for row in got)
    # lexical mode, nothing found
    assert r.search("x", terms=["zzz"], query_embedding=qv[1], snippets=True) == []


def test_batches_tokenizers_and_what_the_facade_refuses(corp, eng):
    ix, streams, qv = corp
    r = Retriever(indexer=eng)
    qs = ["alpha beta", f"gamma {_word(60)}", "beta"]
    got = r.search_batch(qs, query_embeddings=qv[:3], snippets=True, snippet_tokens=12)
    for q in range(3):
        assert got[q] == r.search(qs[q], query_embedding=qv[q], snippets=True, snippet_tokens=12)
    lines = r.batch_search(list(zip("123", qs)), query_embeddings=qv[:3], snippets=True, snippet_tokens=12)
    plain_lines = r.batch_search(list(zip("123", qs)), query_embeddings=qv[:3])
    assert lines.text() == plain_lines.text() and "snippet" not in plain_lines[0]
    second = [e for e in lines if e["query_num"] == "2"]
    assert [(e["snippet"], e["highlights"], e["missing"]) for e in second][:len(got[1])] == \
        [(row["snippet"], row["highlights"], row["missing"]) for row in got[1]]
    # a custom tokenizer needs its spans
    custom = Retriever(indexer=eng, tokenizer=simple_tokenize)
    with pytest.raises(ValueError, match="span_tokenizer"):
        custom.search("alpha beta", query_embedding=qv[0], snippets=True)
    assert custom.search("alpha beta", query_embedding=qv[0]) == r.search("alpha beta", query_embedding=qv[0])
    spans = Retriever(indexer=eng, tokenizer=simple_tokenize, span_tokenizer=simple_tokenize_spans)
    assert spans.search("alpha beta", query_embedding=qv[0], snippets=True) == r.search("alpha beta", query_embedding=qv[0],
                                                                                        snippets=True)
    for bad in (65, 0, -1, 2.5, None):
        with pytest.raises(ValueError, match="snippet_tokens"):
            r.search("alpha beta", query_embedding=qv[0], snippets=True, snippet_tokens=bad)
    r.search("alpha beta", query_embedding=qv[0], snippet_tokens=65)         # off: not looked at
    # an index without texts raises what phrase search raises without a forward index
    texts, ix.texts = ix.texts, None
    try:
        with pytest.raises(MsrError, match="texts"):
            r.search("alpha beta", query_embedding=qv[0], snippets=True)
    finally:
        ix.texts = texts


def test_http_search_with_snippets(corp, eng):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, streams, qv = corp
    r = Retriever(indexer=eng)
    seen = []
    client = TestClient(create_app(r, llm=lambda query, windows: seen.append(windows) or "summary"))
    body = {"query": "alpha beta gamma", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    snip = client.post("/api/search", json=dict(body, snippets=True, snippet_tokens=8))
    assert plain.status_code == 200 and snip.status_code == 200
    want = r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", snippets=True, snippet_tokens=8)
    assert snip.json()["documents"] == want and want
    assert plain.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1")
    assert plain_stripped(plain.json()["documents"]) == [
        {k: v for k, v in row.items() if k not in ("snippet", "highlights", "missing")} for row in want]
    # the summariser receives the new snippets
    assert seen[1] == [row["snippet"] for row in want[:10]] and seen[0] != seen[1] and snip.json()["llm_response"] == "summary"
    hybrid = client.post("/api/search", json=dict(body, mode="hybrid", snippets=True))
    assert hybrid.status_code == 200
    assert hybrid.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", mode="hybrid",
                                                  snippets=True)
    for bad in (65, 0):
        resp = client.post("/api/search", json=dict(body, snippets=True, snippet_tokens=bad))
        assert resp.status_code == 400 and "snippet_tokens" in resp.json()["error"]
    custom = TestClient(create_app(Retriever(indexer=eng, tokenizer=simple_tokenize)))
    resp = custom.post("/api/search", json=dict(body, snippets=True))
    assert resp.status_code == 400 and "span_tokenizer" in resp.json()["error"]
    assert custom.post("/api/search", json=body).json()["documents"] == plain.json()["documents"]

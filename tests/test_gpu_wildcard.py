"""Prefix and wildcard lookup on the GPU (msr_wildcard_terms, DeviceEngine.wildcard_terms, the facades; DESIGN K16): the
kernels against the unfiltered table-filling oracle of wildcard_ref.py, all three outputs, exactly -- the hand vocabulary at
every limit, vocabularies around the span a workgroup owns with every term matching, pattern counts around the LDS group, the
random case, determinism, padding; the ABI's refusals; and the consumers on the small synthetic crawl of the fuzzy tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr import _abi
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from msretr.retriever import Retriever
from test_gpu_fuzzy import _crawl, _postings_only
from wildcard_ref import KNOWN, expected, hand, image, pack_words, random_case

pytestmark = pytest.mark.gpu
PAD = 2                                                      # rows behind n_patterns that must keep the fill
FILLS = (0x5A5A5A5A, 0x77777777, 0x12345678)                # out_term, out_n, out_total
MSR_ERR_INVALID, MSR_ERR_NOT_BOUND = -1, -2                 # msretr.h
S, G = _abi.MSR_FUZZY_SPAN_TERMS, _abi.MSR_FUZZY_WORD_GROUP
RANDOM_LIMIT = 3


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Bound:
    """An engine over postings-only terms with a vocabulary image bound through the raw ABI (test_gpu_fuzzy.Bound's way)."""

    def __init__(self, vocab, weights, bind=True):
        self.vocab, self.weights = list(vocab), list(weights)
        self.eng = DeviceEngine(_postings_only(len(vocab)), max_queries=4, max_k=16, rerank_max_docs=0)
        assert not self.eng.has_vocab
        self.rc = None
        if bind:
            char_off, chars, weight = image(vocab, weights)
            dev = self.eng.device
            self.keep = (torch.from_numpy(np.asarray(char_off, np.int64)).to(dev),
                         torch.from_numpy(np.asarray(chars if len(chars) else [0], np.uint16).view(np.int16)).to(dev),
                         torch.from_numpy(np.asarray(weight, np.uint32).view(np.int32)).to(dev))
            self.rc = self.eng.lib.msr_bind_vocab(self.eng.handle, _P(self.keep[0]), _P(self.keep[1]), _P(self.keep[2]),
                                                  len(vocab), len(chars), self.eng._stream())

    def buffers(self, n, limit):
        dev = self.eng.device
        mk = lambda fill, size: torch.from_numpy(np.full(size, fill, np.uint32).view(np.int32)).to(dev)
        return [mk(FILLS[0], (n + PAD) * limit), mk(FILLS[1], n + PAD), mk(FILLS[2], n + PAD)]

    def call(self, patterns, limit, outs, n_patterns=None, scratch_bytes=None, null=None, misalign=False, keep_scratch=False):
        """One raw msr_wildcard_terms call -> rc.  null: the position of a pointer argument to pass as NULL (0 pat_off, 1
        pat_chars, 2 .. 4 the outputs, 5 the scratch); misalign: the scratch 4 bytes off an 8-byte boundary."""
        dev, n = self.eng.device, len(patterns)
        off, chars = pack_words(patterns)
        d_off = torch.from_numpy(off).to(dev)
        d_chars = torch.from_numpy(np.asarray(chars if len(chars) else [0], np.uint16).view(np.int16)).to(dev)
        need = int(self.eng.lib.msr_wildcard_scratch_bytes(len(self.vocab), max(n, 0), limit))
        scratch = torch.full((max(need, 8) // 8 + 2,), 0x0BADBADBADBADBAD, dtype=torch.int64, device=dev)
        sp = C.c_void_p(scratch.data_ptr() + (4 if misalign else 0))
        ptrs = [_P(d_off), _P(d_chars)] + [_P(t) for t in outs] + [sp]
        if null is not None:
            ptrs[null] = C.c_void_p(0)
        rc = self.eng.lib.msr_wildcard_terms(self.eng.handle, n if n_patterns is None else n_patterns, ptrs[0], ptrs[1], limit,
                                             ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                             need if scratch_bytes is None else scratch_bytes, self.eng._stream())
        torch.cuda.synchronize(dev)
        if keep_scratch:
            self.scratch = scratch.cpu().numpy()[:max(need, 0) // 8 + (need % 8 > 0)]
        return rc

    def run(self, patterns, limit, keep_scratch=False):
        """-> the three host arrays, padding included, of one call into pre-filled buffers."""
        outs = self.buffers(len(patterns), limit)
        rc = self.call(patterns, limit, outs, keep_scratch=keep_scratch)
        assert rc == 0, self.eng.lib.msr_last_error(self.eng.handle)
        return [t.cpu().numpy() for t in outs]

    def check(self, patterns, limit, want=None):
        got = self.run(patterns, limit)
        n = len(patterns)
        want = expected(self.vocab, self.weights, patterns, limit) if want is None else want
        for x, fill, size in zip(got, FILLS, (n * limit, n, n)):
            assert (x[size:].view(np.uint32) == fill).all(), "rows at or above n_patterns were touched"
        for name, x, w in zip(("term", "n", "total"), got, want):
            x = x[:w.size].reshape(w.shape)
            bad = np.argwhere(x != w)
            assert len(bad) == 0, (name, bad[:5].tolist(), [patterns[int(b[0])] for b in bad[:5]], x[bad[0][0]].tolist(),
                                   w[bad[0][0]].tolist())
        return got, want

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def hand_vocab():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    vocab, weights, patterns = hand()
    b = Bound(vocab, weights)
    assert b.rc == 0
    yield b, patterns
    b.close()


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("limit", [1, 2, 8, 16])
def test_hand_vocabulary_every_pattern(hand_vocab, limit):
    b, patterns = hand_vocab
    assert {len(s) for s in b.vocab} >= {1, 2, 31, 32, 33} and {len(p) for p in patterns} >= {0, 1, 31, 32, 33}
    assert b.weights[b.vocab.index("geist")] == 0 and "geist" in patterns and set(p for p, _ in KNOWN) <= set(patterns)
    assert any("\ufffe" in s for s in b.vocab) and "x?y" in patterns
    got, want = b.check(patterns, limit)
    total = dict(zip(patterns, want[2].tolist()))
    assert total["geist"] == 0 and total["gei?t"] == 0 and total["x?y"] == 1 and total["x?"] == 1 and total["t?bingen"] == 2
    assert total["?aus"] == 4 and total[""] == 0 and total["*" * 33] == 0 and total["a" * 32 + "*"] == 0
    assert total["*"] == sum(1 for s, w in zip(b.vocab, b.weights) if w > 0 and len(s) <= 32) > 16
    assert total["a" * 31 + "?"] == 1 and total["a" * 30 + "?"] == 1 and total["*" * 31 + "b"] >= 3 and total["?" * 32] == 1
    assert total["mensa"] == 1 and total["wer?"] == 1 and total["a?b"] == 2           # `a?b`: "aab" and the term "a*b"
    row = dict(zip(patterns, want[0].tolist()))
    haus = b.vocab.index("haus")
    assert row["?aus"][:min(limit, 4)] == [haus, haus + 1, haus + 2, haus + 3][:limit]                   # the id decides
    assert row["t?bingen"][0] == b.vocab.index("tübingen")                                               # the weight decides
    for i in (0, 1, 2, len(patterns) - 3):                   # a pattern alone gives what it gives inside the call
        b.check(patterns[i:i + 1], limit)


def _all_match_vocab(n_terms):
    """n_terms distinct terms that all match `a*`, equal weights."""
    return ["a" + format(i, "x") for i in range(n_terms)], [3] * n_terms


@pytest.mark.parametrize("n_terms", [S - 1, S, S + 1, 2 * S + 1])
def test_every_term_matches_around_a_span(n_terms):
    vocab, weights = _all_match_vocab(n_terms)
    b = Bound(vocab, weights)
    try:
        assert b.rc == 0
        for limit in (1, 16):
            got, want = b.check(["a*", "a?*", "*", "b*", "a0", "a*0", "*f"], limit)
            assert want[0][0].tolist() == list(range(limit)) and want[2][0] == n_terms      # 64 per wave, all waves, all spans
        # the single heaviest match in the last term of the last span
        b.close()
        weights[-1] = 9
        b = Bound(vocab, weights)
        assert b.rc == 0
        got, want = b.check(["a*", vocab[-1], "a*" + vocab[-1][-1]], 16)
        assert want[0][0].tolist() == [n_terms - 1] + list(range(15)) and want[0][1][0] == n_terms - 1 == want[0][2][0]
        b.check(["a*"], 1, want=(np.asarray([[n_terms - 1]], np.int32), np.asarray([1], np.int32), np.asarray([n_terms], np.int32)))
    finally:
        b.close()


@pytest.mark.parametrize("n_patterns", [1, G - 1, G, G + 1, 2 * G + 1])
def test_pattern_counts_around_the_lds_group(hand_vocab, n_patterns):
    b, patterns = hand_vocab
    assert (G - 1, G, G + 1, 2 * G + 1) == (15, 16, 17, 33)
    kinds = ["a*", "*b", "ab*ab", "*a*b*", "mensa", "t?bingen", "", "*ab*ab", "?aus", "a*ba", "a" * 33, "*bib*", "??", "a**b"]
    pick = [kinds[(5 * i + i // 7) % len(kinds)] for i in range(n_patterns)]
    got, want = b.check(pick, 2)
    if n_patterns >= G:
        assert (want[2] > 2).any() and (want[2] == 0).any()


def test_random_case_all_three_outputs_and_the_same_bytes_twice():
    vocab, weights, patterns = random_case()
    assert len(vocab) == 3000 and len(patterns) == 64 and max(weights) == 2 ** 31 - 1 and min(weights) == 0
    b = Bound(vocab, weights)
    try:
        assert b.rc == 0
        first, want = b.check(patterns, RANDOM_LIMIT)
        assert (want[2] > RANDOM_LIMIT).sum() >= 10 and (want[2] == 0).sum() >= 1 and (want[2] == 1).sum() >= 1
        first = b.run(patterns, RANDOM_LIMIT, keep_scratch=True)
        scratch1 = b.scratch.copy()
        again = b.run(patterns, RANDOM_LIMIT, keep_scratch=True)
        assert b"".join(x.tobytes() for x in again) == b"".join(x.tobytes() for x in first)
        assert scratch1.tobytes() == b.scratch.tobytes() and (scratch1 != 0x0BADBADBADBADBAD).all()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the ABI
def test_refusals_leave_the_outputs_untouched(hand_vocab):
    b, _ = hand_vocab
    lib, h = b.eng.lib, b.eng.handle
    p3 = ["a*", "*aus", "mensa"]

    def refused(code=MSR_ERR_INVALID, limit=3, **kw):
        outs = b.buffers(3, limit if 1 <= limit <= 16 else 3)
        assert b.call(p3, limit, outs, **kw) == code, kw
        for t, fill in zip(outs, FILLS):
            assert (t.cpu().numpy().view(np.uint32) == fill).all(), kw
    refused(n_patterns=-1)
    refused(n_patterns=_abi.MSR_WILD_MAX_PATTERNS + 1)
    refused(limit=0)
    refused(limit=_abi.MSR_WILD_MAX_LIMIT + 1)
    for pos in range(6):                                     # pat_off, pat_chars, the three outputs, the scratch
        refused(null=pos)
    need = int(lib.msr_wildcard_scratch_bytes(len(b.vocab), 3, 3))
    assert need == 3 * 1 * (3 * 8 + 4)
    refused(scratch_bytes=need - 1)
    assert "scratch" in lib.msr_last_error(h).decode()
    refused(misalign=True)
    assert lib.msr_wildcard_scratch_bytes(len(b.vocab), 0, 3) == 0
    assert lib.msr_wildcard_scratch_bytes(2 * S + 1, 5, 16) == 5 * 3 * (16 * 8 + 4)
    assert lib.msr_wildcard_scratch_bytes(2 * S + 1, 5, 16) == lib.msr_fuzzy_scratch_bytes(2 * S + 1, 5, 16)
    for bad in ((-1, 1, 1), (10, -1, 1), (10, 1025, 1), (10, 1, 0), (10, 1, 17)):
        assert lib.msr_wildcard_scratch_bytes(*bad) == -1
    # n_patterns == 0 succeeds, launches nothing, needs no pointer
    assert lib.msr_wildcard_terms(h, 0, None, None, 3, None, None, None, None, 0, b.eng._stream()) == 0
    b.check([], 3)                                           # ... through the helper too: nothing but the untouched padding
    b.check(p3, 3)                                           # and the engine still answers


def test_not_bound_without_a_vocabulary():
    b = Bound(["a", "ab"], [1, 1], bind=False)
    try:
        outs = b.buffers(1, 1)
        assert b.call(["a*"], 1, outs) == MSR_ERR_NOT_BOUND and b"msr_bind_vocab" in b.eng.lib.msr_last_error(b.eng.handle)
        assert all((t.cpu().numpy().view(np.uint32) == f).all() for t, f in zip(outs, FILLS))
        with pytest.raises(_abi.MsrError, match="vocabulary"):
            b.eng.wildcard_terms(["a*"])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the consumers
@pytest.fixture(scope="module")
def crawl():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix, qv = _crawl()
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    yield ix, qv, r
    r.engine.close()


def test_engine_and_bm25_wildcard_terms_against_the_oracle(crawl):
    from msretr.bm25 import BM25
    ix, qv, r = crawl
    eng = r.engine
    assert eng.has_vocab
    vocab = sorted(ix.vocab, key=ix.vocab.get)
    df = np.diff(np.asarray(ix.term_off)).tolist()
    patterns = ["uni*", "*bibliothek", "t?bingen", "wort00*", "wort?0?", "*", "", "a" * 33, "mensa", "zzz*", "*ö*z*", "w*1*9"]
    for limit in (1, 8):
        term, n, total = expected(vocab, df, patterns, limit)
        got = eng.wildcard_terms(patterns, limit=limit)
        assert got == [([int(term[i, c]) for c in range(int(n[i]))], int(total[i])) for i in range(len(patterns))]
    assert got[0] == ([ix.vocab["universität"]], 1) and got[3][1] == 10 and len(got[3][0]) == 8 and got[6] == got[7] == ([], 0)
    assert eng.wildcard_terms(["uni\U0001F600*", "uni*"], limit=2) == [([], 0), got[0]]       # not encodable: no lookup
    assert eng.wildcard_terms([]) == []
    with pytest.raises(ValueError):
        eng.wildcard_terms(["uni*"], limit=17)
    named = BM25(eng).wildcard_terms(["Uni*", "wort00*"], limit=3)
    assert named[0] == ([("universität", df[ix.vocab["universität"]])], 1)
    assert named[1][1] == 10 and [t for t, _ in named[1][0]] == [vocab[t] for t in eng.wildcard_terms(["wort00*"], limit=3)[0][0]]
    assert [d for _, d in named[1][0]] == sorted((d for _, d in named[1][0]), reverse=True)


def test_search_expands_the_pattern_and_only_when_asked(crawl):
    ix, qv, r = crawl
    kw = dict(query_embedding=qv[0])
    got = r.search("uni* mensa", wildcards=True, **kw)
    spelled = r.search("x", terms=["mensa", "tübingen", "universität"], **kw)             # typed terms, then the expansion
    assert spelled and list(got) == spelled                  # documents, order and scores, bit for bit
    assert got.expansions == {"uni*": {"terms": ["universität"], "total": 1}}
    assert got.corrections == {} and got.corrected_query is None
    # several expansions, in the lookup's order, cut at max_expansions
    order = [sorted(ix.vocab, key=ix.vocab.get)[t] for t in r.engine.wildcard_terms(["wort00*"], limit=16)[0][0]]
    assert len(order) == 10
    eight = r.search("mensa", patterns=["wort00*"], **kw)    # (a token with a digit is no pattern in the box: patterns=)
    assert eight.expansions == {"wort00*": {"terms": order[:8], "total": 10}}
    assert list(eight) == r.search("x", terms=["mensa", "tübingen"] + order[:8], **kw)
    assert r.search("wort00* mensa", wildcards=True, **kw).expansions == {}
    # max_expansions=1 against max_expansions=8
    en = [sorted(ix.vocab, key=ix.vocab.get)[t] for t in r.engine.wildcard_terms(["*en*"], limit=16)[0][0]]
    assert sorted(en) == ["mensa", "tübingen", "öffnungszeiten"]
    wide = r.search("*en* neckar", wildcards=True, max_expansions=8, **kw)
    one = r.search("*en* neckar", wildcards=True, max_expansions=1, **kw)
    assert wide.expansions == {"*en*": {"terms": en, "total": 3}} and one.expansions == {"*en*": {"terms": en[:1], "total": 3}}
    assert list(wide) == r.search("x", terms=["neckar", "tübingen"] + [t for t in en if t != "tübingen"], **kw)
    assert list(one) == r.search("x", terms=["neckar", "tübingen"] + [t for t in en[:1] if t != "tübingen"], **kw)
    assert list(one) != list(wide)
    # off: today's rows, a plain list; the tokenizer cuts `uni*` to the unknown word `uni`
    off = r.search("uni* mensa", **kw)
    assert off == r.search("uni* mensa", wildcards=False, **kw) == r.search("uni mensa", **kw) and type(off) is list
    assert off != list(got)
    # a query without any pattern under wildcards=True: the same rows
    plain = r.search("mensa öffnungszeiten", wildcards=True, **kw)
    assert list(plain) == r.search("mensa öffnungszeiten", **kw) and plain.expansions == {}
    # patterns= against the same pattern typed in the box
    given = r.search("mensa", patterns=["uni*"], **kw)
    assert list(given) == list(got) and given.expansions == got.expansions
    # a pattern of one literal is skipped, one that matches nothing adds nothing
    few = r.search("u* zzz* mensa", wildcards=True, **kw)
    assert list(few) == r.search("mensa", **kw)
    assert few.expansions == {"u*": {"terms": [], "total": 0, "skipped": True}, "zzz*": {"terms": [], "total": 0}}
    # hybrid mode takes the expanded ids in its lexical half
    hy = r.search("uni* mensa", wildcards=True, mode="hybrid", **kw)
    assert list(hy) == r.search("x", terms=["mensa", "tübingen", "universität"], mode="hybrid", **kw) and hy.expansions == got.expansions
    for bad in (0, 17, True, 2.5):
        with pytest.raises(ValueError, match="max_expansions"):
            r.search("uni* mensa", wildcards=True, max_expansions=bad, **kw)
    with pytest.raises(ValueError, match="required and excluded patterns"):
        r.search("+uni* mensa", wildcards=True, operators=True, **kw)


def test_fuzzy_and_wildcards_together_leave_the_pattern_alone(crawl):
    ix, qv, r = crawl
    kw = dict(query_embedding=qv[1])
    both = r.search("mesna uni*", fuzzy=True, wildcards=True, **kw)
    assert both.corrections == {"mesna": "mensa"} and both.expansions == {"uni*": {"terms": ["universität"], "total": 1}}
    assert list(both) == r.search("x", terms=["mensa", "tübingen", "universität"], **kw) and both
    # `mesn*` matches nothing and is NOT corrected to mensa
    alone = r.search("mesn* neckar", fuzzy=True, wildcards=True, **kw)
    assert alone.corrections == {} and alone.expansions == {"mesn*": {"terms": [], "total": 0}}
    assert list(alone) == r.search("neckar", **kw)


def test_batches_bm25_and_batch_lines(crawl):
    from msretr.bm25 import BM25
    ix, qv, r = crawl
    qs = ["uni* mensa", "mensa öffnungszeiten", "*bibliothek neckar", "t?bingen? schloss", "*en*"]
    got = r.search_batch(qs, query_embeddings=qv[:5], wildcards=True)
    for q in range(5):
        one = r.search(qs[q], query_embedding=qv[q], wildcards=True)
        assert list(got[q]) == list(one) and got[q].expansions == one.expansions
    assert [list(g.expansions) for g in got] == [["uni*"], [], ["*bibliothek"], ["t?bingen"], ["*en*"]]
    assert got[3].expansions["t?bingen"]["terms"] == ["tübingen"] and got[2].expansions["*bibliothek"]["terms"] == ["bibliothek"]
    # chunks of two queries: one lookup per chunk, the same answers
    calls, real = [], r.engine.wildcard_terms
    r.engine.wildcard_terms = lambda ps, limit=8: (calls.append(list(ps)), real(ps, limit=limit))[1]
    try:
        wc = {"patterns": [["uni*"], [], ["*bibliothek"], ["t?bingen", "uni*"], []], "limit": 8}
        ids = [ix.term_ids(t) for t in (["mensa"], ["mensa"], ["neckar"], ["schloss"], ["neckar"])]
        r.final_lists(ids, qv[:5], chunk=2, wildcards=wc)
    finally:
        del r.engine.wildcard_terms
    assert calls == [["uni*"], ["*bibliothek", "t?bingen", "uni*"]]          # none for the chunk without a pattern
    assert [list(e) for e in wc["expansions"]] == [["uni*"], [], ["*bibliothek"], ["t?bingen", "uni*"], []]
    lines = r.batch_search(list(zip("12345", qs)), query_embeddings=qv[:5], wildcards=True)
    assert lines.expansions == [g.expansions for g in got] and lines.corrections is None
    assert r.batch_search(list(zip("12", qs[:2])), query_embeddings=qv[:2]).expansions is None
    assert [(e["rank"], e["url"]) for e in lines] == [(row["rank"], row["url"]) for g in got for row in g]
    bm = BM25(r.engine)
    b_got = bm.search("uni* mensa", wildcards=True)
    assert b_got.expansions == {"uni*": {"terms": ["universität"], "total": 1}} and b_got
    assert list(b_got) == bm._finish(bm.search_terms(["mensa", "universität"]))
    assert bm.search("uni* mensa") == bm.search("uni mensa") and type(bm.search("uni* mensa")) is list
    assert list(bm.search("uni*", wildcards=True)) == bm._finish(bm.search_terms(["universität"]))


def test_snippets_see_the_expanded_terms(crawl):
    from msretr.index_build import bm25_index_from_tokens
    ix, qv, _ = crawl
    doc_ids = [int(d) for d in np.asarray(ix.doc_ids)]
    full = bm25_index_from_tokens(doc_ids, [t.split() for t in ix.texts], keep_tokens=True)
    for k in ("urls", "titles", "texts", "doc_off", "chunk_ids", "emb"):
        setattr(full, k, getattr(ix, k))
    r = Retriever(indexer=full, max_queries=8, max_k=1000)
    try:
        kw = dict(query_embedding=qv[2], snippets=True, snippet_tokens=8)
        got = r.search("uni*", wildcards=True, **kw)
        want = r.search("x", terms=["tübingen", "universität"], **kw)
        assert want and list(got) == want
        assert any("universität" in row["snippet"] and row["highlights"] for row in got)
        assert list(got) != r.search("uni*", **kw)           # without the expansion the windows look for the city alone
    finally:
        r.engine.close()


def test_an_index_without_term_strings_raises_and_a_sharded_engine_refuses(crawl):
    from msretr.bm25 import BM25
    from msretr.distributed import ShardedEngine
    ix, qv, r = crawl
    bare = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                      "total_docs", "doc_off", "chunk_ids", "emb", "urls", "titles", "texts")})
    rb = Retriever(indexer=bare, max_queries=8, max_k=1000)
    try:
        assert not rb.engine.has_vocab
        for kw in (dict(wildcards=True), dict(patterns=["uni*"])):
            with pytest.raises(ValueError, match="vocabulary"):
                rb.search("x", terms=[1, 2], query_embedding=qv[0], **kw)
        with pytest.raises(ValueError, match="vocabulary"):
            BM25(rb.engine).wildcard_terms(["uni*"])
    finally:
        rb.engine.close()
    with pytest.raises(ValueError, match="shard"):
        ShardedEngine(r.engine, 0, 0).search([[1, 2]], qv[:1], wildcards=True)


def test_http_search_with_wildcards(crawl):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, qv, r = crawl
    client = TestClient(create_app(r))
    body = {"query": "uni* mensa", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    wc = client.post("/api/search", json=dict(body, wildcards=True, max_expansions=4))
    assert plain.status_code == 200 and wc.status_code == 200
    want = r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", wildcards=True, max_expansions=4)
    assert wc.json()["documents"] == list(want) and want
    assert wc.json()["expansions"] == {"uni*": {"terms": ["universität"], "total": 1}} and "corrections" not in wc.json()
    assert "expansions" not in plain.json()
    assert plain.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1")
    given = client.post("/api/search", json=dict(body, query="mensa", patterns=["uni*"]))
    assert given.status_code == 200 and given.json()["documents"] == list(want)
    assert client.post("/api/search", json=dict(body, wildcards=True, max_expansions=17)).status_code == 400
    assert client.post("/api/search", json=dict(body, query="+uni* mensa", wildcards=True)).status_code == 400

"""Typo-tolerant lookup on the GPU (msr_bind_vocab / msr_fuzzy_terms, DeviceEngine.fuzzy_terms, the facades; DESIGN K15): the
kernels against the unfiltered plain-loop oracle of fuzzy_ref.py, all four outputs, exactly -- the hand vocabulary at every
tolerance and limit, every vocabulary size around the span a workgroup owns, every word count around the LDS word group, the
random case, determinism, padding; the ABI's refusals and bind-time checks; and the consumers on a small synthetic crawl."""
import ctypes as C

import numpy as np
import pytest
import torch

from fuzzy_ref import expected, hand, image, osa, pack_words, random_case
from msretr import _abi
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from msretr.retriever import Retriever
from msretr.text import preprocess_query, simple_tokenize

pytestmark = pytest.mark.gpu
PAD = 2                                                      # rows behind n_words that must keep the fill
FILLS = (0x5A5A5A5A, 0x3C3C3C3C, 0x77777777, 0x12345678)   # out_term, out_dist, out_n, out_total
MSR_ERR_INVALID, MSR_ERR_NOT_BOUND = -1, -2                # msretr.h
S, G = _abi.MSR_FUZZY_SPAN_TERMS, _abi.MSR_FUZZY_WORD_GROUP
RANDOM_LIMIT = 3


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _postings_only(n_terms):
    """An index of n_terms terms without term strings: every term once in document 0 (the lookup reads no posting)."""
    return CorpusIndex(doc_ids=np.arange(2, dtype=np.int64), doc_len=np.asarray([n_terms, 1], np.int32),
                       term_off=np.arange(n_terms + 1, dtype=np.int64), post_doc=np.zeros(n_terms, np.int32),
                       post_tf=np.ones(n_terms, np.int32), idf=np.ones(n_terms, np.float32), avgdl=float(n_terms + 1) / 2,
                       total_docs=2)


class Bound:
    """An engine over n_terms postings-only terms with a vocabulary image bound through the raw ABI."""

    def __init__(self, vocab, weights):
        self.vocab, self.weights = list(vocab), list(weights)
        self.eng = DeviceEngine(_postings_only(len(vocab)), max_queries=4, max_k=16, rerank_max_docs=0)
        assert not self.eng.has_vocab
        self.rc = self.bind(*image(vocab, weights))

    def bind(self, char_off, chars, weight, n_terms=None):
        dev = self.eng.device
        self.keep = (torch.from_numpy(np.asarray(char_off, np.int64)).to(dev),
                     torch.from_numpy(np.asarray(chars if len(chars) else [0], np.uint16).view(np.int16)).to(dev),
                     torch.from_numpy(np.asarray(weight, np.uint32).view(np.int32)).to(dev))
        return self.eng.lib.msr_bind_vocab(self.eng.handle, _P(self.keep[0]), _P(self.keep[1]), _P(self.keep[2]),
                                           len(char_off) - 1 if n_terms is None else n_terms, len(chars), self.eng._stream())

    def buffers(self, n, limit):
        dev = self.eng.device
        mk = lambda fill, size: torch.from_numpy(np.full(size, fill, np.uint32).view(np.int32)).to(dev)
        return [mk(FILLS[0], (n + PAD) * limit), mk(FILLS[1], (n + PAD) * limit), mk(FILLS[2], n + PAD), mk(FILLS[3], n + PAD)]

    def call(self, words, maxes, limit, outs, n_words=None, scratch_bytes=None, null=None, no_scratch=False):
        """One raw msr_fuzzy_terms call -> rc.  null: the position of a pointer argument to pass as NULL."""
        dev, n = self.eng.device, len(words)
        off, chars = pack_words(words)
        d_off = torch.from_numpy(off).to(dev)
        d_chars = torch.from_numpy(np.asarray(chars if len(chars) else [0], np.uint16).view(np.int16)).to(dev)
        d_max = torch.from_numpy(np.asarray(maxes if n else [0], np.int32)).to(dev)
        need = int(self.eng.lib.msr_fuzzy_scratch_bytes(len(self.vocab), max(n, 0), limit))
        scratch = torch.full((max(need, 8) // 8 + 1,), 0x0BADBADBADBADBAD, dtype=torch.int64, device=dev)
        ptrs = [_P(d_off), _P(d_chars), _P(d_max)] + [_P(t) for t in outs] + [C.c_void_p(0) if no_scratch else _P(scratch)]
        if null is not None:
            ptrs[null] = C.c_void_p(0)
        rc = self.eng.lib.msr_fuzzy_terms(self.eng.handle, n if n_words is None else n_words, ptrs[0], ptrs[1], ptrs[2], limit,
                                          ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7],
                                          need if scratch_bytes is None else scratch_bytes, self.eng._stream())
        torch.cuda.synchronize(dev)
        return rc

    def run(self, words, maxes, limit):
        """-> the four host arrays, padding included, of one call into pre-filled buffers."""
        outs = self.buffers(len(words), limit)
        rc = self.call(words, maxes, limit, outs)
        assert rc == 0, self.eng.lib.msr_last_error(self.eng.handle)
        return [t.cpu().numpy() for t in outs]

    def check(self, words, maxes, limit, want=None):
        got = self.run(words, maxes, limit)
        n = len(words)
        want = expected(self.vocab, self.weights, words, maxes, limit) if want is None else want
        for x, fill, size in zip(got, FILLS, (n * limit, n * limit, n, n)):
            assert (x[size:].view(np.uint32) == fill).all(), "rows at or above n_words were touched"
        for name, x, w in zip(("term", "dist", "n", "total"), got, want):
            x = x[:w.size].reshape(w.shape)
            bad = np.argwhere(x != w)
            assert len(bad) == 0, (name, bad[:5].tolist(), [(words[int(b[0])], maxes[int(b[0])]) for b in bad[:5]],
                                   x[bad[0][0]].tolist(), w[bad[0][0]].tolist())
        return got, want

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def hand_vocab():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    vocab, weights, words = hand()
    b = Bound(vocab, weights)
    assert b.rc == 0
    yield b, words
    b.close()


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("limit", [1, 3, 16])
def test_hand_vocabulary_every_tolerance(hand_vocab, limit):
    b, words = hand_vocab
    assert {len(s) for s in b.vocab} >= {1, 2, 31, 32, 33} and {len(w) for w in words} >= {0, 1, 2, 3, 32, 33}
    assert b.weights[b.vocab.index("geist")] == 0 and "geist" in words and b.weights[[len(s) for s in b.vocab].index(33)] == 0
    for m in (0, 1, 2, 3):
        b.check(words, [m] * len(words), limit)
    mixed = [(3 * i + 1) % 4 for i in range(len(words))]     # 0, 1, 2 and 3 mixed in one call
    assert set(mixed) == {0, 1, 2, 3}
    got, want = b.check(words, mixed, limit)
    both = b.check(words + words, [2] * len(words) + [1] * len(words), limit)[1]
    assert both[3].max() > limit or limit == 16             # rows cut at the limit are among them
    assert (both[3] == 0).any() and ((both[3] > 0) & (both[3] <= limit)).any()
    # a word alone gives what it gives inside the call
    for i in (0, 5, 7, len(words) - 2):
        b.check(words[i:i + 1], [2], limit)


def test_tolerances_the_kernel_itself_refuses(hand_vocab):
    b, words = hand_vocab
    got, _ = b.check(["mensa", "mensa", "mensa", "mensa"], [-1, 3, 7, 1], 3)
    assert got[3][:4].tolist() == [0, 0, 0, 5] and got[0][:9].tolist() == [-1] * 9


def _span_vocab(n_terms, rng):
    """n_terms distinct terms: digits far from every word, with neighbours of "mensa" planted at the first and last term of
    every span, and a cluster of them behind the first term."""
    near = ["mensa", "mensb", "mensc", "mensd", "mense", "mesna", "mnesa", "ensa", "mensaa", "xmensa", "menssa", "mfnsa",
            "mensf", "mensg", "emnsa", "mensh"]
    assert all(osa("mensa", s) <= 1 for s in near) and len(set(near)) == len(near)
    vocab = [f"{i:08d}" for i in range(n_terms)]
    spots = [p for p in (0, 1, 2, 3, 4, 5, S - 1, S, S + 5, 2 * S - 1, 2 * S, n_terms - 1) if 0 <= p < n_terms]
    for k, p in enumerate(dict.fromkeys(spots)):
        vocab[p] = near[k]
    weights = [int(v) for v in rng.choice([1, 2, 2, 9], n_terms)]
    return vocab, weights


@pytest.mark.parametrize("n_terms", [1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1])
def test_vocabulary_sizes_around_a_span(n_terms):
    vocab, weights = _span_vocab(n_terms, np.random.default_rng(n_terms))
    b = Bound(vocab, weights)
    try:
        assert b.rc == 0
        words, maxes = ["mensa", "mesna", "00000000", f"{n_terms - 1:08d}"[:7], "qqqq"], [1, 2, 0, 1, 2]
        for limit in (1, 2, 3, 16):
            _, want = b.check(words, maxes, limit)
        per_span = np.bincount([t // S for t, s in enumerate(vocab) if osa("mensa", s) <= 1], minlength=1)
        if n_terms >= 6:
            assert per_span[0] > 3                           # more than `limit` candidates inside one span (limits 1 .. 3)
        if n_terms == 2 * S + 1:
            assert (per_span > 0).sum() == 3 and want[3][0] == per_span.sum() > 3      # one in each of more than `limit` spans
            first = b.check(["mensa"], [0], 1)[1]
            assert first[0].tolist() == [[0]]                # the first term of the first span ...
            last = b.check([vocab[-1]], [0], 1)[1]
            assert last[0].tolist() == [[n_terms - 1]]       # ... and the only term of the last
        for p in (S - 1, S, 2 * S - 1, 2 * S):               # the terms at a span's edges are found by their own spelling
            if p < n_terms:
                assert b.check([vocab[p]], [0], 1)[1][0].tolist() == [[p]]
    finally:
        b.close()


@pytest.mark.parametrize("n_words", [0, 1, G - 1, G, G + 1, _abi.MSR_FUZZY_MAX_WORDS])
def test_word_counts_around_the_word_group(hand_vocab, n_words):
    b, words = hand_vocab
    short = [w for w in words if 0 < len(w) <= 5]
    pick = [short[(5 * i + i // 7) % len(short)] for i in range(n_words)]
    got, want = b.check(pick, [(i % 3) for i in range(n_words)], 2)          # n_words == 0: nothing but the untouched padding
    if n_words >= G:
        assert (want[3] > 2).any() and (want[3] == 0).any()


def test_random_case_all_four_outputs_and_the_same_bytes_twice():
    vocab, weights, words, maxes = random_case()
    b = Bound(vocab, weights)
    try:
        assert b.rc == 0
        first, want = b.check(words, maxes, RANDOM_LIMIT)
        assert (want[3] > RANDOM_LIMIT).sum() >= 10 and (want[3] == 0).sum() >= 5
        again = b.run(words, maxes, RANDOM_LIMIT)
        assert b"".join(x.tobytes() for x in again) == b"".join(x.tobytes() for x in first)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the ABI
def test_refusals_leave_the_outputs_untouched(hand_vocab):
    b, words = hand_vocab
    lib, h = b.eng.lib, b.eng.handle
    w3, m3 = ["mensa", "kaus", "ab"], [1, 1, 1]

    def refused(code=MSR_ERR_INVALID, limit=3, **kw):
        outs = b.buffers(3, limit if 1 <= limit <= 16 else 3)
        assert b.call(w3, m3, limit, outs, **kw) == code, kw
        for t, fill in zip(outs, FILLS):
            assert (t.cpu().numpy().view(np.uint32) == fill).all(), kw
    refused(n_words=-1)
    refused(n_words=_abi.MSR_FUZZY_MAX_WORDS + 1)
    refused(limit=0)
    refused(limit=_abi.MSR_FUZZY_MAX_LIMIT + 1)
    for pos in range(7):                                     # word_off, word_chars, word_max, the four outputs
        refused(null=pos)
    refused(no_scratch=True)
    need = int(lib.msr_fuzzy_scratch_bytes(len(b.vocab), 3, 3))
    assert need == 3 * 1 * (3 * 8 + 4)
    refused(scratch_bytes=need - 1)
    assert "scratch" in lib.msr_last_error(h).decode()
    assert lib.msr_fuzzy_scratch_bytes(len(b.vocab), 0, 3) == 0
    assert lib.msr_fuzzy_scratch_bytes(2 * S + 1, 5, 16) == 5 * 3 * (16 * 8 + 4)
    for bad in ((-1, 1, 1), (10, -1, 1), (10, 1025, 1), (10, 1, 0), (10, 1, 17)):
        assert lib.msr_fuzzy_scratch_bytes(*bad) == -1
    # n_words == 0 succeeds, launches nothing, needs no pointer
    assert lib.msr_fuzzy_terms(h, 0, None, None, None, 3, None, None, None, None, None, 0, b.eng._stream()) == 0
    b.check(w3, m3, 3)                                       # and the engine still answers


def test_binding_its_checks_and_what_drops_it():
    vocab, weights, words = hand()
    b = Bound(vocab[:5], weights[:5])
    try:
        lib, h = b.eng.lib, b.eng.handle
        assert b.rc == 0
        owned = b.eng.owned_bytes()
        char_off, chars, weight = image(b.vocab, b.weights)
        outs = b.buffers(1, 1)

        def not_bound():
            assert b.call(["ab"], [1], 1, outs) == MSR_ERR_NOT_BOUND
            assert all((t.cpu().numpy().view(np.uint32) == f).all() for t, f in zip(outs, FILLS))
        # every bind-time check, each leaving no vocabulary bound
        down = char_off.copy(); down[2] = down[1] - 1
        shifted = char_off.copy(); shifted[0] = 1
        short_ = char_off.copy(); short_[-1] -= 1
        heavy = weight.copy(); heavy[3] = 2 ** 31
        for args, why in (((down, chars, weight), "descends"), ((shifted, chars, weight), "from 0"),
                          ((short_, chars, weight), "from 0"), ((char_off, chars, heavy), "2^31"),
                          ((char_off[:-1], chars[:int(char_off[-2])], weight[:-1]), "differs")):
            assert b.bind(*args) == MSR_ERR_INVALID and why in lib.msr_last_error(h).decode(), why
            not_bound()
            assert b.eng.owned_bytes() == owned - 8 * 5     # the signature table went with the binding
            assert b.bind(char_off, chars, weight) == 0 and b.eng.owned_bytes() == owned
        assert b.bind(char_off, chars, weight, n_terms=6) == MSR_ERR_INVALID
        assert b.bind(char_off, chars, weight) == 0
        full = weight.copy(); full[3] = 2 ** 31 - 1          # the largest weight wins among equals
        assert b.bind(char_off, chars, full) == 0
        b.vocab, b.weights = b.vocab, full.tolist()
        b.check(["a" * 32], [1], 2)
        # msr_unbind drops it and what the engine derived
        assert lib.msr_unbind(h) == 0
        not_bound()
        assert b.bind(char_off, chars, weight) == MSR_ERR_NOT_BOUND          # no postings
    finally:
        b.close()


def test_not_bound_before_bind_vocab_and_after_new_postings():
    eng = DeviceEngine(_postings_only(5), max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        with pytest.raises(_abi.MsrError, match="vocabulary"):
            eng.fuzzy_terms(["mensa"])
        outs = [torch.zeros(4, dtype=torch.int32, device=eng.device) for _ in range(4)]
        scratch = torch.zeros(64, dtype=torch.int64, device=eng.device)
        one = torch.zeros(4, dtype=torch.int32, device=eng.device)
        rc = eng.lib.msr_fuzzy_terms(eng.handle, 1, _P(one), _P(one), _P(one), 1, *[_P(t) for t in outs], _P(scratch), 512,
                                     eng._stream())
        assert rc == MSR_ERR_NOT_BOUND and b"msr_bind_vocab" in eng.lib.msr_last_error(eng.handle)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the consumers
WORDS = ["mensa", "öffnungszeiten", "bibliothek", "universität", "schloss", "neckar", "tübingen"]


def _crawl(n_docs=240, seed=11):
    """A small synthetic crawl: pages of 10 .. 60 words, the WORDS each in about a fifth of them, with chunks and texts."""
    from msretr.index_build import bm25_index_from_tokens
    rng = np.random.default_rng(seed)
    filler = [f"wort{i:03d}" for i in range(150)]
    doc_ids = (np.arange(n_docs) * 3 + 50).tolist()
    tokens = []
    for d in range(n_docs):
        toks = [filler[j] for j in rng.integers(0, len(filler), int(rng.integers(10, 61)))]
        toks += [w for w in WORDS if rng.random() < 0.2]
        toks += ["tübingen"] * int(rng.random() < 0.6)
        tokens.append([toks[j] for j in rng.permutation(len(toks))])
    ix = bm25_index_from_tokens(doc_ids, tokens)
    ix.urls = [f"https://www.site{d % 17}.de/page/{d}" for d in doc_ids]
    ix.titles = [f"Seite {d}" for d in doc_ids]
    ix.texts = [" ".join(t) for t in tokens]
    cnt = 1 + np.arange(n_docs) % 3
    ix.doc_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    n_chunks = int(cnt.sum())
    ix.chunk_ids = np.arange(n_chunks, dtype=np.int64)
    emb = rng.standard_normal((n_chunks, 768)).astype(np.float32)
    ix.emb = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    qv = rng.standard_normal((8, 768)).astype(np.float32)
    return ix, qv


@pytest.fixture(scope="module")
def crawl():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix, qv = _crawl()
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    yield ix, qv, r
    r.engine.close()


def test_engine_and_bm25_fuzzy_terms_against_the_oracle(crawl):
    from msretr.bm25 import BM25
    from msretr.fuzzy import auto_edits
    ix, qv, r = crawl
    eng = r.engine
    assert eng.has_vocab
    vocab = sorted(ix.vocab, key=ix.vocab.get)
    df = np.diff(np.asarray(ix.term_off)).tolist()
    words = ["mesna", "bibliotek", "mensa", "offnungszeiten", "wort01", "xy", "", "a" * 33, "zzzzzzzz", "schlos", "neckra"]
    auto = [auto_edits(len(w)) for w in words]
    for limit in (1, 5):
        term, dist, n, total = expected(vocab, df, words, auto, limit)
        got = eng.fuzzy_terms(words, limit=limit)
        assert got == [([(int(term[i, c]), int(dist[i, c])) for c in range(int(n[i]))], int(total[i])) for i in range(len(words))]
    assert got[0][0][0] == (ix.vocab["mensa"], 1) and got[2][0][0] == (ix.vocab["mensa"], 0) and got[6] == got[7] == ([], 0)
    assert got[4][1] > 5                                     # "wort01": ten fillers one edit away
    fixed = eng.fuzzy_terms(words, max_edits=2, limit=16)
    t2 = expected(vocab, df, words, [2] * len(words), 16)
    assert [tot for _, tot in fixed] == t2[3].tolist()
    with pytest.raises(ValueError):
        eng.fuzzy_terms(["mensa"], limit=17)
    with pytest.raises(ValueError):
        eng.fuzzy_terms(["mensa"], max_edits=3)
    near = BM25(eng).fuzzy_terms(["mesna", "bibliotek"], limit=3)
    assert near[0][0] == ("mensa", 1, df[ix.vocab["mensa"]]) and near[1][0] == ("bibliothek", 1, df[ix.vocab["bibliothek"]])


def test_search_corrects_the_typo_and_only_when_asked(crawl):
    ix, qv, r = crawl
    kw = dict(query_embedding=qv[0])
    right = r.search("mensa öffnungszeiten", **kw)
    got = r.search("mesna öffnungszeiten", fuzzy=True, **kw)
    assert right and list(got) == right                      # documents, ranks, scores: the rows of the correct spelling
    assert got.corrections == {"mesna": "mensa"}
    assert got.corrected_query == preprocess_query("mesna öffnungszeiten").replace("mesna", "mensa")
    # off: what the parent commit returns, the rows of the known word alone, a plain list
    off = r.search("mesna öffnungszeiten", **kw)
    assert off == r.search("öffnungszeiten", **kw) and off != right and type(off) is list
    assert r.search("mesna öffnungszeiten", fuzzy=False, **kw) == off
    # a clean query: nothing replaced, the same rows
    clean = r.search("mensa öffnungszeiten", fuzzy=True, **kw)
    assert list(clean) == right and clean.corrections == {} and clean.corrected_query is None
    # a word nothing is near stays dropped
    far = r.search("qqqqqqqq öffnungszeiten", fuzzy=True, **kw)
    assert list(far) == off and far.corrections == {}
    # hybrid mode corrects the lexical stage the same way
    hy = r.search("mesna öffnungszeiten", fuzzy=True, mode="hybrid", **kw)
    assert list(hy) == r.search("mensa öffnungszeiten", mode="hybrid", **kw) and hy.corrections == {"mesna": "mensa"}


def test_must_is_corrected_must_not_and_phrases_are_not(crawl):
    ix, qv, r = crawl
    kw = dict(query_embedding=qv[1])
    want = r.search("öffnungszeiten", must=["mensa"], **kw)
    got = r.search("öffnungszeiten", must=["mesna"], fuzzy=True, **kw)
    assert want and list(got) == want and got.corrections == {"mesna": "mensa"}
    assert r.search("öffnungszeiten", must=["mesna"], **kw) == []                 # off: an unknown required word finds nothing
    op = r.search("öffnungszeiten +mesna", operators=True, fuzzy=True, **kw)
    assert list(op) == r.search("öffnungszeiten +mensa", operators=True, **kw) and op.corrections == {"mesna": "mensa"}
    # an excluded typo excludes nothing
    x = r.search("öffnungszeiten", must_not=["mesna"], fuzzy=True, **kw)
    assert list(x) == r.search("öffnungszeiten", **kw) and x.corrections == {}
    assert list(x) != r.search("öffnungszeiten", must_not=["mensa"], **kw)
    # BM25.search: the same policy
    from msretr.bm25 import BM25
    bm = BM25(r.engine)
    b_got = bm.search("mesna öffnungszeiten", fuzzy=True)
    assert list(b_got) == bm.search("mensa öffnungszeiten") and b_got.corrections == {"mesna": "mensa"}
    assert bm.search("mesna öffnungszeiten") == bm.search("öffnungszeiten")


def test_search_batch_of_clean_and_misspelt_queries(crawl):
    ix, qv, r = crawl
    qs = ["mensa öffnungszeiten", "mesna öffnungszeiten", "bibliotek neckar", "schloss", "univeristät neckra"]
    got = r.search_batch(qs, query_embeddings=qv[:5], fuzzy=True)
    for q in range(5):
        one = r.search(qs[q], query_embedding=qv[q], fuzzy=True)
        assert list(got[q]) == list(one) and got[q].corrections == one.corrections
        assert got[q].corrected_query == one.corrected_query
    assert [g.corrections for g in got] == [{}, {"mesna": "mensa"}, {"bibliotek": "bibliothek"}, {},
                                            {"univeristät": "universität", "neckra": "neckar"}]
    pair = r.search_batch(qs[:2], query_embeddings=qv[[0, 0]], fuzzy=True)     # one vector: the typo's rows are the clean query's
    assert list(pair[1]) == list(pair[0]) and pair[0]
    # chunks of two queries: one lookup per chunk, the same answers
    doc, score, _, n = r.final_lists([ix.term_ids(simple_tokenize(preprocess_query(q))) for q in qs], qv[:5], chunk=2,
                                     fuzzy={"terms": [simple_tokenize(preprocess_query(q)) for q in qs]})
    whole = r.search_batch(qs, query_embeddings=qv[:5], fuzzy=True)
    assert [int(v) for v in n] == [len(w) for w in whole]
    lines = r.batch_search(list(zip("12345", qs)), query_embeddings=qv[:5], fuzzy=True)
    assert lines.corrections == [g.corrections for g in got] and lines.corrected_queries[0] is None
    assert lines.text() == r.batch_search(list(zip("12345", [q.replace("mesna", "mensa").replace("bibliotek", "bibliothek")
                                                             .replace("univeristät", "universität").replace("neckra", "neckar")
                                                             for q in qs])), query_embeddings=qv[:5]).text()


def test_a_grown_and_a_shrunk_vocabulary_are_served(crawl):
    from msretr.chunk_index import ChunkTable, attach_chunks
    from msretr.index_build import bm25_add_token_ids, remove_documents
    ix, qv, _ = crawl
    r = Retriever(indexer=DeviceEngine(ix, max_queries=8, max_k=1000))
    try:
        kw = dict(query_embedding=qv[2])
        assert r.search("stocherkhan", fuzzy=True, **kw).corrections == {}
        # a new page brings a new word
        vocab = dict(ix.vocab)
        new_t = vocab["stocherkahn"] = ix.n_terms
        toks = np.asarray([new_t, vocab["neckar"], new_t, vocab["tübingen"]], np.int32)
        grown = bm25_add_token_ids(ix, [9001], np.asarray([0, 4], np.int64), toks, ix.n_terms + 1, vocab=vocab,
                                   docs_meta={9001: ("https://www.site1.de/page/9001", "Kahn", "stocherkahn neckar stocherkahn")})
        e = np.zeros((1, 768), np.float32); e[0, 3] = 1.0
        grown = attach_chunks(grown, ChunkTable(chunk_ids=np.asarray([10 ** 6], np.int64), doc_ids=np.asarray([9001], np.int64),
                                                seqs=[[1]], emb=torch.as_tensor(e)))
        r.update_index(grown)
        got = r.search("stocherkhan", fuzzy=True, **kw)
        assert got.corrections == {"stocherkhan": "stocherkahn"} and list(got) == r.search("stocherkahn", **kw)
        assert "9001" in [row["doc_id"] for row in got]
        assert r.search("mesna", fuzzy=True, **kw).corrections == {"mesna": "mensa"}          # the old words, the new weights
        # its only page goes: the word stays in the vocabulary with an empty posting list and is not suggested
        shrunk = remove_documents(grown, [9001])
        assert "stocherkahn" in shrunk.vocab
        r.update_index(shrunk)
        gone = r.search("stocherkhan", fuzzy=True, **kw)
        assert gone.corrections == {} and list(gone) == r.search("qqqqqqqq", **kw)
        assert r.engine.fuzzy_terms(["stocherkahn"], limit=3) == [([], 0)]
    finally:
        r.engine.close()


def test_http_search_with_fuzzy(crawl):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, qv, r = crawl
    client = TestClient(create_app(r))
    body = {"query": "mesna öffnungszeiten", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    fz = client.post("/api/search", json=dict(body, fuzzy=True))
    assert plain.status_code == 200 and fz.status_code == 200
    want = r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", fuzzy=True)
    assert fz.json()["documents"] == list(want) and want
    assert fz.json()["corrected_query"] == want.corrected_query and "mensa" in want.corrected_query
    assert fz.json()["corrections"] == {"mesna": "mensa"}
    assert "corrected_query" not in plain.json()
    assert plain.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1")
    # an index without term strings: 400
    bare = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                      "total_docs", "doc_off", "chunk_ids", "emb", "urls", "titles", "texts")})
    rb = Retriever(indexer=bare, max_queries=8, max_k=1000)
    try:
        assert not rb.engine.has_vocab
        with pytest.raises(ValueError, match="vocabulary"):
            rb.search("x", terms=[1, 2], query_embedding=qv[0], fuzzy=True)
        resp = TestClient(create_app(rb)).post("/api/search", json=dict(body, terms=["1"], fuzzy=True))
        assert resp.status_code == 400 and "vocabulary" in resp.json()["error"]
    finally:
        rb.engine.close()


def test_a_sharded_engine_refuses(crawl):
    from msretr.distributed import ShardedEngine
    ix, qv, r = crawl
    sh = ShardedEngine(r.engine, 0, 0)
    with pytest.raises(ValueError, match="shard"):
        sh.search([[1, 2]], qv[:1], fuzzy=True)

"""Phrase search on the CPU: the oracle of phrase_ref.py against an independent formulation (documents rendered as strings) on
every case, text.parse_phrases on a table of inputs, and the forward index's bookkeeping through build, add, remove, save /
load, attach_tokens and tokens_from_texts (all on device="cpu")."""
import numpy as np
import pytest

from msretr.index import CorpusIndex, _np
from msretr.index_build import (attach_tokens, bm25_add_token_ids, bm25_index_from_token_ids, bm25_index_from_tokens,
                                remove_documents, tokens_from_texts)
from msretr.text import parse_operators, parse_phrases, simple_tokenize
from phrase_ref import (A, B, BIG, F, N_TERMS, SIZES, X, Y, cand_mask, combine_mask, corpus, expected, phrase_mask_fast,
                        random_rows)

VARIANTS = [(N, False) for N in SIZES] + [(33, True), (1025, True)]


_RENDERED = {}


def _rendered(c):
    """Every document as " t0 t1 ... " (rendered once per corpus)."""
    if id(c) not in _RENDERED:
        tok = [str(t) for t in c.tok_ids.tolist()]
        _RENDERED[id(c)] = (c, [" " + " ".join(tok[c.tok_off[d]:c.tok_off[d + 1]]) + " " for d in range(c.n_docs)])
    return _RENDERED[id(c)][1]


def _string_mask(c, phrase, cand):
    """The independent formulation: document d rendered as " t0 t1 ... " holds the phrase padded by spaces."""
    N, text = c.n_docs, _rendered(c)
    out = np.zeros(N, bool)
    if not 1 <= len(phrase) <= 16 or any(not 0 <= t < N_TERMS for t in phrase):
        return out
    needle = " " + " ".join(str(int(t)) for t in phrase) + " "
    for d in range(N):
        if cand is None or cand[d]:
            out[d] = needle in text[d]
    return out


@pytest.mark.parametrize("N,empty_ends", VARIANTS)
def test_oracle_against_the_string_formulation(N, empty_ends):
    c = corpus(N, empty_ends)
    cases, want = expected(N, empty_ends)
    assert len(cases) >= (20 if N == 1 else 60)
    n_hit = 0
    for r, w in zip(cases, want):
        cm = cand_mask(c, r.cand)
        assert (w == _string_mask(c, r.phrase, cm)).all(), (N, r.claim)
        assert (w == phrase_mask_fast(c.tok_off, c.tok_ids, r.phrase, cm)).all(), (N, r.claim)
        n_hit += bool(w.any())
    assert n_hit >= (3 if N == 1 else 25)                    # the cases hold matching rows and empty ones
    assert len(c.tok_ids) < 400_000
    for r in random_rows(c, 40, seed=N):
        cm = cand_mask(c, r.cand)
        assert (phrase_mask_fast(c.tok_off, c.tok_ids, r.phrase, cm) == _string_mask(c, r.phrase, cm)).all(), r.claim


def test_the_claims_hold_on_the_big_corpus():
    c = corpus(BIG)
    cases, want = expected(BIG)
    by = {r.claim: w for r, w in zip(cases, want)}
    d = c.doc
    lens = np.diff(c.tok_off)
    assert [int(lens[d[n]]) for n in ("len63", "p62_2", "p63_2", "p62_3", "p64_2", "len4097", "len10000")] == \
        [63, 64, 65, 128, 129, 4097, 10000]
    assert lens[d["empty_5"]] == 0 and int(c.tok_ids[-1]) == X
    assert not by["present only across document boundaries (bound_a | bound_b, last | nothing): no match"].any()
    assert not by["L = 17: the ABI gives an empty row (the document l17 holds it)"].any()
    assert by["L = 16"].nonzero()[0].tolist() == sorted([d["l16"], d["l17"]])
    assert by["repeated term: P P in Q P P"].nonzero()[0].tolist() == [d["repeat"]]
    assert by["overlap: P Q P in P Q P Q P"].nonzero()[0].tolist() == [d["overlap"]]
    assert by["a prefix match, a mismatch, then the real match later"].nonzero()[0].tolist() == [d["late"]]
    assert not by["prefix matches only"].any()
    for at in (62, 63, 64):
        assert by[f"two terms starting at stream position {at}"].nonzero()[0].tolist() == [d[f"p{at}_2"]]
        assert by[f"three terms starting at stream position {at}"].nonzero()[0].tolist() == [d[f"p{at}_3"]]
    assert by["10 000 tokens: the only occurrence on the last two tokens"].nonzero()[0].tolist() == [d["len10000"]]
    edge = by["candidate documents at bits 0, 31, 32, 1023, 1024, S - 1, S, N - 1"].nonzero()[0].tolist()
    assert edge == [0, 31, 32, 1023, 1024, 8191, 8192, BIG - 1]
    e = corpus(33, True)
    assert np.diff(e.tok_off)[[0, 32]].tolist() == [0, 0]


def test_combine_mask():
    rng = np.random.default_rng(1)
    N = 70
    m = [rng.random(N) < 0.5 for _ in range(4)]
    assert combine_mask(m, [], [], N).all()
    assert (combine_mask(m, [0, 1], [2], N) == (m[0] & m[1] & ~m[2])).all()
    assert not combine_mask(m, [0, 4], [], N).any() and not combine_mask(m, [-1], [], N).any()
    assert (combine_mask(m, [3], [-1, 4, 9], N) == m[3]).all()
    assert (combine_mask(m, [], [0, 1], N) == ~(m[0] | m[1])).all()


PARSE = [
    ('"max planck" tübingen', ("max planck tübingen", ["max planck"], [])),
    ('mensa -"max planck" heute', ("mensa heute", [], ["max planck"])),
    ('a "b c" d "e f"', ("a b c d e f", ["b c", "e f"], [])),
    ('x "unbalanced y', ('x "unbalanced y', [], [])),
    ('"a b" "c', ('a b "c', ["a b"], [])),
    ('"" a', ("a", [], [])),
    ('-"" a " "', ("a", [], [])),
    ('+"a b" -w +z', ("a b -w +z", ["a b"], [])),
    ('-w -"a b" +z', ("-w +z", [], ["a b"])),
    ('uni-"x y"', ("uni- x y", ["x y"], [])),
    ("no quotes -here +there", ("no quotes -here +there", [], [])),
    ('"single"', ("single", ["single"], [])),
    ("", ("", [], [])),
]


@pytest.mark.parametrize("text,want", PARSE)
def test_parse_phrases(text, want):
    assert parse_phrases(text) == want


def test_parse_phrases_then_operators():
    text, mp, xp = parse_phrases('mensa "max planck" -"old town" +ring -bus')
    assert (text, mp, xp) == ("mensa max planck +ring -bus", ["max planck"], ["old town"])
    assert parse_operators(text) == ("mensa max planck ring", ["ring"], ["bus"])


# ------------------------------------------------------------------------------------------------ the forward index
def _streams(n, seed, n_terms=30, empty=()):
    rng = np.random.default_rng(seed)
    s = [rng.integers(0, n_terms, int(rng.integers(1, 12))).tolist() for _ in range(n)]
    for i in empty:
        s[i] = []
    return s


def _csr(streams):
    off = np.zeros(len(streams) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    return off, np.asarray([t for s in streams for t in s], np.int32)


def _fwd(ix):
    return _np(ix.tok_off).tolist(), _np(ix.tok_ids).tolist()


def test_keep_tokens_stores_the_kept_documents_in_doc_id_order():
    ids = np.array([40, 10, 30, 20, 50], np.int64)
    streams = _streams(5, 1, empty=(2,))                     # doc_id 30 has no tokens: dropped
    off, tok = _csr(streams)
    ix = bm25_index_from_token_ids(ids, off, tok, 30, keep_tokens=True)
    assert _np(ix.doc_ids).tolist() == [10, 20, 40, 50]
    want = [streams[1], streams[3], streams[0], streams[4]]
    assert _fwd(ix) == tuple(x.tolist() for x in _csr(want))
    assert _np(ix.tok_off).dtype == np.int64 and _np(ix.tok_ids).dtype == np.int32
    assert (np.diff(_np(ix.tok_off)) == _np(ix.doc_len)).all()
    plain = bm25_index_from_token_ids(ids, off, tok, 30)
    assert plain.tok_off is None and plain.tok_ids is None
    for name in ("term_off", "post_doc", "post_tf", "idf", "doc_len"):
        assert _np(getattr(plain, name)).tobytes() == _np(getattr(ix, name)).tobytes()
    # the string builder
    words = [[f"w{t}" for t in s] for s in streams]
    sx = bm25_index_from_tokens(ids, words, keep_tokens=True)
    assert bm25_index_from_tokens(ids, words).tok_off is None
    inv = {v: k for k, v in sx.vocab.items()}
    got = [[inv[t] for t in sx.tok_ids[sx.tok_off[i]:sx.tok_off[i + 1]]] for i in range(sx.n_docs)]
    assert got == [words[1], words[3], words[0], words[4]]


def test_add_then_remove_equals_a_build_of_the_final_documents():
    base_ids = np.array([10, 20, 30, 40, 50, 60], np.int64)
    base = _streams(6, 2)
    add_ids = np.array([70, 15, 35, 20, 5, 80], np.int64)    # appended, interleaved, one already indexed (20: skipped), 80 empty
    add = _streams(6, 3, empty=(5,))
    ix = bm25_index_from_token_ids(base_ids, *_csr(base), 30, keep_tokens=True)
    ix2 = bm25_add_token_ids(ix, add_ids, *_csr(add), 30)
    assert ix2.update_counts["added"] == 4 and ix2.update_counts["already_indexed"] == 1
    final = {int(d): s for d, s in zip(base_ids, base)}
    final.update({int(d): s for d, s in zip(add_ids, add) if int(d) != 20 and s})
    ids = sorted(final)
    scratch = bm25_index_from_token_ids(np.asarray(ids), *_csr([final[d] for d in ids]), 30, keep_tokens=True)
    assert _np(ix2.doc_ids).tolist() == ids and _fwd(ix2) == _fwd(scratch)
    # remove, then a replace: the same doc_id comes back with a new stream
    ix3 = remove_documents(ix2, [30, 15, 999])
    new30 = [1, 2, 3, 4]
    ix4 = bm25_add_token_ids(ix3, np.array([30]), *_csr([new30]), 30)
    for d in (30, 15):
        final.pop(d)
    ids3 = sorted(final)
    assert _fwd(ix3) == _fwd(bm25_index_from_token_ids(np.asarray(ids3), *_csr([final[d] for d in ids3]), 30, keep_tokens=True))
    final[30] = new30
    ids4 = sorted(final)
    scratch4 = bm25_index_from_token_ids(np.asarray(ids4), *_csr([final[d] for d in ids4]), 30, keep_tokens=True)
    assert _fwd(ix4) == _fwd(scratch4)
    for name in ("term_off", "post_doc", "post_tf", "doc_len"):
        assert _np(getattr(ix4, name)).tolist() == _np(getattr(scratch4, name)).tolist()
    # a base without a forward index gives a result without one
    bare = bm25_index_from_token_ids(base_ids, *_csr(base), 30)
    assert bm25_add_token_ids(bare, add_ids, *_csr(add), 30).tok_off is None
    assert remove_documents(bare, [30]).tok_off is None


def test_a_document_without_a_row_gets_its_stream_on_add():
    c = corpus(33)
    ix = c.ix                                                # document 5 (doc_id 22) has doc_len 0 and an empty stream
    assert int(_np(ix.doc_len)[5]) == 0
    out = bm25_add_token_ids(ix, np.array([22, 1000]), *_csr([[A, B, F], [X, Y]]), N_TERMS)
    assert out.n_docs == 34 and int(_np(out.doc_ids)[5]) == 22
    off, tok = _np(out.tok_off), _np(out.tok_ids)
    assert tok[off[5]:off[6]].tolist() == [A, B, F] and tok[off[33]:off[34]].tolist() == [X, Y]
    assert (np.diff(off) == _np(out.doc_len)).all()
    keep = [d for d in range(33) if d != 5]
    for d in keep:
        assert tok[off[d]:off[d + 1]].tolist() == c.tok_ids[c.tok_off[d]:c.tok_off[d + 1]].tolist()


def test_save_load_round_trip(tmp_path):
    ix = bm25_index_from_token_ids(np.arange(6) * 2, *_csr(_streams(6, 4)), 30, keep_tokens=True)
    ix.save(tmp_path / "with.npz")
    back = CorpusIndex.load(tmp_path / "with.npz")
    assert _fwd(back) == _fwd(ix) and back.tok_off.dtype == np.int64 and back.tok_ids.dtype == np.int32
    bare = bm25_index_from_token_ids(np.arange(6) * 2, *_csr(_streams(6, 4)), 30)
    bare.save(tmp_path / "without.npz")
    assert CorpusIndex.load(tmp_path / "without.npz").tok_off is None


def test_attach_tokens_accepts_the_true_streams_and_refuses_malformed_ones():
    streams = _streams(7, 5)
    off, tok = _csr(streams)
    ix = bm25_index_from_token_ids(np.arange(7), off, tok, 30)
    assert ix.tok_off is None
    assert attach_tokens(ix, off, tok) is ix
    assert _fwd(ix) == (off.tolist(), tok.tolist())
    fresh = lambda: bm25_index_from_token_ids(np.arange(7), off, tok, 30)
    bad_first = off.copy(); bad_first[0] = 1
    desc = off.copy(); desc[3] = desc[2] - 1
    big_id = tok.copy(); big_id[4] = 30
    neg_id = tok.copy(); neg_id[0] = -1
    moved = off.copy(); moved[3] += 1                        # two documents' lengths differ from doc_len, the total is right
    for o, t, why in ((bad_first, tok, "must be 0"), (desc, tok, "descends|doc_len"), (off[:-1], tok, "offsets"),
                      (off, tok[:-1], "ends at"), (off, big_id, "outside"), (off, neg_id, "outside"), (moved, tok, "doc_len")):
        ix2 = fresh()
        with pytest.raises(ValueError, match=why):
            attach_tokens(ix2, o, t)
        assert ix2.tok_off is None
    # a document without a BM25 row has length 0
    c = corpus(33)
    assert attach_tokens(CorpusIndex(**{k: getattr(c.ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf",
                                                                      "idf", "avgdl", "total_docs")}), c.tok_off, c.tok_ids)


def test_tokens_from_texts():
    texts = ["Max Planck Institut in Tuebingen", "", "Institut Planck Max", "das 3 Planck-Institut"]
    titles = ["Home", None, "", "Max"]
    from msretr.index_build import normalise_document_text
    words = [simple_tokenize(normalise_document_text(t, x)) for t, x in zip(titles, texts)]
    assert words[1] == []
    built = bm25_index_from_tokens([3, 1, 2, 0], words, keep_tokens=True)     # doc_id 1 has no tokens: no document
    assert built.n_docs == 3
    tb = {1: ("u", None, ""), 3: ("u", "Home", texts[0]), 2: ("u", "", texts[2]), 0: ("u", "Max", texts[3])}
    post = {t: [(int(built.doc_ids[d]), int(tf)) for d, tf in zip(built.post_doc[built.term_off[i]:built.term_off[i + 1]],
                                                                  built.post_tf[built.term_off[i]:built.term_off[i + 1]])]
            for t, i in built.vocab.items()}
    ix = CorpusIndex.from_tables(post, {int(d): int(n) for d, n in zip(built.doc_ids, built.doc_len)},
                                 {t: float(built.idf[i]) for t, i in built.vocab.items()}, built.avgdl, urls_db=tb)
    assert ix.n_docs == 4 and ix.tok_off is None             # (the urlsDB-only document 1 is a document here, without a row)
    off, tok = tokens_from_texts(ix)
    attach_tokens(ix, off, tok)
    inv = {v: k for k, v in ix.vocab.items()}
    got = [[inv[t] for t in tok[off[i]:off[i + 1]]] for i in range(4)]
    assert got == [words[3], [], words[2], words[0]]
    assert got[0] == ["max", "das", "planck", "institut"]
    ix.texts[2] = "Institut Planck Max Extra"
    with pytest.raises(ValueError, match="doc_len"):
        tokens_from_texts(ix)
    ix.texts[2] = "Institut Planck Unbekannt"
    with pytest.raises(ValueError, match="vocabulary"):
        tokens_from_texts(ix)

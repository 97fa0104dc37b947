"""CPU checks of the term-set cases (term_set_ref.py) and of the host side of the query operators: the numpy reference
against a brute-force set formulation on every case, every claimed edge present in the corpora, text.parse_operators,
DocSet.from_words and the index binding of a DeviceSets."""
import numpy as np
import pytest
import torch

from msretr.docset import DeviceSets, DocSet, pack_bits
from msretr.text import parse_operators, preprocess_query
from term_set_ref import BIG, HEAVY_DF, S, SIZES, base_mask, brute_force, corpus, random_rows, row_cases, term_set_mask


@pytest.fixture(scope="module")
def corpora():
    return {N: corpus(N) for N in SIZES}


def test_span_constant_and_sizes():
    assert S % 1024 == 0 and S >= 1024
    assert SIZES == [1, 31, 32, 33, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 37]


@pytest.mark.parametrize("N", SIZES)
def test_reference_against_brute_force(corpora, N):
    c = corpora[N]
    rows = row_cases(c) + (random_rows(c, 40) if N <= 1025 or N == BIG else [])
    assert len({r.claim for r in rows}) == len(rows)
    for r in rows:
        bm = base_mask(c, r.base)
        got = term_set_mask(c.z, r.must, r.must_not, bm)
        assert got.dtype == bool and got.shape == (N,)
        assert set(np.nonzero(got)[0].tolist()) == brute_force(c.z, r.must, r.must_not, bm), r.claim


def test_claimed_edges_are_present(corpora):
    c = corpora[BIG]
    off = c.z["term_off"]
    df = lambda name: int(off[c.term[name] + 1] - off[c.term[name]])
    N = BIG
    assert df("all") == N >= HEAVY_DF and df("even") == (N + 1) // 2
    assert df("n2047") == HEAVY_DF - 1 and df("n2048") == HEAVY_DF            # either side of the skip-table threshold
    assert df("empty") == 0
    for d in (0, 31, 32, 1023, 1024, S - 1, S, N - 1):
        assert c.docs[f"one_{d}"].tolist() == [d]
    assert c.docs["one_last"].tolist() == [N - 1]
    lw = c.docs["last_word"]
    assert N % 32 != 0 and len(lw) == N % 32 and (lw >> 5 == (N - 1) >> 5).all()      # all in the last, partial word
    sk = c.docs["skipper"]
    assert not ((sk >= S) & (sk < 2 * S)).any() and (sk < S).any() and (sk >= 2 * S).any()   # span 1 holds none of it
    assert (np.diff(c.z["post_doc"][off[c.term["n2048"]]:off[c.term["n2048"] + 1]]) > 0).all()
    # every term's list ascends strictly (what the engine validates at bind)
    for t in range(len(off) - 1):
        assert (np.diff(c.z["post_doc"][off[t]:off[t + 1]].astype(np.int64)) > 0).all()
    # the base with bits only in the last word
    name, m = c.bases[1]
    assert name == "base_last_word" and m.any() and not m[:((N - 1) // 32) * 32].any()
    claims = " | ".join(r.claim for r in row_cases(c))
    for word in ("unknown must id -1", "unknown must id n_terms", "unknown not ids", "both lists", "repeated", "70 must",
                 "early exit", "2047", "2048", "no posting in a whole span", "last word", "row_base == n_base",
                 "empty list: ignored", "empty list: empty row"):
        assert word in claims, word
    # the small corpora keep the cases they can hold, and lose only those they cannot
    assert "n2048" not in corpora[1025].term and "skipper" not in corpora[S + 1].term and "n2048" in corpora[S - 1].term
    assert len(row_cases(corpora[1])) >= 25


def test_reference_conventions():
    c = corpus(100)
    t, V = c.term, len(c.term)
    full = np.ones(100, bool)
    assert (term_set_mask(c.z, [], []) == full).all()
    assert not term_set_mask(c.z, [-1], []).any() and not term_set_mask(c.z, [V], []).any()
    assert not term_set_mask(c.z, [t["empty"]], []).any()
    assert (term_set_mask(c.z, [], [-1, V, t["empty"]]) == full).all()
    assert not term_set_mask(c.z, [t["even"]], [t["even"]]).any()
    assert (term_set_mask(c.z, [t["even"], t["even"]], []) == (np.arange(100) % 2 == 0)).all()
    odd = np.arange(100) % 2 == 1
    assert not term_set_mask(c.z, [t["even"]], [], odd).any()
    assert (term_set_mask(c.z, [], [t["even"]], odd) == odd).all()


PARSE = [
    # processed query                       scoring text                  must                 must_not
    ("+mensa tübingen",                     "mensa tübingen",             ["mensa"],           []),
    ("mensa +essen -stuttgart tübingen",    "mensa essen tübingen",       ["essen"],           ["stuttgart"]),
    ("mensa -stuttgart",                    "mensa",                      [],                  ["stuttgart"]),
    ("++a b",                               "++a b",                      [],                  []),
    ("--a b",                               "--a b",                      [],                  []),
    ("+-a b",                               "+-a b",                      [],                  []),
    ("-+a",                                 "-+a",                        [],                  []),
    ("uni-tuebingen c++ a+b",               "uni-tuebingen c++ a+b",      [],                  []),
    ("+uni-tuebingen",                      "uni-tuebingen",              ["uni-tuebingen"],   []),
    ("-c++",                                "",                           [],                  ["c++"]),
    ("a - b + c",                           "a - b + c",                  [],                  []),
    ("-",                                   "-",                          [],                  []),
    ("+",                                   "+",                          [],                  []),
    ("-123 +4x",                            "-123 +4x",                   [],                  []),
    ("-überfall +ökologie straße",          "ökologie straße",            ["ökologie"],        ["überfall"]),
    ("-a -a +a",                            "a",                          ["a"],               ["a", "a"]),
    ("  +a \t -b\n",                        "a",                          ["a"],               ["b"]),
    ("",                                    "",                           [],                  []),
    ("plain words only",                    "plain words only",           [],                  []),
]


@pytest.mark.parametrize("text,scoring,must,must_not", PARSE)
def test_parse_operators_table(text, scoring, must, must_not):
    assert parse_operators(text) == (scoring, must, must_not)


def test_parse_operators_after_preprocess_query():
    # the city is appended as a plain scoring term; an excluded word does not score
    assert parse_operators(preprocess_query("Mensa -Stuttgart")) == ("mensa tübingen", [], ["stuttgart"])
    assert parse_operators(preprocess_query("mensa +essen")) == ("mensa essen tübingen", ["essen"], [])
    # either ASCII spelling of the city becomes the city's term BEFORE the parse: it is excluded, not scored, not appended
    for spelling in ("-tuebingen", "-tubingen", "-tübingen", "-Tuebingen"):
        assert parse_operators(preprocess_query(f"mensa {spelling}")) == ("mensa", [], ["tübingen"])
    assert parse_operators(preprocess_query("+tuebingen mensa")) == ("tübingen mensa", ["tübingen"], [])
    # without operators the text is preprocess_query's
    q = preprocess_query("uni-tuebingen c++ kurs")
    assert parse_operators(q) == (q, [], [])


@pytest.mark.parametrize("N", [1, 31, 32, 33, 100, 1025])
def test_docset_from_words_inverts_words(N):
    c = corpus(N)
    rng = np.random.default_rng(N)
    for mask in (rng.random(N) < 0.5, np.ones(N, bool), np.zeros(N, bool), np.arange(N) == N - 1):
        ds = DocSet.from_mask(c.ix, mask)
        back = DocSet.from_words(c.ix, ds.words())
        assert back == ds and back.index is c.ix
        assert DocSet.from_words(c.ix, ds.words().view(np.int32)) == ds                    # the device rows' dtype
        padded = np.concatenate([ds.words(), np.full(3, 0xA5A5A5A5, np.uint32)])            # a row of a wider stride
        assert DocSet.from_words(c.ix, padded) == ds
        assert (back.words() == pack_bits(mask)).all()
    W = (N + 31) // 32
    if W > 1:
        with pytest.raises(ValueError):
            DocSet.from_words(c.ix, np.zeros(W - 1, np.uint32))
    if N % 32:
        bad = np.zeros(W, np.uint32)
        bad[-1] = np.uint32(1) << np.uint32(N % 32)                                        # the first bit past the last document
        with pytest.raises(ValueError):
            DocSet.from_words(c.ix, bad)


def test_device_sets_are_tied_to_their_index():
    c, other = corpus(100), corpus(100, seed=1)
    W = 4
    even = DocSet.from_mask(c.ix, np.arange(100) % 2 == 0)
    bits = torch.from_numpy(np.stack([even.words(), np.zeros(W, np.uint32)]).view(np.int32).copy())
    q_set = torch.tensor([0, -1, 1, 5, -3], dtype=torch.int32)
    ds = DeviceSets(c.ix, bits, q_set, 2, W)
    b, q, n, s = ds                                                                          # unpacks as pack_within's tuple
    assert b is bits and q is q_set and (n, s) == (2, W) and len(ds) == 5 and ds.index is c.ix
    ds.check(c.ix)
    with pytest.raises(ValueError, match="built for another index"):
        ds.check(other.ix)
    c2 = corpus(101)
    with pytest.raises(ValueError, match="built for another index"):
        ds.check(c2.ix)
    try:
        DocSet.from_mask(c.ix, np.zeros(100, bool)).check(other.ix)
    except ValueError as e:
        with pytest.raises(ValueError) as mine:
            ds.check(other.ix)
        assert str(mine.value) == str(e)                                                     # DocSet.check's wording
    assert ds.docset(0) == even
    assert len(ds.docset(1)) == 100                                                          # -1: every document
    assert len(ds.docset(2)) == 0 and len(ds.docset(3)) == 0 and len(ds.docset(4)) == 0      # empty row / out of range
    assert (ds.docset(0) - even).indices().tolist() == []

"""Typo-tolerant search without a GPU (DESIGN K15): the oracle of fuzzy_ref.py on known answers, the host policy of
msretr.fuzzy (the AUTO rule, what is looked up, what is replaced), the vocabulary image CorpusIndex.vocab_image hands to
msr_bind_vocab, and the mix of the random case the GPU test compares -- asserted on the oracle alone."""
import numpy as np
import pytest

from fuzzy_ref import KNOWN, MAX_LEN, expected, hand, osa, random_case
from msretr import fuzzy
from msretr.index import CorpusIndex

RANDOM_LIMIT = 3                                             # the limit test_gpu_fuzzy.py runs the random case with


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("a,b,d", KNOWN)
def test_oracle_on_known_answers(a, b, d):
    assert osa(a, b) == d and osa(b, a) == d


def test_oracle_distance_properties():
    assert osa("ca", "abc") == 3                             # restricted: no substring is edited twice (unrestricted: 2)
    assert osa("ab", "ba") == 1 and osa("tubingen", "tübingen") == 1
    assert osa("", "") == 0 and osa("", "ab") == 2 and osa("mensa", "mensa") == 0
    assert osa("xmensa", "mxensa") == 1 and osa("mensa", "menas") == 1       # a swap at the first and at the last position
    assert osa("mensa", "emnsax") == 2                       # swap plus insert
    assert osa("ä", "a") == 1 and osa("bär", "bar") == 1     # an umlaut is one code point, not its ASCII twin


def test_oracle_order_and_rows_on_the_hand_vocabulary():
    vocab, weights, words = hand()
    term, dist, n, total = expected(vocab, weights, words, [1] * len(words), 3)
    row = lambda w: [vocab[t] for t in term[words.index(w)] if t >= 0]
    assert row("mensb") == ["mensa", "mense", "menso"]       # one distance: the weight decides, descending
    assert row("kaus") == ["haus", "maus", "laus"] and total[words.index("kaus")] == 4     # distance and weight tie: the id
    assert row("mensa")[0] == "mensa" and dist[words.index("mensa")][0] == 0               # the word itself comes first
    assert row("geist") == ["geis"]                          # the term "geist" has weight 0: never a candidate
    assert row("tubingen") == ["tubingen", "tübingen"]
    assert total[words.index("")] == 0 and total[words.index("a" * 32 + "b")] == 0         # length 0 and 33: empty rows
    assert row("a" * 32) == ["a" * 31 + "b"]                 # the 33-code-point term (weight 0) is not among them
    assert (term[n == 0] == -1).all() and (dist[n == 0] == -1).all()
    # a tolerance outside {0, 1, 2} empties the row
    assert expected(vocab, weights, ["mensa"], [3], 3)[3][0] == 0 and expected(vocab, weights, ["mensa"], [-1], 3)[3][0] == 0


def test_random_case_has_every_kind_of_row():
    vocab, weights, words, maxes = random_case()
    assert len(vocab) == 3000 == len(set(vocab)) and len(words) == 64
    assert set("".join(vocab)) == set("abcä") and {len(s) for s in vocab} == set(range(1, 9))
    assert weights.count(0) > 100 and len(set(weights)) < 10 and max(weights) == 2 ** 31 - 1
    assert set(maxes) == {0, 1, 2}
    _, _, n, total = expected(vocab, weights, words, maxes, RANDOM_LIMIT)
    assert (total > RANDOM_LIMIT).sum() >= 10
    assert ((total > 0) & (total <= RANDOM_LIMIT)).sum() >= 10
    assert (total == 0).sum() >= 5
    assert (n == np.minimum(total, RANDOM_LIMIT)).all()


# ------------------------------------------------------------------------------------------------ the host policy
def test_auto_edits():
    assert [fuzzy.auto_edits(n) for n in range(9)] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert fuzzy.auto_edits(32) == 2


def test_lookable():
    assert fuzzy.lookable("mensa") and fuzzy.lookable("a" * 32) and fuzzy.lookable("x\ufffe")
    assert not fuzzy.lookable("") and not fuzzy.lookable("a" * 33) and not fuzzy.lookable("x\uffff")
    assert not fuzzy.lookable("caf\U0001F600") and not fuzzy.lookable(17)


def _index(vocab_terms, df):
    term_off = np.concatenate([[0], np.cumsum(df)]).astype(np.int64)
    return CorpusIndex(doc_ids=np.arange(4, dtype=np.int64), term_off=term_off, vocab={t: i for i, t in enumerate(vocab_terms)})


def test_vocab_image_layout_and_the_three_excluded_kinds():
    terms = ["mensa", "bär", "a" * 33, "leer", "x\uffffy", "a" * 32, "\U0001F600"]
    ix = _index(terms, [3, 2, 5, 0, 4, 1, 9])
    char_off, chars, weight = ix.vocab_image()
    assert char_off.dtype == np.int64 and chars.dtype == np.uint16 and weight.dtype == np.uint32
    assert char_off[0] == 0 and char_off[-1] == len(chars) and (np.diff(char_off) >= 0).all() and len(char_off) == len(terms) + 1
    text = lambda t: "".join(chr(c) for c in chars[char_off[t]:char_off[t + 1]])
    assert text(0) == "mensa" and text(1) == "bär" and text(5) == "a" * 32
    assert weight.tolist() == [3, 2, 0, 0, 0, 1, 0]          # too long / empty posting list / above 0xFFFE: never suggested
    assert ix.vocab_image() is ix.vocab_image()              # cached on the index ...
    ix.term_off = ix.term_off.copy()
    assert ix.vocab_image()[2] is not weight                 # ... for this (vocab, term_off)
    with pytest.raises(ValueError):
        CorpusIndex(doc_ids=np.arange(2), term_off=np.zeros(3, np.int64)).vocab_image()
    # an id that no term names keeps an empty string and weight 0
    gap = CorpusIndex(doc_ids=np.arange(2), term_off=np.asarray([0, 1, 2, 3], np.int64), vocab={"a": 0, "c": 2})
    assert gap.vocab_image()[0].tolist() == [0, 1, 1, 2] and gap.vocab_image()[2].tolist() == [1, 0, 1]


def test_encode_words():
    off, chars = fuzzy.encode_words(["ab", "ä", "xyz"])
    assert off.tolist() == [0, 2, 3, 6] and off.dtype == np.int32 and chars.dtype == np.uint16
    assert chars.tolist() == [ord(c) for c in "abäxyz"]
    assert fuzzy.encode_words([])[0].tolist() == [0]


class _Stub:
    """A lookup that knows a few typos, and records what it was asked."""
    NEAR = {"mesna": 7, "bibliotek": 8, "offnungszeiten": 9}
    NAMES = {7: "mensa", 8: "bibliothek", 9: "öffnungszeiten"}

    def __init__(self):
        self.calls = []

    def __call__(self, words):
        self.calls.append(list(words))
        return [self.NEAR.get(w, -1) for w in words]


def test_replacement_policy_on_a_stub_lookup():
    stub = _Stub()
    terms = [["mesna", "öffnungszeiten", "mesna"], ["bibliotek"], ["xq", "qqqqqq", 5], ["mensa"]]
    ids = [[-1, 3, -1], [-1], [-1, -1, 5], [2]]
    must = [["offnungszeiten"], [], ["bibliotek"], []]
    must_ids = [[-1], [], [-1], []]
    new_ids, new_must, corr = fuzzy.correct(stub, _Stub.NAMES.get, terms, ids, must, must_ids)
    # ONE lookup for the chunk, every unknown word once, in first-occurrence order; short words (tolerance 0), ints and known
    # words are not asked about
    assert stub.calls == [["mesna", "offnungszeiten", "bibliotek", "qqqqqq"]]
    assert new_ids == [[7, 3, 7], [8], [-1, -1, 5], [2]]     # only -1 entries change; without a candidate a -1 stays
    assert new_must == [[9], [], [8], []]                    # must terms: corrected the same way
    assert corr == [{"mesna": "mensa", "offnungszeiten": "öffnungszeiten"}, {"bibliotek": "bibliothek"},
                    {"bibliotek": "bibliothek"}, {}]
    assert ids == [[-1, 3, -1], [-1], [-1, -1, 5], [2]] and must_ids == [[-1], [], [-1], []]      # inputs untouched
    # nothing unknown: the lookup is not called at all
    quiet = _Stub()
    assert fuzzy.correct(quiet, _Stub.NAMES.get, [["mensa"]], [[2]]) == ([[2]], None, [{}]) and quiet.calls == []
    # a word that cannot be looked up is not asked about
    odd = _Stub()
    fuzzy.correct(odd, _Stub.NAMES.get, [["a" * 33, "x\uffffyz", "mesna"]], [[-1, -1, -1]])
    assert odd.calls == [["mesna"]]


def test_must_not_and_phrases_are_not_arguments_of_the_policy():
    """The policy cannot correct an excluded word or a phrase: it is never given one.  Retriever / BM25 pass the scoring terms
    and the must terms only (asserted here on the signature, on the device in test_gpu_fuzzy.py)."""
    import inspect
    assert list(inspect.signature(fuzzy.correct).parameters) == ["lookup", "name_of", "terms", "ids", "must", "must_ids"]
    for doc in (fuzzy.__doc__, fuzzy.correct.__doc__):
        assert "never corrected" in doc or "NOT corrected" in doc


def test_corrected_text_and_results():
    assert fuzzy.corrected_text("mesna öffnungszeiten tübingen", {"mesna": "mensa"}) == "mensa öffnungszeiten tübingen"
    assert fuzzy.corrected_text("Mesna +mesna", {"mesna": "mensa"}) == "mensa +mensa"
    assert fuzzy.corrected_text("mensa", {}) is None
    r = fuzzy.Results([{"rank": 1}], {"mesna": "mensa"}, "mensa")
    assert r == [{"rank": 1}] and r.corrections == {"mesna": "mensa"} and r.corrected_query == "mensa"
    assert fuzzy.Results().corrections == {} and fuzzy.Results().corrected_query is None


def test_constants_agree_with_the_header():
    import os
    import re
    from msretr import _abi
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "msretr.h"), encoding="utf-8").read()
    for name in ("MSR_FUZZY_MAX_LEN", "MSR_FUZZY_MAX_WORDS", "MSR_FUZZY_MAX_LIMIT", "MSR_FUZZY_SPAN_TERMS", "MSR_FUZZY_WORD_GROUP",
                 "MSR_ABI_VERSION"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_abi, name), name
    assert _abi.MSR_ABI_VERSION >= 15 and all(f in _abi._SIGNATURES for f in ("msr_bind_vocab", "msr_fuzzy_terms")) and fuzzy.MSR_FUZZY_MAX_LEN == _abi.MSR_FUZZY_MAX_LEN == MAX_LEN

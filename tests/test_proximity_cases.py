"""The oracle of proximity search (proximity_ref.py) against itself, and the host side of the feature (text.Near,
text.parse_proximity): no GPU.  The plain loops (the definitions of msretr.h), the sliding window / DP and the whole-stream
numpy form must agree on every case of every corpus and on 300 random rows per corpus; ordered rows with span == L are the
exact phrase (phrase_ref.phrase_mask)."""
import numpy as np
import pytest

from msretr._abi import MSR_PHRASE_MAX_TERMS, MSR_PROX_MAX_SPAN
from msretr.text import Near, parse_phrases, parse_proximity
from phrase_ref import cand_mask, phrase_mask
from proximity_ref import (A, B, F, VARIANTS, corpus, expected, mask_of, near_mask, near_mask_2, near_mask_fast, random_rows)


@pytest.mark.parametrize("N,empty_ends", VARIANTS)
def test_the_formulations_agree_on_every_case(N, empty_ends):
    c = corpus(N, empty_ends)
    cases, want = expected(N, empty_ends)
    assert len({(tuple(r.phrase), r.span, r.ordered, r.cand) for r in cases}) > 0.9 * len(cases)
    for r, w in zip(cases, want):
        assert (mask_of(c, r, near_mask_2) == w).all(), (N, r.claim)
        assert (mask_of(c, r, near_mask_fast) == w).all(), (N, r.claim)
        if "no match" in r.claim or "empty row" in r.claim or "nothing" in r.claim:
            assert not w.any(), (N, r.claim)
    if N >= 1025:                                            # the corpus holds every planted document: no edge is left out
        claims = " | ".join(r.claim for r in cases)
        for edge in ("exactly span = 64", "span + 1 = 65", "stream position 127", "lane 63", "chunk c + 2 (10000 tokens)",
                     "a later one matches", "A F F F A A B", "one P", "P Q F P", "B A F A", "over exactly 64 tokens",
                     "stream's last token", "length 0", "shorter than L", "span 65", "L = 17", "id of -1", "id of n_terms",
                     "row_cand == n_cand", "an empty candidate row", "bits 0, 31, 32"):
            assert edge in claims, edge
        hits = [w.any() for w in want]
        assert 0.3 < np.mean(hits) < 0.8                     # matches and misses in a fair mix


@pytest.mark.parametrize("N,empty_ends", VARIANTS)
def test_ordered_rows_with_span_L_are_the_exact_phrase(N, empty_ends):
    c = corpus(N, empty_ends)
    cases, want = expected(N, empty_ends)
    exact = [(r, w) for r, w in zip(cases, want) if r.claim.startswith("ordered, span == L")]
    assert len(exact) >= (40 if N > 1 else 20)
    for r, w in exact:
        assert r.ordered and r.span == len(r.phrase)
        assert (w == phrase_mask(c.tok_off, c.tok_ids, r.phrase, cand_mask(c, r.cand))).all(), (N, r.claim)
    for r in random_rows(c, 40, seed=3):
        got = near_mask(c.streams, r.phrase, len(r.phrase), True, cand_mask(c, r.cand))
        assert (got == phrase_mask(c.tok_off, c.tok_ids, r.phrase, cand_mask(c, r.cand))).all(), (N, r.phrase)


@pytest.mark.parametrize("N,empty_ends", VARIANTS)
def test_the_formulations_agree_on_300_random_rows(N, empty_ends):
    c = corpus(N, empty_ends)
    rows = random_rows(c, 300, seed=N)
    assert {r.ordered for r in rows} == {True, False} and len({r.span for r in rows}) >= 5
    n_hit = 0
    for r in rows:
        w = mask_of(c, r)
        assert (mask_of(c, r, near_mask_2) == w).all(), (N, r)
        assert (mask_of(c, r, near_mask_fast) == w).all(), (N, r)
        n_hit += bool(w.any())
    if N >= 1025:
        assert 60 <= n_hit < 300, n_hit                      # the mix holds empty rows and non-empty ones


def test_the_definitions_on_hand_made_streams():
    one = lambda s, p, span, ordered: bool(near_mask([s], p, span, ordered)[0])
    assert one([A, F, F, B], [A, B], 4, True) and not one([A, F, F, B], [A, B], 3, True)
    assert one([A, F, F, B], [B, A], 4, False) and not one([A, F, F, B], [B, A], 4, True)
    assert not one([A], [A, A], 64, True) and one([A], [A, A], 1, False)
    assert one([A, F, A], [A, A], 3, True) and not one([A, F, A], [A, A], 2, True)
    assert not one([], [A], 64, False) and not one([], [A], 64, True)
    assert not one([A, B], [A, B], 0, True) and not one([A, B], [A, B], 65, False) and not one([A, B], [], 5, False)
    # a match never uses tokens of two documents
    two = near_mask([[F, A], [B, F]], [A, B], 64, False)
    assert not two.any() and not near_mask_fast([0, 2, 4], [F, A, B, F], [A, B], 64, True).any()


def test_parse_proximity():
    assert parse_proximity("mensa tübingen") == ("mensa tübingen", [], [])
    assert parse_proximity('"max planck institut"~3 tübingen') == ("max planck institut tübingen",
                                                                  [Near("max planck institut", 3, ordered=False)], [])
    assert parse_proximity('"a b"~>3') == ("a b", [Near("a b", 3, ordered=True)], [])
    assert parse_proximity('x -"a b"~2 y') == ("x y", [], [Near("a b", 2)])
    assert parse_proximity('+"a b"~>0 c') == ("a b c", [Near("a b", 0, ordered=True)], [])
    # a `~` followed by anything else stays in the text and the phrase stays exact
    for text in ('"a b"~x c', '"a b"~', '"a b"~3x', '"a b"~>', '"a b" ~3', '"a b"~-1'):
        assert parse_proximity(text) == parse_phrases(text), text
        assert parse_proximity(text)[1] == ["a b"]
    assert parse_proximity('"a b"~') == ("a b ~", ["a b"], [])
    assert parse_proximity('"a b"~2 "c') == ('a b "c', [Near("a b", 2)], [])                   # an unbalanced last quote
    assert parse_proximity('"a b"~2 -"c d"~>1 e "f g"') == ("a b e f g", [Near("a b", 2), "f g"], [Near("c d", 1, ordered=True)])
    assert parse_proximity('""~3 a') == ("a", [], [])                                          # empty quotes are dropped
    for text in ('"a b" c -"d e" +"f"', 'a "b', 'uni-tuebingen "a"', '-"a b"', '"a b"~x', 'x "" y', '"a"b"c"'):
        assert parse_proximity(text) == parse_phrases(text), text
    must = parse_proximity('"a b" "c d"~1')[1]
    assert must[0] == "a b" and isinstance(must[0], str) and isinstance(must[1], Near)


def test_near_is_a_small_immutable_value():
    n = Near(["a", "b", "a"], slop=2)
    assert (n.terms, n.slop, n.ordered) == (("a", "b", "a"), 2, False)
    assert n.span == 4 and Near(["a", "b", "a"], 2, ordered=True).span == 5 and Near([7], 0).span == 1
    assert n == Near(("a", "b", "a"), 2) and hash(n) == hash(Near(("a", "b", "a"), 2)) and n != Near(["a", "b", "a"], 2, True)
    assert n.with_terms([4, 5, 4]) == Near([4, 5, 4], 2) and len(n) == 3 and not Near([])
    with pytest.raises(AttributeError):
        n.slop = 3
    with pytest.raises(ValueError, match="slop"):
        Near("a b", -1)
    with pytest.raises(ValueError, match="slop"):
        Near(["a"], 1.5)
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        Near(list(range(MSR_PHRASE_MAX_TERMS + 1)))
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        Near("a").with_terms(["a"] * 17)
    with pytest.raises(ValueError, match="MSR_PROX_MAX_SPAN"):
        Near([1, 2], MSR_PROX_MAX_SPAN - 1)                  # 2 distinct terms + 63 = 65
    assert Near([1, 2], MSR_PROX_MAX_SPAN - 2).span == 64 and Near([1, 1], 63).span == 64
    with pytest.raises(ValueError, match="MSR_PROX_MAX_SPAN"):
        Near([1, 1], 63, ordered=True)                       # ordered: a repeated id counts
    late = Near("a b c", 62)                                 # a string: the span shows once it is tokenised
    with pytest.raises(ValueError, match="MSR_PROX_MAX_SPAN"):
        late.with_terms(["a", "b", "c"])
    with pytest.raises(ValueError):
        late.span

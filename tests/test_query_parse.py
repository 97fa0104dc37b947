"""query.parse_queries against what the two parsers it replaced returned (tests/golden/query_parse_cases.json, recorded from
Retriever._operators / _prepare_ops and the parsing prefix of BM25.search before they were removed), and SearchOptions' range
check against the values the old checks refused.  No GPU."""
import json
import os

import numpy as np
import pytest

from msretr.query import Conditions, SearchOptions, parse_queries
from msretr.text import Near, preprocess_query, simple_tokenize

with open(os.path.join(os.path.dirname(__file__), "golden", "query_parse_cases.json"), encoding="utf-8") as _f:
    CASES = json.load(_f)


def _dec(x):
    """The file's {near, slop, ordered} objects -> text.Near."""
    if isinstance(x, dict):
        return Near(_dec(x["near"]), x["slop"], x["ordered"])
    return [_dec(y) for y in x] if isinstance(x, list) else x


def _options(case):
    return SearchOptions(**case.get("options", {}))


@pytest.mark.parametrize("case", CASES["retriever"], ids=lambda c: c["name"])
def test_retriever_cases(case):
    want = case["want"]
    explicit = Conditions(**{k: _dec(v) for k, v in case.get("explicit", {}).items()})
    call = lambda: parse_queries([preprocess_query(q) for q in case["queries"]], simple_tokenize, _options(case), explicit,
                                 case.get("patterns"))
    if "error" in want:
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == want["error"]
        return
    scoring, embed, cond, patterns = call()
    assert (scoring, embed, patterns) == (want["scoring"], want["embed"], want["patterns"])
    for name in ("must", "must_not", "must_phrases", "must_not_phrases"):
        assert getattr(cond, name) == _dec(want[name]), name


@pytest.mark.parametrize("case", CASES["bm25"], ids=lambda c: c["name"])
def test_bm25_cases(case):
    """BM25.search's call: one query as it is, each list as a one-element list, the patterns through str(), drop_empty."""
    want = case["want"]
    one = lambda v: None if v is None else [v]
    explicit = Conditions(**{k: [_dec(v)] for k, v in case.get("explicit", {}).items()})
    patterns = case.get("patterns")

    def call():
        _options(case).check(patterns=patterns is not None, int_types=int)
        return parse_queries([case["query"]], simple_tokenize, _options(case), explicit,
                             one(None if patterns is None else [str(p) for p in patterns]), drop_empty=True)
    if "error" in want:
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == want["error"]
        return
    (scoring,), _, cond, pats = call()
    pats = None if pats is None else pats[0]
    if want.get("empty"):                                    # BM25.search returns [] here, before it looks at the conditions
        assert not simple_tokenize(scoring) and not pats and cond.empty
        return
    assert simple_tokenize(scoring) or pats
    assert (scoring, pats) == (want["scoring"], want["patterns"])
    for name in ("must", "must_not", "must_phrases", "must_not_phrases"):    # (a pair that is None: BM25.search's empty lists)
        got = getattr(cond, name)
        assert ([] if got is None else got[0]) == _dec(want[name]), name


def test_the_pair_rule_and_the_chunk_slices():
    cond = parse_queries(["a +b", "c"], simple_tokenize, SearchOptions(operators=True))[2]
    assert (cond.must, cond.must_not, cond.must_phrases, cond.must_not_phrases) == ([["b"], []], [[], []], None, None)
    assert not cond.empty and Conditions().empty
    assert cond.slice(1, 2) == Conditions([[]], [[]]) and cond.slice(0, 1).must == [["b"]]
    ids = Conditions([["b", 7]], None, [[["a", "b"], Near("A b", 2, True)]], [[Near(["b"], 1)]]).ids(
        lambda terms: [t if isinstance(t, int) else {"a": 1, "b": 2}.get(t, -1) for t in terms], simple_tokenize)
    assert ids == Conditions([[2, 7]], None, [[[1, 2], Near([1, 2], 2, True)]], [[Near([2], 1)]])
    cond.check(2)
    with pytest.raises(ValueError, match="must: 2 entries for 3 queries"):
        cond.check(3)


@pytest.mark.parametrize("bad", [dict(wildcards=True, max_expansions=0), dict(wildcards=True, max_expansions=17),
                                 dict(wildcards=True, max_expansions=True), dict(wildcards=True, max_expansions=2.0),
                                 dict(snippets=True, snippet_tokens=0), dict(snippets=True, snippet_tokens=65),
                                 dict(facets=True, facet_limit=0), dict(facets=True, facet_limit=65),
                                 dict(facets=True, facet_by="tld"), dict(mode="dense")], ids=str)
def test_range_check_refuses(bad):
    with pytest.raises(ValueError):
        SearchOptions(**bad).check()


def test_range_check_accepts():
    SearchOptions().check()
    SearchOptions(mode="hybrid", snippets=True, snippet_tokens=64, wildcards=True, max_expansions=np.int64(16), facets=True,
                  facet_by="domain", facet_limit=64).check()
    # a limit is looked at only when its feature is on (explicit patterns count as wildcards), as before
    SearchOptions(max_expansions=0, snippet_tokens=0, facet_limit=0, facet_by="tld").check()
    with pytest.raises(ValueError, match="max_expansions"):
        SearchOptions(max_expansions=0).check(patterns=True)
    with pytest.raises(ValueError, match="max_expansions"):  # BM25.search's check takes no numpy integer, as before
        SearchOptions(wildcards=True, max_expansions=np.int64(8)).check(int_types=int)

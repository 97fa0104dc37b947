"""Prefix and wildcard terms without a GPU (DESIGN K16): the oracle of wildcard_ref.py against fnmatch and against known
answers, the query parser and the expansion policy of msretr.wildcard."""
import copy
import fnmatch

import pytest

from msretr import _abi
from msretr.fuzzy import Results
from msretr.wildcard import MIN_LITERALS, encodable, expand, literals, parse_wildcards, usable
from wildcard_ref import KNOWN, expected, glob_match, hand, random_case


# ------------------------------------------------------------------------------------------------ the oracle
def test_the_oracle_gives_the_known_answers():
    for p, answers in KNOWN:
        for t, want in answers.items():
            assert glob_match(p, t) is want, (p, t)
    vocab, _, _ = hand()
    by_len = {n: [t for t in vocab if len(t) == n] for n in (1, 2, 3)}
    assert all(by_len.values())
    assert [all(glob_match("??", t) for t in by_len[n]) for n in (1, 2, 3)] == [False, True, False]
    assert not any(glob_match("??", t) for t in by_len[1] + by_len[3])
    assert all(glob_match(p, t) for p in ("*", "**") for t in vocab)
    assert all(glob_match(p, t) for p in ("?*", "*?") for t in vocab if t) and not glob_match("?*", "") and not glob_match("*?", "")
    # no escape: a term that holds a metacharacter is reached through one
    assert glob_match("a*b", "a*b") and glob_match("a?b", "a*b") and glob_match("wer?", "wer?") and glob_match("wer?", "wert")


@pytest.mark.parametrize("case", ["hand", "random"])
def test_two_independent_oracles_agree_on_every_pair(case):
    vocab, _, patterns = hand() if case == "hand" else random_case()
    assert not any("[" in s for s in vocab + patterns)
    pairs = hits = 0
    for p in patterns:
        for t in vocab:
            got = glob_match(p, t)
            assert got == fnmatch.fnmatchcase(t, p), (p, t)
            pairs += 1
            hits += got
    assert pairs == len(vocab) * len(patterns) and 0 < hits < pairs


def test_expected_orders_by_weight_then_id_and_counts_all():
    vocab, weights, _ = hand()
    term, n, total = expected(vocab, weights, ["?aus", "geist", "t?bingen", "a" * 32 + "*", "", "*"], 3)
    haus = vocab.index("haus")
    assert term[0].tolist() == [haus, haus + 1, haus + 2] and n[0] == 3 and total[0] == 4      # tied on weight: the id decides
    assert term[1].tolist() == [-1, -1, -1] and total[1] == 0                                  # its only match weighs 0
    assert term[2].tolist() == [vocab.index("tübingen"), vocab.index("tubingen"), -1] and n[2] == total[2] == 2
    assert total[3] == total[4] == 0                                                           # 33 and 0 symbols
    assert total[5] == sum(1 for s, w in zip(vocab, weights) if w > 0 and len(s) <= 32)


# ------------------------------------------------------------------------------------------------ the parser
def test_parse_wildcards():
    assert parse_wildcards("uni* mensa tübingen") == ("mensa tübingen", ["uni*"])
    assert parse_wildcards("wo ist die mensa in tübingen?") == ("wo ist die mensa in tübingen?", [])      # punctuation
    assert parse_wildcards("t?bingen? mensa") == ("mensa", ["t?bingen"])
    assert parse_wildcards("mensa *bibliothek uni*thek") == ("mensa", ["*bibliothek", "uni*thek"])
    # a digit, a hyphen: not a pattern, left as it is
    assert parse_wildcards("uni-t*bingen b27* mensa") == ("uni-t*bingen b27* mensa", [])
    # inside quotes nothing is looked at, whether or not the phrases are parsed later
    assert parse_wildcards('"uni* mensa" neckar') == ('"uni* mensa" neckar', [])
    assert parse_wildcards('"uni* mensa" neck*') == ('"uni* mensa"', ["neck*"])
    assert parse_wildcards('-"alte aula*" aula*') == ('-"alte aula*"', ["aula*"])
    assert parse_wildcards('mensa "unbalanced uni*') == ('mensa "unbalanced', ["uni*"])           # no pair: no quoted text
    # required and excluded patterns
    for q in ("+uni* mensa", "mensa -uni*", "-t?bingen"):
        with pytest.raises(ValueError, match="required and excluded patterns are not supported"):
            parse_wildcards(q)
    assert parse_wildcards("+mensa -neckar") == ("+mensa -neckar", [])
    # a text without a pattern comes back unchanged, white space and all
    for q in ("", "mensa  tübingen ", "was? wo?", "c++ a-b"):
        assert parse_wildcards(q) == (q, [])
    assert parse_wildcards("* ?? a*") == ("", ["*", "?", "a*"])     # patterns all the same; expand() skips them


def test_literals_and_what_is_looked_up():
    assert MIN_LITERALS == 2
    assert [literals(p) for p in ("*", "a*", "??", "ab*", "t?bingen")] == [0, 1, 0, 2, 7]
    assert usable("ab*") and not usable("a*") and not usable("??") and not usable("")
    assert encodable("a" * 32) and not encodable("a" * 33) and not encodable("") and not encodable("ab\U0001F600*")
    assert not encodable("a\uffff*") and encodable("a\ufffe*")


# ------------------------------------------------------------------------------------------------ the policy
class FakeLookup:
    def __init__(self, table):
        self.table, self.calls = table, []

    def __call__(self, patterns):
        self.calls.append(list(patterns))
        return [self.table.get(p, ([], 0)) for p in patterns]


def test_expand_one_call_per_chunk_and_none_without_patterns():
    look = FakeLookup({"uni*": ([7, 8, 9], 5), "*thek": ([9, 3], 2)})
    name = lambda t: f"t{t}"
    ids, patterns = [[1, 2], [4], [5, -1]], [["uni*"], [], ["*thek", "uni*", "uni*"]]
    before = copy.deepcopy((ids, patterns))
    new_ids, exp = expand(look, name, ids, patterns, 8)
    assert look.calls == [["uni*", "*thek"]]                 # ONE call, distinct patterns, first-occurrence order
    assert (ids, patterns) == before                         # inputs not modified
    assert new_ids == [[1, 2, 7, 8, 9], [4], [5, -1, 9, 3, 7, 8]]
    assert exp[0] == {"uni*": {"terms": ["t7", "t8", "t9"], "total": 5}} and exp[1] == {}
    assert exp[2] == {"*thek": {"terms": ["t9", "t3"], "total": 2}, "uni*": {"terms": ["t7", "t8", "t9"], "total": 5}}
    assert list(exp[2]) == ["*thek", "uni*"]
    none = FakeLookup({})
    assert expand(none, name, [[1], [2]], [[], None], 8) == ([[1], [2]], [{}, {}]) and none.calls == []
    assert expand(none, name, [[1]], None, 8) == ([[1]], [{}]) and none.calls == []
    # the limit cuts what a generous lookup returns
    assert expand(FakeLookup({"uni*": ([7, 8, 9], 5)}), name, [[1]], [["uni*"]], 2)[0] == [[1, 7, 8]]


def test_expand_does_not_add_an_id_twice():
    look = FakeLookup({"uni*": ([7, 2, 9], 3), "un*": ([9, 7, 6], 3)})
    new_ids, exp = expand(look, str, [[2, 2, 5]], [["uni*", "un*"]], 8)
    assert new_ids == [[2, 2, 5, 7, 9, 6]]                   # 2 was typed, 9 and 7 came with the first pattern
    assert exp[0]["uni*"]["terms"] == ["7", "2", "9"] and exp[0]["un*"]["terms"] == ["9", "7", "6"]


def test_expand_stops_at_the_engines_limit_and_says_so():
    assert _abi.MSR_MAX_QUERY_TERMS == 64
    typed = list(range(100, 160))                            # 60 unique ids
    look = FakeLookup({"ab*": ([1, 2, 3], 3), "cd*": ([4, 5, 6], 9), "ef*": ([100, 7], 2)})
    new_ids, exp = expand(look, str, [typed], [["ab*", "cd*", "ef*"]], 8)
    assert new_ids[0] == typed + [1, 2, 3, 4] and len(set(new_ids[0])) == 64
    assert exp[0]["ab*"] == {"terms": ["1", "2", "3"], "total": 3}
    assert exp[0]["cd*"] == {"terms": ["4"], "total": 9, "truncated": True}
    assert exp[0]["ef*"] == {"terms": ["100"], "total": 2, "truncated": True}  # an id the query holds costs nothing
    full = list(range(64))
    again, exp = expand(look, str, [full], [["ab*"]], 8)
    assert again == [full] and exp[0]["ab*"] == {"terms": ["1", "2", "3"], "total": 3}


def test_expand_skips_a_pattern_below_two_literals():
    look = FakeLookup({"ab*": ([1], 1)})
    new_ids, exp = expand(look, str, [[9]], [["a*", "*", "??", "ab*", "a" * 33 + "*"]], 8)
    assert look.calls == [["ab*"]] and new_ids == [[9, 1]]
    for p in ("a*", "*", "??", "a" * 33 + "*"):
        assert exp[0][p] == {"terms": [], "total": 0, "skipped": True}
    only = FakeLookup({})
    assert expand(only, str, [[9]], [["a*"]], 8)[0] == [[9]] and only.calls == []
    # patterns are lower-cased like the query
    up = FakeLookup({"uni*": ([3], 1)})
    assert expand(up, str, [[9]], [["Uni*"]], 8) == ([[9, 3]], [{"uni*": {"terms": ["3"], "total": 1}}])


def test_results_carry_expansions_and_default_to_none():
    r = Results([{"a": 1}])
    assert r == [{"a": 1}] and r.expansions == {} and r.corrections == {} and r.corrected_query is None
    r = Results([], None, None, {"uni*": {"terms": ["uni"], "total": 1}})
    assert r.expansions == {"uni*": {"terms": ["uni"], "total": 1}} and Results.expansions == {}

"""The composed oracle of the query options (options_ref.py) and its table of cases (options_cases.py), on the CPU: the oracle
earns its trust against plain loops over the token streams, no case is vacuous, the pair table is complete, and no two rows of a
fused list are close enough for the GPU's rounding to swap them."""
from functools import lru_cache
from itertools import combinations

import numpy as np
import pytest

import options_ref as ref
from msretr.text import Near
from options_cases import BATCHES, EXCLUSIVE, FEATURES, WIDE, WIDE_TOP, crawl

MODES = ("lexical", "hybrid")
PARITY_BAR = 5e-6            # bench.py's rerank_parity
MIN_GAP = 4 * PARITY_BAR


@lru_cache(maxsize=None)
def answers(b, mode):
    return ref.expected(crawl(), BATCHES[b], mode, True)


def _cases():
    return [(b, q) for b in range(len(BATCHES)) for q in range(len(BATCHES[b].queries))]


def test_the_table_has_the_shape_the_suite_relies_on():
    assert sum(len(b.queries) for b in BATCHES) == 32 and all(len(b.queries) == 8 for b in BATCHES)
    for b in BATCHES:
        assert len(b.features) == len(b.sites) == len(b.seeds) == len(b.topic) == 8
        assert all(len(v) == 8 for v in b.lists.values()) and (b.term_lists is None or len(b.term_lists) == 8)
    assert sum(b.term_lists is None for b in BATCHES) == 2   # text syntax and explicit lists
    text = " ".join(q for b in BATCHES if b.term_lists is None for q in b.queries)
    for syntax in (" +", " -", ' "', ' -"', '"~2', '"~>1', "uni*", "t?bingen"):
        assert syntax in text, syntax


def test_every_pair_of_features_is_on_together_somewhere():
    """The pair table of options_cases: every pair of FEATURES is declared together by at least one query (every batch runs
    in both modes and under both settings of diversification), but for the pairs that cannot be (EXCLUSIVE)."""
    have = {frozenset(p) for b in BATCHES for f in b.features for p in combinations(sorted(f), 2)}
    want = {frozenset(p) for p in combinations(FEATURES, 2)} - EXCLUSIVE
    assert not want - have, sorted(map(sorted, want - have))
    assert any(len(f) == len(FEATURES) - 1 for b in BATCHES for f in b.features)           # one case has everything on
    assert not any(frozenset(p) in EXCLUSIVE for b in BATCHES for f in b.features for p in combinations(sorted(f), 2))


CONDITIONS = {"within", "must", "must_not", "must_phrase", "must_not_phrase", "near_ordered", "near_unordered"}


def _substance(e):
    """What a feature has to change to count: the documents, their scores and order, the passages, what was swallowed, where
    a row came from, and the counts over the match set -- not the mere presence of a key or of a bookkeeping entry
    (`expansions`, `corrections`, `highlights`, `missing`), which a switch of the whole call changes for every query."""
    rows = [(r["doc"], r["score"], r["snippet"], r.get("matched_by"), tuple(d["doc_id"] for d in r.get("duplicates", ()))) for r in e["rows"]]
    return rows, e["collapsed"], e["hits"], e["facets"], e["facet_values"]


@pytest.mark.parametrize("mode", MODES)
def test_no_case_is_vacuous(mode):
    """A query declares exactly the conditions it has, every switch it declares is on, and the oracle's answer without that ONE
    feature differs IN SUBSTANCE (_substance).  Facets add counts and change nothing else: a query that declares them has
    hits and a non-empty facet list, and more than one value hit."""
    c = crawl()
    bad = []
    for b, batch in enumerate(BATCHES):
        for q, plan in enumerate(ref.plans(c, batch)):
            on = ref.features_on(plan, c)
            assert batch.features[q] <= on, (b, q, sorted(batch.features[q] - on))
            assert batch.features[q] & CONDITIONS == on & CONDITIONS or not batch.features[q], (b, q, sorted(on & CONDITIONS))
            full = answers(b, mode)[q]
            for f in sorted(batch.features[q]):
                if f.startswith("facets"):
                    if not (full["hits"] > 0 and len(full["facets"]) > 0 and full["facet_values"] > 1):
                        bad.append((b, q, f))
                elif _substance(ref.evaluate(c, ref.without(plan, f), mode, True)) == _substance(full):
                    bad.append((b, q, f))
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
def test_rejected_pages_with_copies_are_passive_in_the_collapse(mode):
    """Three pages with copies are rejected by the response models (a NULL title): an original and its print view, and another
    original's print view.  In the cases with the collapse on that find them, the rejected original ranks AHEAD of its copies
    in the fused list and still leads nothing: its mirror is shown and swallows nothing; the other original does not swallow
    its rejected print view.  The oracle's answer with a collapse that ignores the table differs, so the cases tell a
    retriever that treats a rejected page as a leader from a right one."""
    c = crawl()
    gone, gone_print, other_print = c.rejected
    mirror = c.copies[gone][1]
    other = next(p for p, cs in c.copies.items() if cs[0] == other_print)
    assert all(c.ix.titles[d] is None for d in c.rejected) and c.ix.titles[mirror] is not None and c.ix.titles[other] is not None
    sig = ref.tables(c).sig
    assert min(ref.dedup_ref.matches(sig[gone], sig[mirror]), ref.dedup_ref.matches(sig[other], sig[other_print])) >= 58
    told, ahead = 0, 0
    for b, batch in enumerate(BATCHES):
        for q, plan in enumerate(ref.plans(c, batch)):
            e = answers(b, mode)[q]
            fused = e["fused"][0]
            if plan.collapse is None or gone not in fused or mirror not in fused:
                continue
            wrong = ref.evaluate(c, plan, mode, True, passive=False)
            shown = {r["doc"]: r for r in e["rows"]}
            drops = {d: lead for d, lead, _ in e["drops"]}
            assert not set(c.rejected) & (set(drops) | set(drops.values()) | set(shown)), (b, q)
            if fused.index(gone) < min(fused.index(mirror), fused.index(gone_print) if gone_print in fused else len(fused)):
                ahead += 1
                assert mirror not in drops and mirror in {d for d, _, _ in wrong["drops"]}, (b, q)
                if mirror in shown:
                    assert "duplicates" not in shown[mirror], (b, q)
            if ref.public(wrong) != ref.public(e):
                told += 1
                assert wrong["collapsed"] > e["collapsed"], (b, q)
    assert ahead >= 3 and told >= ahead, (ahead, told)


@pytest.mark.parametrize("mode", MODES)
def test_mostly_non_empty(mode):
    got = [answers(b, mode) for b in range(len(BATCHES))]
    assert sum(len(e["rows"]) > 0 for es in got for e in es) >= 24                        # three quarters of 32
    for b, es in enumerate(got):
        assert any(e["collapsed"] > 0 for e in es), b                                      # (collapse is on in every batch)
        assert any(e["hits"] is not None and e["hits"] > len(e["rows"]) for e in es), b    # (... and so are facets)
    # the cases the table promises
    c = crawl()
    unknown, lone, empty, few, capped = got[2][2], got[2][3], got[2][4], got[2][7], got[3][1]
    assert unknown["scored"] == [-1, -1] and unknown["hits"] == 0 and (len(unknown["rows"]) > 0) == (mode == "hybrid")
    assert empty["set"] is not None and not empty["set"].any() and empty["rows"] == [] and empty["hits"] == 0
    assert 0 < int(few["set"].sum()) and 0 < len(few["fused"][0]) < BATCHES[2].switches["top_k"]
    page, copy = c.must_copy
    docs = [r["doc"] for r in lone["rows"]]
    assert copy in docs and page not in docs and not lone["set"][page] and lone["set"][copy]
    assert "duplicates" not in lone["rows"][docs.index(copy)] and all(copy != d for d, _, _ in lone["drops"])
    assert ref.dedup_ref.matches(ref.tables(c).sig[page], ref.tables(c).sig[copy]) >= 58   # ... which the collapse would take
    assert capped["scored"].count(-1) == 1 and len(set(capped["scored"])) == ref.MAX_QUERY_TERMS
    assert capped["expansions"] == {"bib*": {"terms": [], "total": 3, "truncated": True}}


def _holds(s, p):
    """Plain loops: does the token list s hold the phrase / window p?"""
    if not isinstance(p, Near):
        L = len(p)
        return any(s[i:i + L] == list(p) for i in range(len(s) - L + 1))
    terms = list(p.terms)
    if p.ordered:
        span = len(terms) + p.slop

        def follow(j, prev, stop):
            if j == len(terms):
                return True
            return any(s[i] == terms[j] and follow(j + 1, i, stop) for i in range(prev + 1, min(stop, len(s))))
        return any(s[i] == terms[0] and follow(1, i, i + span) for i in range(len(s)))
    span = len(set(terms)) + p.slop
    return any(all(t in s[i:i + span] for t in set(terms)) for i in range(len(s)))


@pytest.mark.parametrize("mode", MODES)
def test_rows_satisfy_their_conditions_by_plain_loops(mode):
    """Independent of every mask helper: the token streams are scanned directly.  Every expected row (and every page the
    collapse dropped) lies in `within`, holds every required term, phrase and window and no excluded one; no row repeats a
    document; every dropped duplicate's leader is a kept row that ranked earlier."""
    c = crawl()
    words = lambda d: [c.names[t] for t in c.tok[c.off[d]:c.off[d + 1]]]
    checked = 0
    for b, batch in enumerate(BATCHES):
        for q, plan in enumerate(ref.plans(c, batch)):
            e = answers(b, mode)[q]
            _, must_ids, _ = ref.correct(c, plan)
            must = [c.names[t] if t >= 0 else None for t in must_ids]       # (a required word the vocabulary lacks: no page has it)
            docs = [r["doc"] for r in e["rows"]]
            assert len(set(docs)) == len(docs), (b, q)
            for d in docs + [d for d, _, _ in e["drops"]]:
                s = words(d)
                assert plan.within is None or plan.within[d], (b, q, d)
                assert all(w in s for w in must) and not any(w in s for w in plan.must_not), (b, q, d)
                assert all(_holds(s, p) for p in plan.must_phrases), (b, q, d)
                assert not any(_holds(s, p) for p in plan.must_not_phrases), (b, q, d)
                checked += 1
            rank = {d: i for i, d in enumerate(e["fused"][0])}
            kept = set(e["fused"][0]) - {d for d, _, _ in e["drops"]}
            for d, lead, m in e["drops"]:
                assert lead in kept and rank[lead] < rank[d] and m >= int(np.ceil(plan.collapse * 64)), (b, q, d, lead)
            shown = {r["doc"]: r for r in e["rows"]}
            for d, lead, _ in e["drops"]:
                assert lead not in shown or any(x["doc_id"] == str(int(c.z["doc_ids"][d])) for x in shown[lead]["duplicates"])
    assert checked > 1000


@pytest.mark.parametrize("mode", MODES)
def test_no_two_fused_rows_are_near_tied(mode):
    """Adjacent rows of every fused list differ by at least four times the rerank parity bar, so the rounding of the GPU's
    chain cannot reorder them: the GPU comparison needs no unordered groups (0 rows, below the 2 % the suite allows).  The
    same margin holds towards diversification's relevance threshold 0.8 and, for the cosines, at the dense stage's cut."""
    grouped = 0
    for b in range(len(BATCHES)):
        for q, e in enumerate(answers(b, mode)):
            s = np.asarray(e["fused"][1])
            if len(s) > 1:
                gap = -np.diff(s)
                print(b, q, "rows", len(s), "min gap %.3e" % gap.min())
                grouped += int((gap < MIN_GAP).sum())
                assert gap.min() >= MIN_GAP, (b, q, float(gap.min()))
            assert not len(s) or np.abs(s - 0.8).min() >= MIN_GAP, (b, q)
            assert e["dense_gap"] is None or e["dense_gap"] >= 5e-5, (b, q, e["dense_gap"])
    assert grouped == 0


@pytest.mark.parametrize("mode", MODES)
def test_the_wide_case_outgrows_the_copied_columns(mode):
    """The case beside the table: with the reranker's top_k raised and diversification off its first query keeps more rows
    than the 128 columns the retriever copies back per query, the collapse drops some, and the tie margin holds."""
    wide, small = ref.expected(crawl(), WIDE, mode, False, WIDE_TOP)
    assert len(wide["rows"]) > 128 and wide["collapsed"] > 0 and 0 < len(small["rows"]) < 128
    for e in (wide, small):
        gap = -np.diff(np.asarray(e["fused"][1]))
        print("rows", len(e["rows"]), "min gap %.3e" % gap.min())
        assert gap.min() >= MIN_GAP and (e["dense_gap"] is None or e["dense_gap"] >= 5e-5)

"""CPU checks of tests/select_cases.py: (a) the model of the select's control flow gives the reference's answer on every
case, (b) every branch tag is reached by a case that names it, (c) every planted mutation of the model is caught by at least
one case -- the evidence that tests/test_gpu_select.py, which runs the same cases through the kernels, would notice a select
that is subtly wrong.  Zeros compare by value with +0.0 bits, everything else by bits (select_cases.same_scores)."""
import numpy as np
import pytest

import select_cases as sc

_SEEN = {}


def _queries(case):
    """Every query of a small call; of a wide one the first, the last and a stride between (the rows are alike by design)."""
    return range(case.nq) if case.nq <= 8 else sorted({0, case.nq - 1, *range(0, case.nq, max(1, case.nq // 6))})


def _agrees(case, q, mut=None):
    docs, scores, state, tags = sc.model(case, q, mut)
    e_docs, e_scores = case.expected(q)
    return docs.tolist() == e_docs.tolist() and sc.same_scores(scores, e_scores), tags


@pytest.mark.parametrize("name", [n for n, _ in sc.CASES])
def test_model_equals_reference_and_reaches_its_branches(name):
    case = sc.build(name)
    assert case.nq <= sc.MAX_QUERIES and case.k <= 1024
    reached = set()
    for q in _queries(case):
        ok, tags = _agrees(case, q)
        assert ok, (name, q)
        reached |= tags
    assert case.tags <= reached, f"{name}: built to reach {sorted(case.tags - reached)}, reached {sorted(reached)}"
    _SEEN[name] = set(case.tags)


def test_every_branch_has_a_case_that_names_it():
    named = set()
    for name, fn in sc.CASES:
        named |= _SEEN[name] if name in _SEEN else set(fn().tags)
    assert named == set(sc.TAGS), sorted(set(sc.TAGS) - named)


CATCHERS = {                 # the cases each mutation is tried on (any of them returning a wrong answer catches it)
    "last_score_digit": ("group_float32_5000_k10", "group_float64_5000_k10"),
    "last_index_digit": ("tie200_one_index_block_k10",),
    "clamped_bin_resolved": ("win_bin0_clamped", "win_bound_too_low"),
    "cap_compare": ("group_4097_best_is_last",),
    "stage_overflow": ("stage_overflow_float32", "stage_overflow_float64"),
    "tie_descending": ("all_equal_float32_70000", "tie200_one_index_block_k10"),
}


@pytest.mark.parametrize("mut", list(sc.MUTATIONS))
def test_each_planted_mutation_returns_a_wrong_answer_somewhere(mut):
    assert set(CATCHERS) == set(sc.MUTATIONS)
    caught = []
    for name in CATCHERS[mut]:
        case = sc.build(name)
        assert all(_agrees(case, q)[0] for q in _queries(case)), name          # the unmutated model is right on it
        if not all(_agrees(case, q, mut)[0] for q in _queries(case)):
            caught.append(name)
    assert caught == list(CATCHERS[mut]), f"'{sc.MUTATIONS[mut]}' goes unnoticed on {sorted(set(CATCHERS[mut]) - set(caught))}"


def test_required_shapes_are_among_the_cases():
    """The row lengths, k values and query counts the select is pinned at."""
    built = {name: fn for name, fn in sc.CASES}
    lens, ks, nqs = set(), set(), set()
    for name in built:
        if name.startswith(("random_", "nq", "row_above")):
            c = built[name]() if not name.startswith("row_above") else None
            if c is not None:
                lens.add(c.n), ks.add(c.k), nqs.add(c.nq)
    assert {1, 63, 64, 65, 8191, 8192, 8193, 4 * 8192 + 1, 300001} <= lens
    assert {1, 2, 63, 64, 65, 100, 1000, 1023, 1024} <= ks
    assert {5, 1100, 2100} <= nqs and 2100 > sc.GRID
    assert sc.build("row_above_2p24").n > 1 << 24


def test_reference_is_the_plain_stable_sort():
    s = np.array([1.0, np.nan, -0.0, 0.0, -np.inf, np.inf, 1.0, -2.0], np.float32)
    d, v = sc.reference(s, None, 10)
    assert d.tolist() == [5, 0, 6, 2, 3, 7] and sc.same_scores(np.array([np.inf, 1, 1, 0, 0, -2], np.float32), v)
    assert not sc.same_scores(np.array([np.inf, 1, 1, -0.0, 0, -2], np.float32), v)

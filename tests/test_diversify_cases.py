"""The diversification cases on the host (tests/diversify_cases.py; DESIGN K6b): DESIGN's reduction, as plain loops, IS the
oracle on every generated case; both are the reference's own function on the executed fixtures (the old one and the edge
lists); and every named edge list has the property it is named for, counted with the oracle's own pieces."""
import json
import os
from urllib.parse import urlparse

import numpy as np
import pytest

import diversify_cases as dc


def _same(case, top_k, thr, **kw):
    a, b = dc.expected(case, top_k, thr, **kw), dc.reduced(case, top_k, thr, **kw)
    assert a == b, (case["name"], case["doc"].tolist(), case["score"].tolist(), top_k, thr, kw, a, b)
    return a


def test_reduction_equals_the_oracle_on_every_small_list():
    cases = dc.small_lists()
    assert 50_000 < len(cases) < 100_000
    assert {len(c["doc"]) for c in cases} == {1, 2, 3, 4, 5} and {c["top_k"] for c in cases} == {1, 2, 3, 4, 5, 6}
    rows = {tuple(c["score"]) for c in cases if len(c["doc"]) == 5}
    has = lambda f: any(f(r) for r in rows)
    assert has(lambda r: len(set(r)) == 5) and has(lambda r: len(set(r)) == 1) and has(lambda r: r[-1] == 0.0 and r[0] > 0)
    assert has(lambda r: dc.T in r and dc.BELOW in r) and has(lambda r: 5e-5 in r)
    assert has(lambda r: r.count(0.9) >= 2 and r.count(0.5) >= 2)          # ties on both sides of the threshold
    filled = shifted_to_zero = longer = 0
    for c in cases:
        got = _same(c, c["top_k"], dc.T)
        filled += any(s != c["score"][i] for i, s in got)
        shifted_to_zero += any(s == 0.0 and c["score"][i] > 0 for i, s in got)
        longer += len(got) > c["top_k"]
    assert filled > 1000 and shifted_to_zero > 100 and longer > 1000         # the fill, the clamp and the negative slice occur


@pytest.mark.parametrize("thr", dc.THRESHOLDS[1:])
def test_reduction_equals_the_oracle_at_other_thresholds(thr):
    for c in dc.small_lists(4):
        _same(c, c["top_k"], thr)
    for c in dc.edge_lists():
        _same(c, c["top_k"], thr)


def test_reduction_equals_the_oracle_on_edges_widths_tables_and_off():
    short = dc.DOMAIN_TABLE[:3 * dc.SLOTS + 2]
    for c in dc.edge_lists():
        for table in (dc.DOMAIN_TABLE, None, short):
            _same(c, c["top_k"], dc.T, table=table)
        _same(c, c["top_k"], dc.T, diversification=False)
        for top_k in (1, 2, len(c["doc"]), len(c["doc"]) + 1):
            _same(c, top_k, dc.T)
    n_calls = 0
    for M, top_k, cases in dc.widths():
        assert [c["n"] for c in cases] == [-3, 0, 1, M - 1, M, M + 7] and all(len(c["doc"]) == M for c in cases)
        for c in cases:
            got = _same(c, top_k, dc.T, max_cand=M)
            assert len(_same(c, top_k, dc.T, max_cand=M, diversification=False)) == min(top_k, len(dc._accepted(c, dc.DOMAIN_TABLE, M)))
            if c["n"] <= 0:
                assert got == []
        n_calls += 1
    assert n_calls == 7 * 4


def test_both_equal_the_executed_fixtures():
    with open(os.path.join(dc.GOLDEN, "diversification.json"), encoding="utf-8") as f:
        old = json.load(f)["cases"]
    assert len(old) == 10
    for c in old:
        doms = {}
        e = [(doms.setdefault(urlparse(u).netloc.lower(), len(doms)), float(s)) for _, u, s in c["input"]]
        case = dc.make("fixture", e)
        ids = [int(i) for i, _, _ in c["input"]]
        for fn in (dc.expected, dc.reduced):
            assert [[ids[i], s] for i, s in fn(case, c["top_k"])] == c["expected"]
    new = dc.load_fixture()["cases"]
    want = dc.fixture_inputs()
    assert len(new) == len(want) >= 5 * 25 and max(len(c["doc"]) for c in new) <= 40
    for got, (case, top_k, thr) in zip(new, want):                            # the fixture IS the generator's lists ...
        assert got["name"] == case["name"] and got["doc"] == case["doc"].tolist() and got["score"] == case["score"].tolist()
        assert got["top_k"] == top_k and got["threshold"] == thr and got["domain"] == dc.domains(case["doc"]).tolist()
        for fn in (dc.expected, dc.reduced):                                  # ... and the reference returned what both give
            assert [[i, s] for i, s in fn(case, top_k, thr)] == got["expected"], (case["name"], thr, fn.__name__)


def test_every_edge_list_has_its_edge():
    cases = dc.edge_lists()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        a = dc.anatomy(c, c["top_k"])
        claims = dict(c["claims"])
        assert claims, c["name"]
        if "slice_sign" in claims:
            assert np.sign(a["n_medium"] + a["remaining"]) == claims.pop("slice_sign"), c["name"]
        if "delta_sign" in claims:
            assert a["delta"] is not None and np.sign(a["delta"]) == claims.pop("delta_sign"), c["name"]
        for k, v in claims.items():
            assert a[k] == v, (c["name"], k, a[k], v)
        assert a["n_kept"] + a["n_dropped"] == a["n_accepted"]
    by = {c["name"]: dc.anatomy(c, c["top_k"]) for c in cases}
    K = 5
    # the number of high domains at top_k - 1, top_k, top_k + 1 and 2 top_k; n_medium + remaining below, at and above 0
    assert [by[f"high{h}_medium{m}"]["n_high"] for h, m in ((4, 3), (5, 3), (6, 3), (10, 2), (10, 5), (6, 1))] == [4, 5, 6, 10, 10, 6]
    assert by["high6_medium3"]["remaining"] == -1 and by["high6_medium3"]["n_final"] == 6 + 2
    assert by["high10_medium2"]["n_medium"] + by["high10_medium2"]["remaining"] < 0 and by["high10_medium2"]["n_final"] == 10
    assert by["high10_medium5"]["n_medium"] + by["high10_medium5"]["remaining"] == 0 and by["high10_medium5"]["n_final"] == 10
    assert by["high6_medium1"]["n_medium"] + by["high6_medium1"]["remaining"] == 0
    assert by["high5_medium3"]["remaining"] == 0 and by["high5_medium3"]["n_final"] == K and by["high5_medium3"]["n_added"] == 0
    assert by["high4_medium3"]["n_final"] == K
    assert [by[f"kept{k}"]["n_kept"] for k in (4, 5, 6)] == [4, 5, 6] and by["kept4"]["n_added"] == 1 and by["kept6"]["n_added"] == 0
    assert [by[f"accepted{k}"]["n_accepted"] for k in (4, 5, 6)] == [4, 5, 6]
    # the wave edges: accepted slots and accepted ranks around every multiple of 64
    c = next(c for c in cases if c["name"] == "accepted_around_the_wave_edges")
    acc = np.nonzero(dc.domains(c["doc"]) >= 0)[0].tolist()
    assert all({64 * k - 1, 64 * k, 64 * k + 1} <= set(acc) for k in range(1, 16)) and acc[-1] == 1023 and len(acc) == 47
    c = next(c for c in cases if c["name"] == "ranks_across_the_wave_edges")
    a = by["ranks_across_the_wave_edges"]
    assert a["n_accepted"] > 960 and a["n_kept"] > 256 and a["n_high"] > 64 and a["n_dropped"] > 64 and a["n_added"] > 64
    assert by["every_entry_kept"]["n_kept"] == 1018 and by["high_domains_in_pairs"]["n_high"] == 512
    # repeated documents: one document at three slots
    c = next(c for c in cases if c["name"] == "documents_repeated")
    assert np.bincount(c["doc"] % dc.SLOTS)[5] == 5 and len(set(c["doc"].tolist())) == 3

"""The K-split sweep's bind rule and ring bookkeeping, restated in Python (tests/dense_geometry_cases.py), on the CPU.

* every named layout gets the verdict written next to it, from the restated rule and from the library's own chunk_layout
  (msr_debug_chunk_layout: host only, no device);
* the bookkeeping with two retired blocks per unit and the window rule alone -- what the engine shipped before -- mislabels
  or loses documents on sustained sparse layouts: the reason the bind now walks the bookkeeping;
* with the walk, no accepted layout mislabels a document: every named case, and 2 000 seeded layouts of that family."""
import ctypes as C

import numpy as np
import pytest

import dense_geometry_cases as G


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", G.CASES, ids=_ids(G.CASES))
def test_named_cases_get_their_stated_verdict(case):
    assert 0 < case.doc_off[-1] <= 4096
    assert tuple(int(x) for x in G.window_rule(case.doc_off)) == case.window
    r = G.bind_rule(case.doc_off)
    assert (r["wide_ok"], r["wide_ok64"]) == case.wide
    if case.doc_off[-1] <= 511:                                     # one span whatever the CU count
        assert all(G.bind_rule(case.doc_off, n_cus=n)["n_spans"] == 1 for n in (1, 8, 256, 304))


def test_the_edges_are_where_the_issue_puts_them():
    """The documents under two consecutive groups span 96 (taken) / 97 (refused); 32 / 33 for the 64-document ring; one group's
    rows span 32 / 33 -- each with the first document at offset 0 and 31 of its block."""
    def spans(off):
        off = np.asarray(off)
        n = int(off[-1])
        two = max(G._last_doc_below(off, min(16 * (u + 2), n) - 1) - G._last_doc_below(off, 16 * u) for u in range((n + 15) // 16))
        one = max(G._last_doc_below(off, min(16 * (u + 1), n) - 1) - G._last_doc_below(off, 16 * u) for u in range((n + 15) // 16))
        return two, one
    for lead in (0, 31):
        first = lambda name: int(np.nonzero(np.diff(G.BY_NAME[name].doc_off))[0][0])
        for name, two in ((f"window96_lead{lead}", 96), (f"window97_lead{lead}", 97), (f"ring64_span32_lead{lead}", 32),
                          (f"ring64_span33_lead{lead}", 33)):
            assert spans(G.BY_NAME[name].doc_off)[0] == two and first(name) % 32 == lead, name
        assert spans(G.BY_NAME[f"group32_lead{lead}"].doc_off)[1] == 32
        assert spans(G.BY_NAME[f"group33_lead{lead}"].doc_off)[1] == 33
    assert G.BY_NAME["window96_lead0"].wide == (1, 0) and G.BY_NAME["window97_lead0"].wide == (0, 0)
    assert G.BY_NAME["ring64_span32_lead31"].wide == (1, 1) and G.BY_NAME["ring64_span33_lead31"].wide == (1, 0)
    assert G.BY_NAME["group32_lead31"].wide[0] == 1 and G.BY_NAME["group33_lead31"].wide[0] == 0


def test_run_and_partial_cases_cover_the_stated_sizes():
    for run in (1, 31, 32, 33, 95, 96, 97, 200):
        lead, trail = G.BY_NAME[f"leading_run{run}"].counts, G.BY_NAME[f"trailing_run{run}"].counts
        assert not any(lead[:run]) and lead[run] > 0 and not any(trail[-run:]) and trail[-run - 1] > 0
    seen = {(len(c.counts) % 32, sum(c.counts) % 16) for c in G.CASES if c.name.startswith("partial_")}
    assert {d for d, _ in seen} == {1, 31} and {r for _, r in seen} == {1, 15}
    big = [c for c in G.CASES if G.bind_rule(c.doc_off)["n_spans"] > 1 and c.wide[0]]
    assert len(big) >= 2                                            # accepted cases with span cuts inside the pattern
    # CorpusIndex.shard cuts at the first document at or after half the rows: shard 0 ends with the document in front of a
    # run, shard 1 begins with that whole run (and ends with the layout's last one)
    s0, s1 = (G.BY_NAME[f"shard{r}of2_gap95_x64"].counts for r in range(2))
    assert s0[-1] == 16 and not any(s1[:95]) and s1[95] == 16 and not any(s1[-95:])
    assert s0 + s1 == G.BY_NAME["sustained_1x16_gap95_x64"].counts


def test_two_blocks_per_unit_lose_documents_on_sustained_layouts():
    """The reason for the walk, kept on record: with the window rule alone these layouts were taken, and the kernel's two
    retirements per unit fall behind.  Counts for one span, a ring of 128 (both the plain and the pipelined instance: the
    kernel retires after unit g the blocks complete before it, rows_done = 16 g)."""
    want = {"sustained_1x16_gap64_x16": 0, "sustained_1x16_gap70_x16": 12, "sustained_1x16_gap80_x16": 24,
            "sustained_1x16_gap95_x16": 24, "sustained_16x1_gap48_x16": 0, "sustained_16x1_gap56_x16": 272,
            "sustained_16x1_gap64_x16": 384}
    for name, n_wrong in want.items():
        c = G.BY_NAME[name]
        assert G.bind_rule(c.doc_off, lag_walk=False)["wide_ok"] == 1, name      # the old rule took every one of them
        wrong = G.ring_walk(c.doc_off, G.make_spans(c.doc_off, 256), G.RING, retire=2)
        assert len(wrong) == n_wrong and bool(wrong) == c.loses, (name, len(wrong))
        has = np.diff(c.doc_off) > 0
        if wrong:                                                   # both kinds: a document with rows lost, a chunk-less one
            assert has[wrong].any() and (~has[wrong]).any(), name   # reporting another document's rows
            assert has[G.planted_document(c)] and G.planted_document(c) in wrong
    # three retirements per unit would have kept up on all of them (the alternative fix, not taken)
    for name in want:
        c = G.BY_NAME[name]
        assert G.ring_walk(c.doc_off, G.make_spans(c.doc_off, 256), G.RING, retire=3) == [], name


@pytest.mark.parametrize("n_cus", [256, 8, 1])
def test_no_accepted_named_case_mislabels_a_document(n_cus):
    for c in G.CASES:
        r = G.bind_rule(c.doc_off, n_cus=n_cus)
        spans = G.make_spans(c.doc_off, n_cus)
        if r["wide_ok"]:
            assert G.ring_walk(c.doc_off, spans, G.RING, retire=2) == [], c.name
        if r["wide_ok64"]:
            assert G.ring_walk(c.doc_off, spans, G.RING64, retire=2) == [], c.name
        if n_cus == 256:
            assert bool(G.ring_walk(c.doc_off, spans, G.RING, retire=2)) == c.loses, c.name


def test_no_accepted_random_sustained_layout_mislabels_a_document():
    rng = np.random.default_rng(20240)
    n, accepted, old_rule_lost = 3200, 0, 0
    for _ in range(n):
        off = G.offsets(G.random_sustained(rng))
        assert off[-1] == 256
        spans = G.make_spans(off, 256)
        r = G.bind_rule(off)
        wrong = G.ring_walk(off, spans, G.RING, retire=2)
        if r["wide_ok"]:
            accepted += 1
            assert wrong == []
            if r["wide_ok64"]:
                assert G.ring_walk(off, spans, G.RING64, retire=2) == []
        elif G.bind_rule(off, lag_walk=False)["wide_ok"]:
            old_rule_lost += 1
            assert wrong != []                                      # the walk refuses nothing the kernel would get right
    assert accepted >= 2000 and accepted >= n // 2, accepted
    assert old_rule_lost >= 100, old_rule_lost                      # the family does reach what the old rule let through


# ------------------------------------------------------------------------------------------------ the library's own rule
@pytest.fixture(scope="module")
def lib():
    from msretr import _abi
    return _abi.load()


def _native(lib, doc_off, n_cus=256):
    off = np.ascontiguousarray(doc_off, dtype=np.int32)
    out = (C.c_int32 * 4)(0, 0, 0, n_cus)
    rc = lib.msr_debug_chunk_layout(off.ctypes.data_as(C.c_void_p), len(off) - 1, out)
    assert rc == 0, lib.msr_last_error(None)
    return dict(wide_ok=out[0], wide_ok64=out[1], tiles_ok=out[2], n_spans=out[3])


@pytest.mark.parametrize("case", G.CASES, ids=_ids(G.CASES))
def test_library_rule_equals_the_restatement_on_named_cases(lib, case):
    for n_cus in (256, 8, 1):
        assert _native(lib, case.doc_off, n_cus) == G.bind_rule(case.doc_off, n_cus=n_cus), n_cus
    got = _native(lib, case.doc_off)
    assert (got["wide_ok"], got["wide_ok64"]) == case.wide


def test_library_rule_equals_the_restatement_on_random_layouts(lib):
    rng = np.random.default_rng(7)
    verdicts = set()
    for i in range(300):
        if i % 3 == 0:
            counts = G.random_sustained(rng)
        else:                                                       # runs of 0 .. 100 chunk-less documents among 0 .. 20-row ones
            counts = []
            while sum(counts) < int(rng.integers(1, 1500)):
                counts += [0] * int(rng.integers(0, 101)) * int(rng.random() < 0.3)
                counts += rng.integers(0, int(rng.choice([2, 6, 21])), size=int(rng.integers(1, 40))).tolist()
        off = G.offsets(counts)
        n_cus = int(rng.choice([1, 3, 256]))
        got = _native(lib, off, n_cus)
        assert got == G.bind_rule(off, n_cus=n_cus), (i, n_cus)
        verdicts.add((got["wide_ok"], got["wide_ok64"]))
    assert verdicts == {(0, 0), (1, 0), (1, 1)}


def test_library_rule_refuses_malformed_offsets(lib):
    out = (C.c_int32 * 4)(0, 0, 0, 0)
    for bad in ([1, 2, 3], [0, 5, 3]):
        off = np.asarray(bad, np.int32)
        assert lib.msr_debug_chunk_layout(off.ctypes.data_as(C.c_void_p), len(off) - 1, out) != 0
    assert lib.msr_debug_chunk_layout(None, 0, out) != 0
    one = np.zeros(1, np.int32)                                     # no documents at all: nothing to refuse
    assert lib.msr_debug_chunk_layout(one.ctypes.data_as(C.c_void_p), 0, out) == 0

"""The inputs of test_gpu_bm25_rounds.py checked on the CPU: the cap and R come from the sources the library is compiled from,
every list has the counts its name claims, the round cut puts the edges where the cases say, and the kernel's mark / rank /
round rule restated in numpy (bm25_round_cases.restated) equals oracle/bm25_ref.topk bit for bit on every query, setting
and span width."""
import numpy as np
import pytest

import bm25_round_cases as rc
from oracle import bm25_ref

TILE, N, SPAN8, CAP, RES = rc.TILE, rc.N_DOCS, rc.SPAN8, rc.CAP, rc.RES


@pytest.fixture(scope="module")
def corpus():
    z, T = rc.build_corpus()
    queries, names = rc.build_queries(z, T)
    return z, T, queries, names


def _list(z, t):
    return z["post_doc"][z["term_off"][t]:z["term_off"][t + 1]].astype(np.int64)


def _span_words(docs, s):
    d = docs[(docs >= s * SPAN8) & (docs < (s + 1) * SPAN8)] - s * SPAN8
    return rc.bitmap_words(d, SPAN8 // 32), d


def test_cap_and_resident_chunks_come_from_the_sources():
    assert CAP == rc.round_cap() and CAP % 128 == 0 and 128 <= CAP <= TILE      # the kernel's static_assert restated
    assert RES == rc.resident_chunks() and 1 <= RES <= 16
    assert rc.COUNTS == (CAP - 1, CAP, CAP + 1, 2 * CAP, 2 * CAP + 1, 8192)


def test_corpus_is_well_formed(corpus):
    z, T, _, _ = corpus
    assert len(z["doc_len"]) == N == 60 * TILE + 517 and N % 32 == 5
    assert z["term_off"][0] == 0 and z["term_off"][-1] == len(z["post_doc"]) == len(z["post_tf"])
    for t in range(len(z["idf"])):
        d = _list(z, t)
        assert len(d) > 0 and d[0] >= 0 and d[-1] < N and (np.diff(d) > 0).all(), t
    df = np.diff(z["term_off"])
    assert len(T["neg_tabled"]) == 64 and len(T["neg_untabled"]) == 2
    assert all(df[t] >= rc.HEAVY_DF and z["idf"][t] < 0 for t in T["neg"])
    # documents that LACK a looked-up term are as common as documents that have it
    assert all(0.3 < 1 - df[t] / N < 0.5 for t in T["neg_tabled"])


def test_touched_counts_of_a_span(corpus):
    z, T, _, _ = corpus
    single = _list(z, T["count_single"])
    union = [_list(z, t) for t in T["count_union"]]
    for s, c in enumerate(rc.COUNTS):
        w, d = _span_words(single, s)
        assert len(d) == c
        cuts = [x for x in rc.round_cuts(w, CAP) if x[3]]
        assert (len(cuts) == 1) == (c <= CAP)
        assert sum(x[3] for x in cuts) == c and all(x[3] <= CAP for x in cuts)
        if c > CAP:
            assert len(cuts) >= -(-c // CAP)                  # word granularity: a round may end short of the cap
        u = np.unique(np.concatenate([x[(x >= s * SPAN8) & (x < (s + 1) * SPAN8)] for x in union]))
        assert len(u) == c
        per = [int(((x >= s * SPAN8) & (x < (s + 1) * SPAN8)).sum()) for x in union]
        assert sum(per) > c                                   # the three lists overlap
        if c < SPAN8:
            assert all(p < CAP for p in per), (s, per)        # (8192 cannot be the union of three lists below the cap)


def test_round_edges(corpus):
    z, T, _, _ = corpus
    W = rc.FILL_WORD
    # the document that fills the first round: bit 31 of word W / bit 0 of word W + 1 / the last document of a tile / of the span
    for name, s, word, bit in (("fill_bit31", 0, W, 31), ("fill_bit0", 1, W + 1, 0), ("fill_tile_edge", 3, TILE // 32 - 1, 31),
                               ("fill_span_edge", 4, SPAN8 // 32 - 1, 31)):
        w, d = _span_words(_list(z, T[name]), s)
        assert d[CAP - 1] == 32 * word + bit, name
        cuts = [x for x in rc.round_cuts(w, CAP) if x[3]]
        assert cuts[0][3] == CAP and cuts[0][1] >= word + 1, name
        if name == "fill_span_edge":
            assert len(cuts) == 1 and len(d) == CAP and d[-1] == SPAN8 - 1
            assert (5 * SPAN8 in _list(z, T[name]))                  # the next span starts with a posting of the list
        else:
            assert len(cuts) == 2 and cuts[1][3] == len(d) - CAP > 0
        if name == "fill_tile_edge":
            assert d[CAP] == TILE
    # a word that does not fit: the round is cut in front of it, one short of the cap
    w, d = _span_words(_list(z, T["overfull_word"]), 2)
    assert d[CAP - 1] == 32 * W and d[CAP] == 32 * W + 5
    cuts = [x for x in rc.round_cuts(w, CAP) if x[3]]
    assert cuts[0][3] == CAP - 1 and cuts[0][1] == W and cuts[1][0] == W
    d = _list(z, T["bits_0_31"])
    assert set((d % 32).tolist()) == {0, 31} and len(d) == 2 * (N // 32) + 1
    assert _list(z, T["last_word_doc"]).tolist() == [N - 2] and (N - 2) // 32 == N // 32      # the partial word of 5 bits


def test_resident_chunk_slices(corpus):
    z, T, _, _ = corpus
    df = np.diff(z["term_off"])
    h = _list(z, T["res_heavy"])
    assert df[T["res_heavy"]] >= rc.HEAVY_DF                   # skip table: a span's slice is exactly its postings
    assert ((h // SPAN8) == 0).sum() == 64 * RES and ((h // SPAN8) == 1).sum() == 64 * RES + 1
    m = _list(z, T["res_med"])
    assert 64 < df[T["res_med"]] < rc.HEAVY_DF
    assert ((m // SPAN8) == 2).sum() == 64 * RES and ((m // SPAN8) == 3).sum() == 64 * RES + 1
    assert len(T["one"]) == 40 and all(df[t] == 1 for t in T["one"])
    assert len({int(_list(z, t)[0]) // SPAN8 for t in T["one"]}) == 1


def test_queries_cover_the_looked_up_term_positions(corpus):
    z, T, queries, names = corpus
    q = dict(zip(names, queries))
    tabled, unt = set(T["neg_tabled"]), set(T["neg_untabled"])
    assert q["neg_first"][0] in tabled and q["neg_last"][-1] in tabled
    assert q["neg_middle"][1] in tabled and q["neg_middle"][0] not in tabled and q["neg_middle"][2] not in tabled
    two = q["neg_two_in_a_row"]
    assert two[1] in tabled and two[2] in tabled and two[1] != two[2]
    assert sum(t in tabled for t in q["neg_three"]) == 3
    assert q["untabled_beside_tabled"][0] in unt and q["untabled_beside_tabled"][1] in tabled
    assert len(q["ones_40_of_64"]) == len(set(q["ones_40_of_64"])) == 64
    assert sum(t in set(T["one"]) for t in q["ones_40_of_64"]) == 40
    assert len(q["ones_R"]) == RES and len(q["ones_R_plus_1"]) == RES + 1
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("k,ms", rc.SETTINGS)
def test_restated_kernel_equals_the_oracle_bit_for_bit(corpus, k, ms):
    z, T, queries, names = corpus
    tabled = set(T["neg_tabled"])
    assert tabled == rc.tabled_terms(z)
    multi = 0
    for name, q in zip(names, queries):
        d0, s0 = bm25_ref.topk(z, q, k, ms)
        for tpw in (1, 8):
            stats = []
            d1, s1 = rc.restated(z, tabled, q, k, ms, tpw, stats=stats)
            assert d0.tolist() == d1.tolist(), (name, tpw)
            assert s0.tobytes() == s1.tobytes(), (name, tpw)
            multi += sum(len(c) > 1 for _, c, _ in stats)
    assert multi > 50                                         # spans that really run in several rounds

"""The inputs of test_gpu_bm25_spans.py checked on the CPU: the corpus has the shapes its docstring promises, the restated
width rule gives the widths the GPU cases are named after, the oracle the GPU is held to agrees with the reference-shaped
loops on these shapes, and every setting leaves the rows the span-width code paths need (short rows, full rows, touched
documents that are dropped in front of kept documents of the same accumulator slot)."""
import math

import numpy as np
import pytest

import bm25_span_cases as sc
from oracle import bm25_ref

TILE, N = sc.TILE, sc.N_DOCS


@pytest.fixture(scope="module")
def corpus():
    z, T = sc.build_corpus()
    queries, names = sc.build_queries(z, T)
    return z, T, queries, names


def _list(z, t):
    return z["post_doc"][z["term_off"][t]:z["term_off"][t + 1]].astype(np.int64)


def test_corpus_is_well_formed_and_has_the_promised_lengths(corpus):
    z, T, _, _ = corpus
    V = len(z["idf"])
    assert len(z["doc_len"]) == N == 60 * TILE + 517 and (N + TILE - 1) // TILE == 61
    assert z["term_off"][0] == 0 and z["term_off"][-1] == len(z["post_doc"]) == len(z["post_tf"])
    assert (z["post_tf"] >= 1).all() and (z["post_tf"] <= 5).all() and (z["doc_len"] >= 5).all()
    for t in range(V):
        d = _list(z, t)
        assert len(d) > 0 and d[0] >= 0 and d[-1] < N and (np.diff(d) > 0).all(), t     # strictly ascending, in range
    df = np.diff(z["term_off"])
    # list classes: long negative (64 tabled + 6 streamed), idf 0, long positive, every whole-list class boundary
    assert len(T["neg"]) == 70 and len(T["neg_tabled"]) == 64 and len(T["neg_untabled"]) == 6
    assert all(df[t] >= sc.HEAVY_DF and z["idf"][t] < 0 for t in T["neg"])
    assert min(df[t] for t in T["neg_tabled"]) >= max(df[t] for t in T["neg_untabled"])
    assert z["idf"][T["zero"]] == 0.0 and df[T["zero"]] > N // 2 and z["idf"][T["pos_long"]] > 0 and df[T["pos_long"]] > N // 2
    for n in (1, 63, 64, 65, 2047, 2048, 2049, 9000):
        assert df[T["len_%d" % n]] == n
    assert df[T["short_neg"]] <= 64 and z["idf"][T["short_neg"]] < 0
    # exactly 64 .. 385 postings in single tiles at the first, a middle and the last tile of a span of 8
    for cls in ("med", "heavy"):
        for pos, off in sc.TILE_POS.items():
            t = T["tile_%s_%s" % (cls, pos)]
            assert (df[t] >= sc.HEAVY_DF) == (cls == "heavy") and df[t] > 64
            per_tile = np.bincount(_list(z, t) // TILE, minlength=61)
            for s, c in enumerate(sc.TILE_COUNTS):
                assert per_tile[8 * s + off] == c, (cls, pos, s)
                assert (8 * s + off) % 8 == off
            if cls == "med":
                assert per_tile.sum() == sum(sc.TILE_COUNTS)
    # both sides of every tile edge, document 0 and N - 1, in one medium list
    e = set(_list(z, T["edges"]).tolist())
    assert 64 < len(e) < sc.HEAVY_DF and 0 in e and N - 1 in e
    assert all(t * TILE - 1 in e and t * TILE in e for t in range(1, 61))
    for name, edge in (("straddle_8192", 8192), ("straddle_2048", 2048)):
        d = _list(z, T[name])
        assert len(d) == 80 and d[0] == edge - 40 and d[-1] == edge + 39
    d = _list(z, T["one_tile"])
    assert 64 < len(d) < sc.HEAVY_DF and d[0] // TILE == d[-1] // TILE == 37
    # the 64 probes of the medium-list round look at the last posting of chunks of ceil(len / 64): those are tile edges
    d = _list(z, T["probe_chunks"])
    ch = (len(d) + 63) // 64
    assert 64 < len(d) < sc.HEAVY_DF and len(d) == 61 * ch
    for c in range(61):
        assert d[(c + 1) * ch - 1] == min((c + 1) * TILE, N) - 1 and d[c * ch] >= c * TILE
    # heavy lists with whole empty spans / dense tiles next to empty tiles
    d = _list(z, T["heavy_blocks"])
    assert len(d) == 3000 >= sc.HEAVY_DF and set((d // sc.SPAN8).tolist()) == {0, 6}
    per_tile = np.bincount(_list(z, T["heavy_dense"]) // TILE, minlength=61)
    assert per_tile[20] == per_tile[22] == per_tile[59] == TILE and per_tile[60] == 517 and per_tile.sum() == 3 * TILE + 517
    # the window pass: two terms far below the strongest one, one of them in every document
    top = max(float(x) for x in z["idf"])
    assert z["idf"][T["strong"]] == np.float32(top)
    assert abs(z["idf"][T["tiny_a"]] / top - 1e-7) < 1e-9 and abs(z["idf"][T["tiny_all"]] / top - 3e-9) < 1e-10
    assert df[T["tiny_all"]] == N
    assert z["avgdl"] == float(np.float32(z["doc_len"].mean()))


def test_width_rule_restated_gives_the_widths_the_cases_are_named_after():
    n_tiles = (N + TILE - 1) // TILE
    assert sorted({v[0] for v in sc.WIDTH_CASES.values()}) == [1, 2, 4, 8]
    for nq, (tpw, spans, last, parts, per) in sc.WIDTH_CASES.items():
        assert sc.split_rule(n_tiles, nq) == (tpw, spans), nq
        assert n_tiles - (spans - 1) * tpw == last, nq
        assert sc.select_parts(spans, nq) == (parts, per), nq
    # what the cases are there for: a short last span with an odd tile count; a select workgroup with several segments; select
    # workgroups that own no segment; a last workgroup with fewer segments than the others
    assert sc.WIDTH_CASES[1024][2] == 5 and sc.WIDTH_CASES[1024][2] < 8
    parts, per = sc.select_parts(61, 100)
    assert per == 4 and [p for p in range(parts) if p * per >= 61] == [16, 17, 18, 19]
    parts, per = sc.select_parts(61, 255)
    assert 61 - (parts - 1) * per == 5
    parts, per = sc.select_parts(31, 265)
    assert 31 - (parts - 1) * per == 1


def test_fill_puts_every_query_at_many_positions(corpus):
    _, _, queries, _ = corpus
    nd = len(queries)
    for nq in sc.WIDTH_CASES:
        idx = sc.fill(nd, nq)
        assert len(idx) == nq
        seen = np.concatenate([sc.fill(nd, nq, start) for start in sc.calls_for(nd, nq)])
        assert set(seen.tolist()) == set(range(nd)), nq          # every distinct query runs at every width
        stride = int(idx[1] - idx[0]) % nd
        assert math.gcd(stride, nd) == 1
        if nq >= 4 * nd:
            pos = np.nonzero(idx == 5)[0]
            assert len(pos) >= 4 and len(set((pos % 64).tolist())) >= 3      # not always the same lane / workgroup slot


def test_queries_cover_the_kinds_the_kernel_distinguishes(corpus):
    z, T, queries, names = corpus
    assert 30 <= len(queries) <= 48 and len(set(names)) == len(names)
    uniq = [list(dict.fromkeys(q)) for q in queries]
    assert max(len(u) for u in uniq) == 64 and sum(len(u) == 50 for u in uniq) == 1
    assert [] in queries
    q = dict(zip(names, queries))
    assert set(T["neg_untabled"]) <= set(q["untabled"])
    tabled = set(T["neg_tabled"])
    assert q["neg_first"][0] in tabled and q["neg_last"][-1] in tabled and q["neg_repeated"].count(q["neg_repeated"][0]) == 2
    # a looked-up term behind more than four streamed terms
    b = q["beyond_prefetch"]
    streamed_before = [sum(1 for x in b[:i] if x not in tabled) for i, t in enumerate(b) if t in tabled]
    assert max(streamed_before) > 4
    assert any(t < 0 for t in q["unknown_ids"]) and any(t >= len(z["idf"]) for t in q["unknown_ids"])


def test_oracle_agrees_with_the_reference_shaped_loops_on_a_cut_down_corpus(corpus):
    z, _, queries, names = corpus
    small = sc.cut_down(z, 3 * TILE + 517)                       # 4 tiles, the last one partial
    assert len(small["doc_len"]) == 3589 and small["term_off"][-1] == len(small["post_doc"])
    for name, q in zip(names, queries):
        for k, ms in ((1000, 0.0), (100, -100.0), (1000, 0.75)):
            d0, s0 = bm25_ref.topk(small, q, k, ms)
            d1, s1 = bm25_ref.topk_literal(small, q, k, ms)
            assert d0.tolist() == d1.tolist(), (name, k, ms)
            assert s0.tobytes() == s1.tobytes(), (name, k, ms)


def test_every_setting_leaves_short_rows_full_rows_and_dropped_documents(corpus):
    z, _, queries, names = corpus
    for k, ms in sc.SETTINGS:
        lens = [len(bm25_ref.topk(z, q, k, ms)[0]) for q in queries]
        assert any(0 < n < k for n in lens), (k, ms)
        assert any(n == k for n in lens), (k, ms)
        assert any(n == 0 for n in lens), (k, ms)
    # min_score = 0.75: touched-but-dropped documents in a tile whose FOLLOWING tile, in the same span of 8, keeps documents
    # in the same accumulator slots -- what a missed reset at the end of a tile would corrupt
    hit = []
    for name, q in zip(names, queries):
        ut, qtf = bm25_ref.prepare_query(q, z["term_off"])
        if not ut:
            continue
        acc, touched = bm25_ref.scores_dense(z, ut, qtf)
        dropped = np.zeros(61 * TILE, bool); kept = np.zeros(61 * TILE, bool)
        dropped[:N] = touched & ~(acc >= 0.75)
        kept[:N] = touched & (acc >= 0.75)
        dropped, kept = dropped.reshape(61, TILE), kept.reshape(61, TILE)
        for t in range(60):
            if t % 8 != 7 and (dropped[t] & kept[t + 1]).any():
                hit.append((name, t))
                break
    assert len(hit) >= 5, hit
    # and documents pushed below 0 by a looked-up negative term in front of kept ones (min_score = 0)
    q = queries[names.index("neg_between")]
    acc, touched = bm25_ref.scores_dense(z, *bm25_ref.prepare_query(q, z["term_off"]))
    assert (touched & (acc < 0)).any() and (touched & (acc >= 0)).any()


def test_document_sets_of_the_restricted_calls():
    m = sc.within_masks()
    assert m["none"] is None and not m["empty"].any() and m["one"].sum() == 1 and m["every_other"].sum() == (N + 1) // 2
    b = np.nonzero(m["block"])[0]
    assert b[0] == 8000 and b[-1] == 8399 and b[0] // TILE != b[-1] // TILE and b[0] // sc.SPAN8 != b[-1] // sc.SPAN8
    t = np.nonzero(m["tail_word"])[0]
    assert t[0] == (N // 32) * 32 and t[-1] == N - 1 and 0 < len(t) < 32

"""The catalogue of the call-sequence tests (tests/call_sequence_cases.py), checked without a GPU: the names, every input
predicate numpy can decide (the sizes against the capacities read from the sources, the heavy / light split, the branch tags of
the select cases), the reproducibility of the seeded sequences, and that every public method of DeviceEngine is placed.

Two things this file does NOT show.  Entry.methods is declared by hand next to each entry, not observed from its calls: the
introspection test proves that every public method is NAMED by an entry or excluded with a reason, so that a new entry point
cannot be added without someone placing it; that the named methods are really called is what the path predicates and oracles
of the GPU file show (final_lists_hybrid declares none: it goes through the Retriever).  And the catalogue borrows helpers of
other test modules by their private names (test_gpu_hybrid's _planted / _with_urls / NH / QH / DENSE_K, options_cases' _streams
/ _word), because the issue asks for the existing fixtures, not copies of them: a rename there breaks the import here, loudly."""
import numpy as np
import pytest

import bm25_span_cases as sc
import call_sequence_cases as cs
import select_cases as S


def test_names_are_unique_and_every_entry_is_placed():
    names = [e.name for e in cs.PROBES + cs.DIRTIERS]
    assert len(names) == len(set(names))
    assert all(e.kind == "probe" and e.check is None and e.group is None for e in cs.PROBES)
    for d in cs.DIRTIERS:
        assert d.kind == "dirtier" and callable(d.check) and d.group in cs.GROUPS, d.name
        assert d.bundles and set(d.bundles) <= set(cs.ALL), d.name
    assert {d.group for d in cs.DIRTIERS} == set(cs.GROUPS)
    for b in cs.ALL:                                           # every bundle has probes of its own stage and dirtiers
        assert len(cs.entries_for(b, "probe")) >= 5 and len(cs.entries_for(b, "dirtier")) >= 15, b
    assert cs.MAX_QUERIES >= 512 and cs.MAX_K <= 1024
    # about a dozen probes, one per stage, at the batch sizes of the three dense paths
    assert {"bm25_topk_16", "bm25_topk_within", "dense_topk_8", "dense_topk_100", "dense_topk_200", "dense_topk_within",
            "dense_topk_batched_100", "dense_topk_batched_200", "dense_topk_grouped", "score_docs_union", "rerank_chain",
            "final_lists_hybrid", "merge_topk", "select_f32", "select_f64_list", "dense_begin_end"} == {p.name for p in cs.PROBES}
    assert 8 <= 64 < 100 <= cs.caps()["bt_slice"] == 128 < 200


def test_select_picks_carry_their_tags():
    caps = cs.caps()
    assert caps["sel_cap"] == S.CAP and caps["sel_bins"] == S.BINS and caps["stage"] == S.STAGE
    for name, (case_name, tags) in cs.SELECT_PICKS.items():
        case = cs.select_case(case_name)
        assert set(tags) <= set(S.TAGS) and case.k <= cs.MAX_K and case.nq <= cs.MAX_QUERIES, name
        states, reached = cs.modelled(case_name)
        assert set(tags) <= reached and case.tags <= reached, (name, sorted(reached))
        done = [st[S.STATE_FIELDS.index("done")] for st in states]
        if "row_general" in tags:
            assert not any(done), name                         # more than MSR_SEL_CAP share the prefix: done == 0
    # the tie groups against the cap
    g = cs.select_case("group_float32_5000_k10")
    assert 5000 > caps["sel_cap"] and int((g.scores[0] >= S._bits32(np.uint32(0x3F880000))).sum()) == 5000
    lt = cs.select_case("list_ties_over_cap")
    assert (lt.counts.sum(axis=1) == 9000).all() and 9000 > caps["sel_cap"]
    st = cs.select_case("stage_overflow_float32")
    assert 3000 > caps["stage"] and st.scores.shape[1] == 5 * S.PART
    fv = cs.select_case("k_above_valid_float32")
    assert [len(fv.expected(q)[0]) for q in range(3)] == [100, 1, 0] and fv.k == 101
    w = cs.select_case("within_mixed_sets")
    assert w.q_set.tolist() == [-1, 0, 1, 2, 9, -7, 3] and not w.set_bits[2].any() and w.set_bits.shape[0] == 4
    for name in cs.SELECT_PROBES.values():                     # the probes are plain: done early, nothing overflows
        states, reached = cs.modelled(name)
        assert not reached & {"row_general", "win_overflow", "stage_overflow", "cap_plus_one"}, (name, sorted(reached))
        assert cs.select_case(name).k <= cs.MAX_K
    nan = cs.nan_row_case()
    assert np.isnan(nan.scores[1]).all() and [len(nan.expected(q)[0]) for q in range(3)] == [100, 0, 100]
    gp = cs.gate_per64_case()
    assert gp.nq == 130 and cs.GATE_WORDS == (1, 0, 5) and (gp.scores[5] == 0.5).all() and (gp.scores[70] == 0.25).all()
    assert gp.scores.shape[1] > caps["sel_cap"]                # both tie groups exceed the cap: one in an ON, one in the OFF slice


def test_bm25_slices_are_what_they_are_named():
    L = cs.lex_inputs()
    assert len(L.queries) == 43 + 9 + 1 and L.n_docs == sc.N_DOCS == 61 * 1024 - 507
    for nq, split in cs.SPLITS.items():
        assert sc.split_rule(61, nq) == split, nq
    for nq in (16, 512):
        w, heavy = L.heavy_set(0.0, cs.SPLITS[nq][0])
        H, Lt = np.nonzero(heavy)[0], np.nonzero(~heavy)[0]
        assert len(H) >= 4 and len(Lt) >= 8
        assert heavy[L.slice_rows("heavy", nq)].all() and not heavy[L.slice_rows("light", nq)].any()
        assert len(L.slice_rows("heavy", nq)) == nq == len(L.slice_rows("light", nq))
        for n in ("neg_alone", "unknown_only", "empty"):       # no streamed term at all among the light
            assert w[L.name[n]] == 0 and not heavy[L.name[n]]
    V = len(L.z["idf"])
    assert all(t < 0 or t >= V for t in L.queries[L.name["unknown_only"]]) and L.queries[L.name["empty"]] == []
    assert len(L.mixed16) == 16 == len(set(L.mixed16)) and max(L.mixed16) < 43
    names = L.within_names(16)
    assert set(names) == set(L.masks) and not L.masks["empty"].any()
    assert len(L.z2["doc_len"]) == L.n_docs and len(L.z2["idf"]) != V         # the rebind target is another index


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_dense_inputs_overflow_what_they_say(fmt):
    caps = cs.caps()
    D = cs.dense_inputs(fmt)
    c = D.c
    big_docs = np.unique(np.searchsorted(c.doc_off, np.nonzero(c.row_query == D.big)[0], side="right") - 1)
    assert len(big_docs) == 5500 > caps["gf_pair_cap"] and 5500 > caps["sel_cap"] and 5500 > caps["gm_pair_cap"]
    assert c.queries[D.big].kind == "big" and D.big not in D.ordinary and len(D.distinct) == 16
    n_tiles = len(c.tiles) - 1
    assert n_tiles >= 2 * 100 and n_tiles >= 64                 # the streaming pass serves k = 10 and the grouped dirtier's k = 100
    assert 50 * 100 > caps["merge_cap"]                        # 50 copies of one row at k = 100: past the merge's LDS image
    assert D.n_docs >= cs.MAX_K + 1 and 0 < c.split_doc < D.n_docs
    idx, q = D.rows(200)
    assert q.shape == (200, 768) and set(idx) == set(range(16)) and np.isfinite(q).all() and (np.abs(q).sum(axis=1) > 0).all()
    assert set(D.within_names(16)) == set(D.masks) and D.masks["block"].sum() == 400


def test_hybrid_inputs():
    from test_gpu_hybrid import DENSE_K, NH, QH
    h = cs.hyb_inputs()
    assert h.n_docs == NH == h.ix.n_docs and len(h.terms) == QH == len(h.qv) and h.dense_k == DENSE_K
    assert h.terms[3] == [-1, -2] and h.planted.shape == (QH, DENSE_K) and h.distinct.shape == (64, 768)
    assert h.ix.tok_off is not None and len(h.ix.vocab) == h.ix.n_terms and len(h.tok_off) == NH + 1
    assert h.facet.min() == -1 and h.facet.max() == 40
    df = np.diff(h.z["term_off"])
    assert df[30] > NH / 2 and df[31] > NH / 2                 # the phrase's words: negative idf, hence min_score = -1e9 there
    assert all(0 < df[t] < NH / 2 for t in h.mid[:4])
    n_tiles = len(A_tiles(h.doc_off)) - 1
    assert n_tiles >= 2 * 100                                  # the streaming pass serves the split calls and k = 100
    assert set(h.rows(200)[0]) == set(range(64)) and not h.masks["empty"].any()


def A_tiles(doc_off):
    import dense_adversary as A
    return A.greedy_tiles(doc_off)


def test_refusals_name_their_entry_points():
    from msretr import _abi
    assert set(cs.REFUSALS_RAW) <= set(_abi._SIGNATURES)
    for b in cs.ALL:
        want = cs.refusals_expected(b)
        assert cs.REFUSALS_ANY <= want and (("dense_topk_batched_k" in want) == (b == "bf16"))
    assert len(cs.refusals_expected("hyb")) == 30
    split = cs.by_name("split_begin_refused_calls_end")
    assert "bf16" in split.bundles and "dense_topk_batched" in split.methods      # the bf16 guard is tried with the image built


def test_merge_inputs():
    docs, sco, ns = cs.merge_lists_input()
    assert docs.shape == (3, 4, 37) and (np.diff(sco, axis=2) <= 0).all()
    docs, sco, ns, k, _ = cs.merge_overflow_input()
    assert (sco[7, 1] > sco[:7, 1].max()).all()                # query 1: one shard holds all of the best
    assert np.isnan(sco[2, 0, 3]) and ns[:, 2].tolist() == [-3, 0, k, k + 5, 1, -1, k + 1000, 7] and (ns[:, 3] == 0).all()


def test_seeded_sequences_are_reproducible():
    for b in cs.ALL:
        seqs = [cs.seeded_sequence(s, b) for s in cs.SEQUENCE_SEEDS]
        assert len(cs.SEQUENCE_SEEDS) == 3 and all(len(s) == cs.SEQUENCE_STEPS == 200 for s in seqs)
        assert seqs == [cs.seeded_sequence(s, b) for s in cs.SEQUENCE_SEEDS]
        assert len({tuple(s) for s in seqs}) == 3
        probes = {e.name for e in cs.entries_for(b, "probe")}
        dirt = {e.name for e in cs.entries_for(b, "dirtier")}
        for s in seqs:
            assert set(s) <= probes | dirt and set(s) & probes and set(s) & dirt
        assert dirt <= set().union(*map(set, seqs)), (b, sorted(dirt - set().union(*map(set, seqs))))   # every dirtier is drawn
        assert probes <= set().union(*map(set, seqs))


def test_every_public_method_of_the_engine_is_placed():
    from msretr.engine import DeviceEngine
    public = {n for n, v in vars(DeviceEngine).items() if not n.startswith("_") and (callable(v) or isinstance(v, property))}
    used = set()
    for e in cs.PROBES + cs.DIRTIERS:
        assert set(e.methods) <= public, (e.name, sorted(set(e.methods) - public))
        used |= set(e.methods)
    assert set(cs.EXCLUDED_METHODS) <= public, sorted(set(cs.EXCLUDED_METHODS) - public)
    assert not used & set(cs.EXCLUDED_METHODS), sorted(used & set(cs.EXCLUDED_METHODS))
    assert all(isinstance(r, str) and len(r) > 20 for r in cs.EXCLUDED_METHODS.values())
    missing = public - used - set(cs.EXCLUDED_METHODS)
    assert not missing, f"DeviceEngine methods neither in a catalogue entry nor excluded with a reason: {sorted(missing)}"

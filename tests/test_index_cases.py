"""CPU checks of tests/index_cases.py: the numpy reference agrees with the oracle's builder and with the product's torch
restatement, the kernel constants the cases are built around are the ones in the sources, and every case meets the claim it
records -- so that tests/test_gpu_index_edges.py, which runs the same cases through the kernels, hits the edges it names."""
import time

import numpy as np
import pytest

import index_cases as ic


def _same(got, want, what):
    for g, w, name in zip(got, want, ("term_off", "post_doc", "post_tf")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


def test_the_constants_the_cases_are_built_around_are_the_kernels():
    c = ic.constants()
    assert c["CH"] == ic.CH == 4096 and c["RB"] == ic.RB == 4096 and c["MSR_SCAN_BLOCK"] == ic.SCAN_BLOCK == 4096
    assert c["MERGE_TILE"] == ic.MERGE_TILE == 2048 and c["COMPACT_TILE"] == ic.COMPACT_TILE == 2048


def test_ref_build_by_hand():
    off, doc, tf = ic.ref_build([0, 3, 3, 7], [2, 0, 2, 1, 2, 2, 0], 4)
    assert off.tolist() == [0, 2, 3, 5, 5] and doc.tolist() == [0, 2, 2, 0, 2] and tf.tolist() == [1, 1, 1, 2, 2]
    assert off.dtype == np.int64 and doc.dtype == np.int32 and tf.dtype == np.int32
    off, doc, tf = ic.ref_build([0, 0], [], 3)
    assert off.tolist() == [0, 0, 0, 0] and len(doc) == len(tf) == 0


@pytest.mark.parametrize("name", ["radix_P65_whole", "radix_P1025_split", "passes_V257"])
def test_ref_build_equals_the_oracle_builder(name):
    """oracle/build_ref.index_from_tokens over string tokens; ref_build over the same tokens in the oracle's numbering."""
    from oracle import build_ref
    case = dict(ic.small_build_cases())[name]()
    toks = [[f"w{t}" for t in case.tok_ids[a:b]] for a, b in zip(case.tok_off[:-1], case.tok_off[1:])]
    ref = build_ref.index_from_tokens(np.arange(case.n_docs), toks)
    ids = np.array([ref["vocab"][w] for tl in toks for w in tl], np.int32)
    _same(ic.ref_build(case.tok_off, ids, len(ref["vocab"])), (ref["term_off"], ref["post_doc"], ref["post_tf"]), name)
    assert np.array_equal(ref["doc_len"], np.diff(case.tok_off))


@pytest.mark.parametrize("name", [n for n, _ in ic.small_build_cases() if not n.startswith("passes_")])
def test_ref_build_equals_the_torch_restatement(name):
    from msretr.index_build import bm25_index_from_token_ids
    case = dict(ic.small_build_cases())[name]()
    ix = bm25_index_from_token_ids(np.arange(case.n_docs), case.tok_off, case.tok_ids, case.n_terms, device="cpu")
    assert ix.total_docs == case.n_docs                     # no token-less document: the numbering is the corpus's own
    _same(ic.ref_build(case.tok_off, case.tok_ids, case.n_terms), (ix.term_off.numpy(), ix.post_doc.numpy(), ix.post_tf.numpy()),
          name)


def _claims(case):
    """(chunks per document, entries before the chunk merge, postings, radix passes) recomputed from the tokens."""
    lens = np.diff(case.tok_off)
    chunks = -(-lens // ic.constants()["CH"])
    first = np.concatenate([[0], np.cumsum(chunks)[:-1]])
    chunk_of = np.repeat(first, lens) + (np.arange(case.tok_off[-1]) - np.repeat(case.tok_off[:-1], lens)) // ic.CH
    p_pre = len(np.unique(chunk_of.astype(np.int64) * case.n_terms + case.tok_ids))
    bits = 0
    while (1 << bits) < case.n_terms:
        bits += 1
    return chunks, p_pre, int(ic.ref_build(case.tok_off, case.tok_ids, case.n_terms)[0][-1]), (bits + 7) // 8


def _meets_its_claims(case):
    assert (np.diff(case.tok_off) > 0).all() and case.tok_ids.min() >= 0 and case.tok_ids.max() < case.n_terms
    chunks, p_pre, p_post, passes = _claims(case)
    assert np.array_equal(chunks, case.chunks) and (p_pre, p_post, passes) == (case.p_pre, case.p_post, case.passes), case.name
    assert (p_pre > p_post) <= case.split


@pytest.mark.parametrize("name", [n for n, _ in ic.small_build_cases()])
def test_every_build_case_meets_its_claims(name):
    case = dict(ic.small_build_cases())[name]()
    _meets_its_claims(case)
    assert case.name == name


def test_chunk_edge_corpus_holds_what_it_names():
    case = ic.chunk_edge_corpus()
    lens = np.diff(case.tok_off)
    term_off, post_doc, post_tf = ic.ref_build(case.tok_off, case.tok_ids, case.n_terms)
    for L in ic.CHUNK_EDGE_LENGTHS:
        assert lens[case.notes[f"len{L}"]] == L
    assert post_doc[:term_off[1]].tolist() == list(range(case.n_docs))                  # term 0 in every document
    d = case.notes["one_term"]
    assert lens[d] == 12289 == post_tf[d] and case.chunks[d] == 4
    assert set(case.tok_ids[case.tok_off[d]:case.tok_off[d + 1]].tolist()) == {0}
    d = case.notes["all_distinct"]
    assert lens[d] == ic.CH == len(set(case.tok_ids[case.tok_off[d]:case.tok_off[d + 1]].tolist()))
    d = case.notes["len4097"]
    assert case.tok_ids[case.tok_off[d + 1] - 1] in case.tok_ids[case.tok_off[d]:case.tok_off[d] + ic.CH]
    assert term_off[case.n_terms] - term_off[case.n_terms - 1] >= 3                     # the last term id occurs
    assert case.split and case.p_pre > case.p_post and case.passes == 2


def test_radix_edge_corpora_hit_their_posting_counts():
    c = ic.constants()
    assert {c["RB"], c["RB"] // 4, 64} <= set(ic.RADIX_EDGE_P)
    for edge in (64, c["RB"] // 4, c["RB"]):
        assert {edge - 1, edge, edge + 1} <= set(ic.RADIX_EDGE_P)
    assert {2 * c["RB"] - 1, 2 * c["RB"] + 1, 37 * c["RB"] + 5} <= set(ic.RADIX_EDGE_P)
    for P in ic.RADIX_EDGE_P:
        whole, split = ic.radix_edge_corpus(P, False), ic.radix_edge_corpus(P, True)
        assert not whole.split and whole.p_pre == whole.p_post == P
        assert split.split and split.p_post == P and split.p_pre == P + 1


def test_pass_count_corpora_cover_0_to_4_passes_and_both_ends_of_the_vocabulary():
    want = {1: 0, 2: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, 1 << 24: 3, (1 << 24) + 1: 4}
    assert set(ic.PASS_COUNT_TERMS) == set(want)
    for V in ic.PASS_COUNT_TERMS:
        case = ic.pass_count_corpus(V)
        assert case.passes == want[V] and 1000 <= case.p_post == case.p_pre <= 10_000
        used = np.unique(case.tok_ids)
        assert used[0] == 0 and used[-1] == V - 1
        if case.passes >= 2:                            # ids that differ only in the byte of the last pass
            shift = 8 * (case.passes - 1)
            low = used & ((1 << shift) - 1)
            assert max(len(set((used[low == v] >> shift).tolist())) for v in (0, 5, 0xAB)) >= min(((V - 1) >> shift) + 1, 40)


def test_scale_corpus_is_above_three_scan_levels_and_its_reference_is_affordable():
    case = ic.scale_corpus()
    t0 = time.perf_counter()
    _meets_its_claims(case)
    took = time.perf_counter() - t0
    block = ic.constants()["MSR_SCAN_BLOCK"]
    assert case.p_post > block * block and case.split and case.passes == 2
    d = case.notes["long_doc"]
    assert 8500 <= np.diff(case.tok_off)[d] <= 9500 and case.chunks[d] == 3
    assert took < 60, f"reference and claims of the scale corpus took {took:.1f} s"


def test_merge_and_compact_shapes_hit_their_tile_edges():
    for P in ic.MERGE_EDGE_P:
        a, a_map, b, b_map, V, n_docs, a_docs = ic.merge_edge_case(P, "interleaved")
        assert int(a[0][-1] + b[0][-1]) == P and len(a_map) == a_docs and len(a_map) + len(b_map) == n_docs
    assert {ic.MERGE_TILE + d for d in (-1, 0, 1)} | {2 * ic.MERGE_TILE + d for d in (-1, 0, 1)} <= set(ic.MERGE_EDGE_P)
    for P in ic.COMPACT_EDGE_P:
        assert int(ic.table(np.random.default_rng(P), 3000, 900, P)[0][-1]) == P
    a, _, b, _, V, _, na = ic.merge_head_case("appended")
    assert a[0][1] == na > 40 * ic.MERGE_TILE and b[0][100] == b[0][1] and b[0][-1] > b[0][len(a[0]) - 1] and V > len(b[0]) - 1
    a, _, b, _, V, _, _ = ic.merge_one_posting_case()
    assert np.median(np.diff(a[0])[np.diff(a[0]) > 0]) == 1 and b[0][len(a[0]) - 1] == 0

"""The fuse contract on the CPU: rerank_ref.fuse_from_gather -- what the fuse kernel gets
and returns -- pinned bit for bit to the reference's pooled stage, and the case set of tests/rerank_cases.py shown to have
teeth: every restated wrong fuse, and every restated wrong gather, fails on it.  No GPU."""
import numpy as np
import pytest

import rerank_cases as RC
from oracle import rerank_ref


@pytest.fixture(scope="module")
def cases():
    return RC.fuse_cases()


@pytest.mark.parametrize("f", RC.fixture_cases(), ids=lambda f: f"case{f['case']}")
def test_fuse_from_gather_equals_the_fixture(f):
    """cos / meta built from the reference's own cosines (shuffled slots, garbage past cand_n) -> the reference's pooled
    stage: documents in order (equal scores ascending, which the fixture leaves open), scores, normalised BM25 and winning
    chunk, all ==."""
    c = RC.fixture_fuse_case(f)
    doc, score, orig, chunk, n, rows = RC.fuse_ref(c)
    assert n == len(f["docs"]) and rows == sum(f["n_rows"])
    ranked = f["stages"][-1]
    assert score[:n].tolist() == ranked["new_similarity"]
    exp = sorted(zip(ranked["new_similarity"], ranked["doc_id"], ranked["old_similarity"], ranked["chunk_id"]),
                 key=lambda t: (-t[0], t[1]))
    got = list(zip(score[:n].tolist(), doc[:n].tolist(), orig[:n].tolist(), [f["chunk_id"][x] for x in chunk[:n]]))
    assert got == exp
    assert (doc[n:] == -1).all() and np.isneginf(score[n:]).all() and (chunk[n:] == -1).all() and (orig[n:] == 0).all()


def test_chain_defaults_unchanged():
    """max_boost / max_decay keywords default to the reference's constants."""
    v = [0.2, 0.9, 0.4]
    assert rerank_ref.positional_adjust(v, 3) == rerank_ref.positional_adjust(v, 3, 0.1, 0.05)
    assert rerank_ref.positional_adjust(v, 3, 0.5, 0.0)[1] == 1.0
    assert rerank_ref.positional_adjust(v, 3, 0.0, 0.0) == v


def test_restatement_agrees(cases):
    """wrong_fuse without a mistake is the fuse: the negative controls below differ from it in their mistake only."""
    for c in cases:
        assert RC.same_fuse(RC.wrong_fuse(c, None), RC.fuse_ref(c)), c["name"]


@pytest.mark.parametrize("bug", RC.BUGS)
def test_every_wrong_fuse_fails_a_case(cases, bug):
    hit = [c["name"] for c in cases if not RC.same_fuse(RC.wrong_fuse(c, bug), RC.fuse_ref(c))]
    assert hit, f"no case tells the fuse from one with mistake {bug}"


def test_case_set_covers_the_edges(cases):
    names = {c["name"] for c in cases}
    for want in ("n_1", "n_63", "n_64", "n_65", "n_511", "n_512", "n_513", "n_1000", "n_1024", "cand_n_above_M",
                 "none_kept", "one_kept", "all_cos_equal", "all_bm25_equal", "both_equal", "equal_final_scores",
                 "group_min_without_rows", "url_group_minus_one", "duplicate_slots_0"):
        assert want in names
    out = {c["name"]: RC.fuse_ref(c) for c in cases}
    assert out["none_kept"][4] == 0 and out["none_kept"][5] == 0
    assert out["one_kept"][4] == 1 and out["one_kept"][0][0] == 50
    eq = out["equal_final_scores"]
    assert eq[4] == RC.M and len(set(eq[1][1:RC.M - 1].tolist())) == 1
    assert (np.diff(eq[0][1:RC.M - 1]) > 0).all()
    # the duplicate-slot cases: the first slot's BM25 is what counts
    for c in cases:
        if c["name"].startswith("duplicate_slots"):
            first = {}
            for m in range(c["n"]):
                first.setdefault(int(c["doc"][m]), float(c["bm"][m]))
            assert len(first) < c["n"]
    # the cand_n > M case reads all M slots
    assert out["cand_n_above_M"][4] > 0


def test_wrong_gathers_exceed_the_bar():
    """The gather bar (tests/test_gpu_rerank.py) separates the f32 gather from what a faster wrong gather would return: cosines
    from f16- or bf16-rounded rows, from the neighbouring document's row, or without the row's inv_norm each exceed the bar
    on the test's corpus.  (The restated f32 gather itself must stay inside it: float64 of the f32 inputs.)"""
    z = RC.gather_corpus()
    E, q = z["emb"], z["queries"]
    c, A = RC.cos64(q, E)
    bar = RC.gather_bar(A, c)
    assert (np.abs(RC.gather_restated(q, E) - c) <= bar).all()
    for kw in (dict(rows="f16"), dict(rows="bf16"), dict(shift=1), dict(inv="none")):
        err = np.abs(RC.gather_restated(q, E, **kw) - c)
        assert (err > bar).any(), kw

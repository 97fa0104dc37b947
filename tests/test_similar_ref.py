"""The exactness argument of msr_dense_topk_grouped on the host: the top k of a group's per-document maximum equals the merge of
its rows' top (k + |excl_g|) lists, ties included (similar_ref.py)."""
import numpy as np
import pytest

from similar_ref import brute_force, dense_scores, merge_lists, row_lists


def _case(rng, R, N, quant=None, dup_rows=(), chunkless=0.1):
    S = rng.standard_normal((R, N))
    if quant:
        S = np.round(S * quant) / quant                         # few distinct values: ties within and across rows
    S[:, rng.random(N) < chunkless] = -np.inf                   # chunk-less documents score nowhere
    for a, b in dup_rows:
        S[b] = S[a]
    C = rng.integers(0, 10 * N, size=(R, N))
    return S, C


def _groups(rng, R, G):
    cut = np.sort(rng.integers(0, R + 1, size=G - 1))
    return np.concatenate([[0], cut, [R]]).astype(np.int64)


def _check(S, C, goff, excl, k, min_score=-np.inf, depth="group"):
    want = brute_force(S, C, goff, excl, k, min_score)
    if depth == "group":                                        # each row's list only as deep as its group needs
        R = S.shape[0]
        got_rows = [None] * R
        for g in range(len(goff) - 1):
            need = k + len(excl[g])
            for r in range(goff[g], goff[g + 1]):
                d, s, c, n = row_lists(S[r:r + 1], C[r:r + 1], need)
                got_rows[r] = (d[0], s[0], c[0], n[0])
        kk = max([k + len(e) for e in excl])
        doc = np.full((R, kk), -1); sc = np.full((R, kk), -np.inf); ch = np.full((R, kk), -1); n = np.zeros(R, int)
        for r, (d, s, c, m) in enumerate(got_rows):
            doc[r, :len(d)], sc[r, :len(s)], ch[r, :len(c)], n[r] = d, s, c, m
    else:                                                       # one depth for all rows: k + max |excl_g| (the engine's call)
        doc, sc, ch, n = row_lists(S, C, k + max(len(e) for e in excl))
    got = merge_lists(doc, sc, ch, n, goff, excl, k, min_score)
    assert got == want


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("depth", ["group", "call"])
def test_merge_of_row_lists_equals_brute_force(seed, depth):
    rng = np.random.default_rng(seed)
    R, N, G = int(rng.integers(1, 30)), int(rng.integers(5, 300)), int(rng.integers(1, 6))
    S, C = _case(rng, R, N, quant=[None, 2, 8][seed % 3])
    goff = _groups(rng, R, G)
    excl = [rng.choice(N, size=int(rng.integers(0, 6)), replace=False).tolist() for _ in range(G)]
    k = int(rng.integers(1, N + 5))
    _check(S, C, goff, excl, k, depth=depth)


def test_exact_ties_duplicate_rows_and_equal_maxima():
    rng = np.random.default_rng(100)
    S, C = _case(rng, 8, 40, quant=1, dup_rows=[(0, 3), (1, 2)])
    S[5, 7] = S[6, 7] = 9.0                                     # equal maxima of one document from two rows: row 5 wins
    want = brute_force(S, C, [0, 8], [[]], 10)
    assert want[0][0][:2] == (7, 9.0) and want[0][0][3] == 5
    for k in (1, 3, 10, 40, 60):
        _check(S, C, np.array([0, 4, 8]), [[], [7]], k)
        _check(S, C, np.array([0, 4, 8]), [[], [7]], k, depth="call")


def test_all_rows_the_same_and_every_document_tied():
    S = np.zeros((6, 50))                                       # every row lists the same documents, every score equal
    C = np.arange(300).reshape(6, 50)
    got = brute_force(S, C, [0, 6], [[0, 1]], 10)
    assert [t[0] for t in got[0]] == list(range(2, 12)) and all(t[3] == 0 for t in got[0])
    _check(S, C, np.array([0, 6]), [[0, 1]], 10)


def test_exclusion_min_score_empty_groups_and_k_past_the_eligible():
    rng = np.random.default_rng(7)
    S, C = _case(rng, 10, 30, chunkless=0.3)
    goff = np.array([0, 0, 4, 4, 10, 10])                       # empty groups at the front, inside and at the back
    excl = [[1], [0, 2, 5], [], [3], []]
    for k in (1, 5, 30, 100):
        for ms in (-np.inf, 0.0, 1.0, 5.0):
            _check(S, C, goff, excl, k, ms)
            _check(S, C, goff, excl, k, ms, depth="call")
    got = merge_lists(*row_lists(S, C, 100 + 3), goff, excl, 100)
    assert got[0] == [] and got[2] == [] and got[4] == []
    elig = np.isfinite(S[4:10]).any(axis=0)
    elig[3] = False
    assert len(got[3]) == int(elig.sum())                       # k past the eligible count returns all of them
    for g, e in enumerate(excl):
        assert not set(e) & {t[0] for t in got[g]}


def test_dense_scores_per_document_maximum():
    rng = np.random.default_rng(1)
    doc_off = np.array([0, 2, 2, 5, 6])
    emb = rng.standard_normal((6, 768))
    emb[4] = 0.0                                                # a zero row: cosine 0
    q = np.stack([emb[3] * 2.0, np.zeros(768)])
    S, A = dense_scores(emb, doc_off, q)
    assert np.isneginf(S[:, 1]).all() and A[0, 2] == 3 and abs(S[0, 2] - 1.0) < 1e-12
    assert (S[1, [0, 2, 3]] == 0.0).all() and A[1, 0] == 0      # a zero query: every cosine 0, the first row wins

"""The similar-documents contract (msr_dense_topk_grouped) stated in numpy, for test_similar_ref.py and test_gpu_similar.py.

Group g of query rows scores a document d by S_g(d) = max over its rows r of score_r(d); the group's result is the top k of
the documents outside excl_g with S_g(d) >= min_score, ordered by (score desc, doc asc); each entry names the row that gave
the maximum (the lowest among equal maxima) and that row's arg-max chunk.  No import of the package's device code."""
import numpy as np


def row_topk(scores, kk):
    """One row's dense list: the kk best documents by (score desc, doc asc) among finite scores (-inf = a chunk-less document).
    -> doc indices (int64 array)."""
    s = np.asarray(scores)
    d = np.nonzero(np.isfinite(s))[0]
    order = np.lexsort((d, -s[d]))
    return d[order][:kk]


def row_lists(scores, chunks, kk):
    """Per-row lists of depth kk from a score matrix [R, N] and an arg-max chunk matrix [R, N] (what msr_dense_topk returns
    for R query rows): -> (doc [R, kk], score [R, kk], chunk [R, kk], n [R]), padded with -1 / -inf / -1."""
    R = scores.shape[0]
    doc = np.full((R, kk), -1, np.int64)
    sc = np.full((R, kk), -np.inf, scores.dtype)
    ch = np.full((R, kk), -1, np.int64)
    n = np.zeros(R, np.int64)
    for r in range(R):
        d = row_topk(scores[r], kk)
        n[r] = len(d)
        doc[r, :len(d)], sc[r, :len(d)], ch[r, :len(d)] = d, scores[r, d], chunks[r, d]
    return doc, sc, ch, n


def merge_lists(doc, score, chunk, n, group_off, exclude, k, min_score=-np.inf):
    """The host merge: per group every entry of its rows' lists, the best per document (lowest row among equal scores), the
    excluded documents and scores below min_score dropped, top k by (score desc, doc asc).
    -> list per group of (doc, score, chunk, src_row) tuples."""
    out = []
    for g in range(len(group_off) - 1):
        best = {}
        for r in range(int(group_off[g]), int(group_off[g + 1])):
            for j in range(int(n[r])):
                d, s = int(doc[r, j]), score[r, j]
                cur = best.get(d)
                if cur is None or s > cur[0]:                   # rows visited in ascending order: equal scores keep the lowest
                    best[d] = (s, int(chunk[r, j]), r)
        ex = set(int(x) for x in exclude[g])
        res = [(d, s, c, r) for d, (s, c, r) in best.items() if d not in ex and s >= min_score]
        res.sort(key=lambda t: (-t[1], t[0]))
        out.append(res[:k])
    return out


def brute_force(scores, chunks, group_off, exclude, k, min_score=-np.inf):
    """The definition on the full score matrix [R, N]: S_g(d) over every document.  -> the same shape as merge_lists."""
    out = []
    N = scores.shape[1]
    for g in range(len(group_off) - 1):
        r0, r1 = int(group_off[g]), int(group_off[g + 1])
        if r1 == r0:
            out.append([])
            continue
        blk = scores[r0:r1]
        S = blk.max(axis=0)
        ex = set(int(x) for x in exclude[g])
        res = []
        for d in range(N):
            if d in ex or not np.isfinite(S[d]) or not S[d] >= min_score:
                continue
            r = r0 + int(np.nonzero(blk[:, d] == S[d])[0][0])  # the lowest row reaching the maximum
            res.append((d, S[d], int(chunks[r, d]), r))
        res.sort(key=lambda t: (-t[1], t[0]))
        out.append(res[:k])
    return out


def dense_scores(emb, doc_off, q):
    """float64 cosines: [R, N] per-document maximum over its chunks (-inf without chunks) and the first arg-max chunk row.
    Zero rows and zero queries have norm 1 (sklearn normalize)."""
    e = np.asarray(emb, np.float64)
    en = np.linalg.norm(e, axis=1)
    e = e / np.where(en == 0, 1.0, en)[:, None]
    qq = np.asarray(q, np.float64)
    qn = np.linalg.norm(qq, axis=1)
    qq = qq / np.where(qn == 0, 1.0, qn)[:, None]
    cos = qq @ e.T
    off = np.asarray(doc_off, np.int64)
    N = len(off) - 1
    S = np.full((len(qq), N), -np.inf)
    A = np.full((len(qq), N), -1, np.int64)
    for d in range(N):
        a, b = off[d], off[d + 1]
        if b > a:
            blk = cos[:, a:b]
            A[:, d] = a + blk.argmax(axis=1)
            S[:, d] = blk.max(axis=1)
    return S, A

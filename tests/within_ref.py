"""The restricted-search contract stated on the oracle's full lists (imported by test_docset.py and test_gpu_within.py)."""
import numpy as np


def restrict_list(doc, score, n, mask, k):
    """One query's FULL unrestricted list (every accepted document, in the unrestricted order) -> the restricted top k: its
    first k entries whose document is in the set `mask` (bool [N]).  -> (doc, score) arrays of length <= k."""
    doc, score = np.asarray(doc)[:int(n)], np.asarray(score)[:int(n)]
    keep = np.asarray(mask, bool)[doc.astype(np.int64)] if len(doc) else np.zeros(0, bool)
    return doc[keep][:k], score[keep][:k]


def bm25_full(z, terms, min_score=0.0, k1=1.2, b=0.75):
    """Every accepted document of one query, in the unrestricted order, from the oracle (bm25_ref.topk with k = N)."""
    from oracle import bm25_ref
    N = len(z["doc_ids"])
    return bm25_ref.topk(z, terms, max(N, 1), min_score, k1, b)

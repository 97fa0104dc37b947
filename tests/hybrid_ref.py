"""The hybrid candidate list and the hybrid step on the CPU, composed from the oracle (imported by test_hybrid_ref.py and
test_gpu_hybrid.py): BM25 top k_lex (oracle.bm25_ref.topk), dense top dense_k (oracle.dense_ref.quick_search), the dense-only
documents scored with the BM25 sum of oracle.bm25_ref.scores_dense, the joined list through the rerank chain of
oracle.rerank_ref (via OracleEngine).  Numpy only."""
import numpy as np

from oracle import bm25_ref, dense_ref

SRC_LEXICAL, SRC_DENSE, SRC_BOTH = 1, 2, 3


def k_lex(top_k, rerank_max_docs, dense_k):
    """Lexical candidates of a hybrid step: the chain holds <= rerank_max_docs candidates, dense_k are the dense stage's."""
    if dense_k < 1:
        raise ValueError("dense_k < 1")
    k = min(int(top_k), int(rerank_max_docs) - int(dense_k))
    if k < 1:
        raise ValueError("no room for lexical candidates")
    return k


def point_scores(z, terms, docs, k1=1.2, b=0.75):
    """-> (score float64 [len(docs)], touched bool [len(docs)]): the reference's BM25 sum of each named document for the query
    `terms` (term ids with repeats / unknown ids); a document outside [0, N) gets 0.0 / False."""
    docs = np.asarray(docs, np.int64).reshape(-1)
    N = len(z["doc_len"])
    ut, qtf = bm25_ref.prepare_query(terms, z["term_off"])
    acc, touched = bm25_ref.scores_dense(z, ut, qtf, k1, b)
    ok = (docs >= 0) & (docs < N)
    d = np.where(ok, docs, 0)
    return np.where(ok, acc[d], 0.0), ok & touched[d]


def union_list(lex_doc, lex_score, dense_doc, dense_bm25):
    """One query.  The lexical list unchanged and in its order, then the dense list's documents that are not in it, in dense
    rank order, each with its score dense_bm25[j]; dense entries < 0 or repeating an earlier dense entry are skipped.
    -> (doc int32, score float64, src int32: 1 lexical only, 2 dense only, 3 both)."""
    lex_doc = [int(d) for d in lex_doc]
    in_dense = {int(d) for d in dense_doc if int(d) >= 0}
    doc, score = list(lex_doc), [float(s) for s in lex_score]
    src = [SRC_BOTH if d >= 0 and d in in_dense else SRC_LEXICAL for d in lex_doc]
    seen = set(lex_doc)
    for d, s in zip(dense_doc, dense_bm25):
        d = int(d)
        if d < 0 or d in seen:
            continue
        seen.add(d)
        doc.append(d); score.append(float(s)); src.append(SRC_DENSE)
    return np.asarray(doc, np.int32), np.asarray(score, np.float64), np.asarray(src, np.int32)


def pad_lists(lists, width):
    """[(doc, score, src)] per query -> arrays [Q, width] padded with -1 / -inf / 0, and n [Q]."""
    Q = len(lists)
    doc = np.full((Q, width), -1, np.int32); score = np.full((Q, width), -np.inf); src = np.zeros((Q, width), np.int32)
    n = np.zeros(Q, np.int32)
    for q, (d, s, r) in enumerate(lists):
        assert len(d) <= width
        doc[q, :len(d)], score[q, :len(d)], src[q, :len(d)], n[q] = d, s, r, len(d)
    return doc, score, src, n


def candidates(z, emb, doc_off, terms, qvec, top_k, rerank_max_docs, dense_k, k1=1.2, b=0.75, mask=None):
    """The hybrid candidate list of one query from the oracle alone.  mask (bool [N], optional): both stages restricted to
    the documents of the set (the full lists filtered, as within_ref.restrict_list does)."""
    kl = k_lex(top_k, rerank_max_docs, dense_k)
    N = len(z["doc_len"])
    if mask is None:
        ld, ls = bm25_ref.topk(z, terms, kl, 0.0, k1, b)
        dd, _, _ = dense_ref.quick_search(emb, doc_off, qvec, dense_k)
    else:
        fd, fs = bm25_ref.topk(z, terms, max(N, 1), 0.0, k1, b)
        keep = np.asarray(mask, bool)[fd]
        ld, ls = fd[keep][:kl], fs[keep][:kl]
        ad, _, _ = dense_ref.quick_search(emb, doc_off, qvec, N)
        dd = ad[np.asarray(mask, bool)[ad]][:dense_k]
    ds, _ = point_scores(z, terms, dd, k1, b)
    return union_list(ld, ls, dd, ds)


def fused(oracle_engine, cand_doc, cand_score, cand_n, qvec, smoothing=0.15, max_chunks=10):
    """The rerank chain on the CPU (OracleEngine.rerank_gather + rerank_fuse = oracle.rerank_ref) for padded candidate lists."""
    import torch
    cos, meta = oracle_engine.rerank_gather(torch.as_tensor(np.asarray(qvec, np.float32)), cand_doc, cand_n, max_chunks=max_chunks)
    return oracle_engine.rerank_fuse(cand_doc, cand_score, cand_n, cos, meta, smoothing=smoothing, max_chunks=max_chunks)

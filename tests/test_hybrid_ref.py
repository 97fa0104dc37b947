"""Hybrid candidates without a GPU: the CPU helper (tests/hybrid_ref.py) on hand-made cases, the capacity rule, and the two
new entry points in the header, the ctypes table and the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

import hybrid_ref as H
from oracle import bm25_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msr_bm25_score_docs", "msr_union_candidates")


def _tiny():
    # 6 documents, 3 terms: term 0 in documents 0..4 (negative idf), term 1 in 1 and 3, term 2 in 5
    postings = {"a": [(10, 1), (11, 2), (12, 1), (13, 3), (14, 1)], "b": [(11, 1), (13, 2)], "c": [(15, 4)]}
    doc_len = {10: 5, 11: 7, 12: 3, 13: 9, 14: 4, 15: 6}
    idf = {"a": -0.6, "b": 0.5, "c": 0.8}
    return bm25_ref.index_from_tables(postings, doc_len, idf, 5.5)


def test_union_order_sources_and_scores():
    doc, score, src = H.union_list([7, 3, 9], [5.0, 4.0, 1.0], [3, 20, -1, 20, 7, 11], [40.0, -0.25, 9.0, 8.0, 50.0, 0.0])
    assert doc.tolist() == [7, 3, 9, 20, 11]                       # the lexical list in its order, then dense rank order
    assert score.tolist() == [5.0, 4.0, 1.0, -0.25, 0.0]           # lexical scores kept; first place of a repeat counts
    assert src.tolist() == [3, 3, 1, 2, 2]                         # a document of both lists appears once, src 3
    d, s, r = H.union_list([], [], [4, 2], [0.0, 1.5])
    assert d.tolist() == [4, 2] and r.tolist() == [2, 2]
    d, s, r = H.union_list([4, 2], [2.0, 1.0], [], [])
    assert d.tolist() == [4, 2] and r.tolist() == [1, 1] and s.tolist() == [2.0, 1.0]
    d, s, r, n = H.pad_lists([(doc, score, src), (np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int32))], 8)
    assert n.tolist() == [5, 0] and (d[0, 5:] == -1).all() and np.isneginf(s[1]).all() and (r[1] == 0).all()


def test_point_scores_are_the_oracle_sums():
    z, vocab = _tiny()
    terms = [vocab["b"], vocab["a"], vocab["b"], 99, -1]           # b twice (qtf 2), a, two unknown ids
    ut, qtf = bm25_ref.prepare_query(terms, z["term_off"])
    assert ut == [vocab["b"], vocab["a"]] and qtf == [2, 1]
    acc, touched = bm25_ref.scores_dense(z, ut, qtf)
    docs = [5, 1, 0, 1, -1, 6]
    s, t = H.point_scores(z, terms, docs)
    assert s[:4].tolist() == acc[[5, 1, 0, 1]].tolist() and t.tolist() == [False, True, True, True, False, False]
    assert s[0] == 0.0 and s[4] == 0.0 and s[5] == 0.0              # no query term / outside the index: 0.0, not matched
    assert s[2] < 0                                                # the negative-idf term alone: the true (negative) sum
    # the point score of a document the top-k returns is the top-k's score
    d, sc = bm25_ref.topk(z, terms, 10)
    assert H.point_scores(z, terms, d)[0].tolist() == sc.tolist()
    s, t = H.point_scores(z, [-3, 99], [0, 1])
    assert s.tolist() == [0.0, 0.0] and not t.any()


def test_candidates_dense_only_document_without_a_term():
    z, vocab = _tiny()
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((6, 768)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    doc_off = np.arange(7, dtype=np.int64)
    q = emb[5].copy()                                             # document 5 is the dense top hit; it holds term c only
    doc, score, src = H.candidates(z, emb, doc_off, [vocab["b"]], q, top_k=1000, rerank_max_docs=1000, dense_k=2)
    assert doc[:2].tolist() == [3, 1] or doc[:2].tolist() == [1, 3]
    assert 5 in doc.tolist()
    i = doc.tolist().index(5)
    assert score[i] == 0.0 and src[i] == 2 and i >= 2
    assert len(set(doc.tolist())) == len(doc)


def test_capacity_rule():
    from msretr.retriever import hybrid_k_lex
    for top_k, cap, dk in ((1000, 1000, 100), (1000, 1024, 100), (50, 1000, 100), (1000, 1000, 999), (10, 12, 5)):
        want = min(top_k, cap - dk)
        assert H.k_lex(top_k, cap, dk) == want == hybrid_k_lex(top_k, cap, dk)
    assert H.k_lex(1000, 1000, 100) == 900
    for bad in ((1000, 1000, 0), (1000, 1000, 1000), (1000, 100, 200), (1000, 1000, -3)):
        with pytest.raises(ValueError):
            H.k_lex(*bad)
        with pytest.raises(ValueError):
            hybrid_k_lex(*bad)


def test_header_declares_and_abi_binds_both_functions():
    from msretr import _abi
    hdr = open(os.path.join(ROOT, "include", "msretr.h"), encoding="utf-8").read()
    for name in NEW:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
        assert m, f"{name} is not declared in msretr.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _abi._SIGNATURES, f"{name} is not bound in _abi"
        assert len(_abi._SIGNATURES[name][1]) == n_args, (name, n_args, len(_abi._SIGNATURES[name][1]))
    assert len(_abi._SIGNATURES["msr_bm25_score_docs"][1]) == 11 and len(_abi._SIGNATURES["msr_union_candidates"][1]) == 16
    ver = int(re.search(r"#define MSR_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _abi.MSR_ABI_VERSION >= 8


def test_built_library_exports_both_symbols():
    from msretr import _abi
    assert os.path.exists(_abi.LIB_PATH), "build the library first (__graft_entry__.build)"
    lib = _abi.load()
    for name in NEW:
        assert hasattr(lib, name)
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT " + name + r"$", out, flags=re.M), name

#!/usr/bin/env python3
"""Cost of the hybrid candidates (msr_bm25_score_docs, msr_union_candidates; DESIGN K10) at the bench shape: synthetic_corpus
1 M documents / 5 M chunks / 1 M terms, 256 queries, k_lex 900, dense_k 100.  Device events around each call, one warm-up,
median of --iters (>= 10), all in one process from the same library:
  * msr_bm25_score_docs on the dense lists, msr_union_candidates;
  * the yardsticks: msr_bm25_topk (k_lex) of the same queries, and the workaround the point kernel replaces --
    msr_bm25_topk_within with per-query sets of the dense lists and min_score = -inf (device time only: the sets are built
    before the clock starts, the host round trip it needs is not counted);
  * the whole step: Retriever.final_lists lexical, hybrid, and one dense_topk call (host clock around the synchronising call).
Prints one JSON line.
    python tools/hybrid_bench.py [--docs 1000000] [--chunks 5000000] [--queries 256] [--iters 11]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.docset import DocSet  # noqa: E402
from msretr.engine import DeviceEngine  # noqa: E402
from msretr.retriever import Retriever, hybrid_k_lex  # noqa: E402
from msretr.synthetic import SEED, synthetic_corpus, synthetic_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--chunks", type=int, default=5_000_000)
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--top-k", type=int, default=1000)
ap.add_argument("--dense-k", type=int, default=100)
ap.add_argument("--iters", type=int, default=11)
a = ap.parse_args()
assert a.iters >= 10
assert torch.cuda.is_available(), "this benchmark needs the MI355X (no CPU timing stands in for it)"
dev = torch.device("cuda", 0)


def log(*x):
    print(*x, file=sys.stderr, flush=True)


def timed(fn, iters=a.iters):
    """Median device time (ms) of fn() over iters calls, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def wall(fn, iters=a.iters):
    """Median host time (ms) of a call that ends synchronised."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


t0 = time.time()
ix = synthetic_corpus(a.docs, n_chunks=a.chunks, n_terms=a.terms, seed=SEED, device=dev)
terms, qv = synthetic_queries(ix, a.queries, seed=777, device=dev)
log(f"corpus {ix.n_docs} docs, {ix.n_chunks} chunks in {time.time() - t0:.1f}s")
Q = a.queries
eng = DeviceEngine(ix, device=0, max_queries=Q, max_k=a.top_k, rerank_max_docs=a.top_k)
k_lex = hybrid_k_lex(a.top_k, eng.rerank_max_docs, a.dense_k)
packed = eng.pack_queries(terms)
lex = eng.bm25_topk(None, k=k_lex, packed=packed)
dd, _, _, dn = eng.dense_topk(qv, k=a.dense_k, want_chunk=False)
dbm, touched = eng.bm25_score_docs(None, dd, dn, packed=packed)
union = eng.union_candidates(lex, dd, dbm, dn)
torch.cuda.synchronize()
out = {"shape": {"docs": ix.n_docs, "chunks": ix.n_chunks, "queries": Q, "k_lex": k_lex, "dense_k": a.dense_k,
                 "slots": int(dn.sum().item()), "device": torch.cuda.get_device_name(0)}}
out["bm25_score_docs_ms"] = timed(lambda: eng.bm25_score_docs(None, dd, dn, packed=packed))
out["union_candidates_ms"] = timed(lambda: eng.union_candidates(lex, dd, dbm, dn))
out["bm25_topk_ms"] = timed(lambda: eng.bm25_topk(None, k=k_lex, packed=packed))
# the workaround: restricted top-k over per-query sets of the dense lists, every list streamed (min_score < 0)
dd_h, dn_h = dd.cpu().numpy(), dn.cpu().numpy()
sets = []
for q in range(Q):
    m = np.zeros(ix.n_docs, bool)
    m[dd_h[q, :dn_h[q]]] = True
    sets.append(DocSet.from_mask(ix, m))
bits, q_set, n_sets, stride = eng.pack_within(sets, Q)
eng.pack_within = lambda within, n: (bits, q_set, n_sets, stride)      # (the sets are on the device before the clock starts)
wa = eng.bm25_topk(None, k=a.dense_k, min_score=-float("inf"), packed=packed, within=sets)
out["workaround_within_ms"] = timed(lambda: eng.bm25_topk(None, k=a.dense_k, min_score=-float("inf"), packed=packed, within=sets))
del eng.pack_within
# the workaround returns the same sums (for the documents of the dense list that hold a query term)
wd, ws, wn = [x.cpu().numpy() for x in wa]
ps, pt = dbm.cpu().numpy(), touched.cpu().numpy()
agree = True
for q in range(Q):
    look = dict(zip(wd[q, :wn[q]].tolist(), ws[q, :wn[q]].tolist()))
    for j in range(int(dn_h[q])):
        if pt[q, j]:
            agree &= look.get(int(dd_h[q, j])) == float(ps[q, j])
out["workaround_agrees_bit_for_bit"] = bool(agree)
# the whole step
r = Retriever(indexer=eng)
qv_h = qv
out["final_lists_lexical_ms"] = wall(lambda: r.final_lists(terms, qv_h, a.top_k))
out["final_lists_hybrid_ms"] = wall(lambda: r.final_lists(terms, qv_h, a.top_k, mode="hybrid", dense_k=a.dense_k))
out["dense_topk_ms"] = timed(lambda: eng.dense_topk(qv, k=a.dense_k, want_chunk=False))
out["lexical_plus_dense_ms"] = out["final_lists_lexical_ms"] + out["dense_topk_ms"]
n = union[3].cpu().numpy()
src = union[2].cpu().numpy()
out["candidates_per_query"] = float(n.mean())
out["dense_only_per_query"] = float((src == 2).sum() / Q)
print(json.dumps(out))
eng.close()

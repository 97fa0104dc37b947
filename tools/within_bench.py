#!/usr/bin/env python3
"""Cost of document sets (msr_bm25_topk_within / msr_dense_topk_within) at the bench shape: synthetic_corpus 1 M documents /
5 M chunks / 1 M terms, 256 queries, top-1000.  Device events around each call (median of --iters):
  * BM25 (scoring kernel + select) unrestricted vs restricted to random sets of density 1, 0.5, 0.05, 0.001;
  * restricted dense top-100 per 64 queries (the sweeps) next to the unrestricted 256-query call;
  * one Retriever.search restricted to a site:-sized set (~0.1 % of the corpus), wall clock.
Prints one JSON line.
    python tools/within_bench.py [--docs 1000000] [--chunks 5000000] [--queries 256] [--iters 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.docset import DocSet  # noqa: E402
from msretr.engine import DeviceEngine  # noqa: E402
from msretr.retriever import Retriever  # noqa: E402
from msretr.synthetic import SEED, synthetic_corpus, synthetic_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--chunks", type=int, default=5_000_000)
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--k", type=int, default=1000)
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda", 0)


def log(*x):
    print(*x, file=sys.stderr, flush=True)


def timed(fn, iters):
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


t0 = time.time()
ix = synthetic_corpus(a.docs, n_chunks=a.chunks, n_terms=a.terms, seed=SEED, device=dev)
terms, qv = synthetic_queries(ix, a.queries, seed=777, device=dev)
log(f"corpus {ix.n_docs} docs, {ix.n_chunks} chunks in {time.time() - t0:.1f}s")
Q = a.queries
eng = DeviceEngine(ix, device=0, max_queries=Q, max_k=a.k, rerank_max_docs=a.k)
packed = eng.pack_queries(terms)
rng = np.random.default_rng(1)
out = {"docs": ix.n_docs, "chunks": ix.n_chunks, "queries": Q, "k": a.k, "device": torch.cuda.get_device_name(0)}

# BM25: the library calls themselves (sets packed beforehand), and the scoring kernel alone (the engine's own event pairs)
q_off, q_terms, q_qtf, _ = packed
o_doc = torch.empty((Q, a.k), dtype=torch.int32, device=dev)
o_score = torch.empty((Q, a.k), dtype=torch.float64, device=dev)
o_n = torch.empty((Q,), dtype=torch.int32, device=dev)
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)


def bm25_call(bits=None, q_set=None, n_sets=0, stride=0):
    if n_sets == 0:
        rc = eng.lib.msr_bm25_topk(eng.handle, P(q_off), P(q_terms), P(q_qtf), Q, a.k, C.c_double(0.0), P(o_doc), P(o_score),
                                   P(o_n), eng._stream())
    else:
        rc = eng.lib.msr_bm25_topk_within(eng.handle, P(q_off), P(q_terms), P(q_qtf), Q, a.k, C.c_double(0.0), P(bits), n_sets,
                                          stride, P(q_set), P(o_doc), P(o_score), P(o_n), eng._stream())
    assert rc == 0, rc


def taat_ms(fn):
    eng.set_timing(True)
    for _ in range(a.iters):
        fn()
    torch.cuda.synchronize()
    ms, n = eng.kernel_time_ms(1)
    eng.set_timing(False)
    return ms / max(n, 1)


out["bm25_ms"] = timed(bm25_call, a.iters)
out["bm25_taat_ms"] = taat_ms(bm25_call)
for dens in (1.0, 0.5, 0.05, 0.001):
    ds = DocSet.from_mask(ix, rng.random(ix.n_docs) < dens if dens < 1 else np.ones(ix.n_docs, bool))
    bits, q_set, n_sets, stride = eng.pack_within(ds, Q)
    call = lambda: bm25_call(bits, q_set, n_sets, stride)
    out[f"bm25_within_{dens}_ms"] = timed(call, a.iters)
    out[f"bm25_within_{dens}_taat_ms"] = taat_ms(call)
    out[f"bm25_within_{dens}_facade_ms"] = timed(lambda: eng.bm25_topk(None, k=a.k, packed=packed, within=ds), a.iters)
    log(f"bm25 density {dens}: {out[f'bm25_within_{dens}_ms']:.3f} ms (kernel {out[f'bm25_within_{dens}_taat_ms']:.3f}) vs "
        f"{out['bm25_ms']:.3f} ms (kernel {out['bm25_taat_ms']:.3f}) unrestricted")

q64 = qv[:64].contiguous()
out["dense_path_unrestricted_256"] = None
out["dense_256_ms"] = timed(lambda: eng.dense_topk(qv, k=100), a.iters)
out["dense_path_unrestricted_256"] = eng.dense_path()
out["dense_64_ms"] = timed(lambda: eng.dense_topk(q64, k=100), a.iters)
ds = DocSet.from_mask(ix, rng.random(ix.n_docs) < 0.05)
ds.to(dev)
out["dense_within_64_ms"] = timed(lambda: eng.dense_topk(q64, k=100, within=ds), a.iters)
bits, q_set, n_sets, stride = eng.pack_within(ds, 64)
d_doc = torch.empty((64, 100), dtype=torch.int32, device=dev)
d_score = torch.empty((64, 100), dtype=torch.float32, device=dev)
d_chunk = torch.empty((64, 100), dtype=torch.int32, device=dev)
d_n = torch.empty((64,), dtype=torch.int32, device=dev)
out["dense_within_64_lib_ms"] = timed(lambda: eng.lib.msr_dense_topk_within(
    eng.handle, P(q64), 64, 100, 0, P(bits), n_sets, stride, P(q_set), P(d_doc), P(d_score), P(d_chunk), P(d_n), eng._stream()),
    a.iters)
out["dense_path_within"] = eng.dense_path()
out["dense_within_256_ms"] = timed(lambda: eng.dense_topk(qv, k=100, within=ds), max(1, a.iters // 2))

r = Retriever(indexer=eng)
site = DocSet.from_mask(ix, rng.random(ix.n_docs) < 0.001)     # a site:-sized set (~1000 documents)
site.to(dev)
qh = qv[0].cpu().numpy()
r.search("q", terms=terms[0], query_embedding=qh, within=site)
torch.cuda.synchronize()
ts = []
for _ in range(a.iters):
    t = time.perf_counter()
    res = r.search("q", terms=terms[0], query_embedding=qh, within=site)
    ts.append((time.perf_counter() - t) * 1e3)
out["retriever_search_site_ms"] = float(np.median(ts))
out["retriever_search_site_results"] = len(res)
ts = []
for _ in range(a.iters):
    t = time.perf_counter()
    r.search("q", terms=terms[0], query_embedding=qh)
    ts.append((time.perf_counter() - t) * 1e3)
out["retriever_search_ms"] = float(np.median(ts))
eng.close()
print(json.dumps(out))

#!/usr/bin/env python3
"""Cost of facet counts over whole match sets (msr_facet_counts, DESIGN K17) at the bench shape: synthetic_corpus 1 M documents
/ 1 M terms (postings only), host ids from a skewed draw (a few hosts hold most pages, a tail of a few thousand), 256 rows per
call.  Per mix of counting terms
  (a) three rare terms,  (b) one mid-frequency term,  (c) one term in about half of the corpus
it reports the device time of msr_facet_counts alone (events, one warm-up, median of --iters), DeviceEngine.facet_counts with
its upload and its copy back (host clock), the bytes of the byte model (4 per posting of the listed terms, 2 per document of a
non-empty word of the match set, 2 T written and 2 T read per row; no base rows here) and the same answers from np.bincount
over host-built masks on the host clock -- asserted equal.  Beside them the BM25 stage of a 256-query chunk of the same run.
Prints one JSON line.
    python tools/facet_bench.py [--docs 1000000] [--rows 256] [--iters 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.engine import DeviceEngine  # noqa: E402
from msretr.facets import build_table  # noqa: E402
from msretr.synthetic import SEED, synthetic_corpus  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--rows", type=int, default=256)
ap.add_argument("--hosts", type=int, default=4000)
ap.add_argument("--limit", type=int, default=10)
ap.add_argument("--k", type=int, default=1000)
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda", 0)
PEAK_GBS = 6100.0                                            # streaming read the README measures (6.1 TB/s)


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


def host_timed(fn, iters):
    """Median host time (ms) of fn() -- a call that waits for its own result -- after one warm-up call."""
    fn()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


t0 = time.time()
ix = synthetic_corpus(a.docs, n_chunks=0, n_terms=a.terms, seed=SEED, device=dev)
R, N = a.rows, ix.n_docs
off = ix.term_off.cpu().numpy()
df = np.diff(off)
post = ix.post_doc.cpu().numpy()
log(f"corpus {N} docs, {int(off[-1])} postings in {time.time() - t0:.1f}s")
rng = np.random.default_rng(2)
w = 1.0 / (1.0 + np.arange(a.hosts)) ** 1.3                  # a few hosts hold most pages, a long tail
value = rng.choice(a.hosts, N, p=w / w.sum()).astype(np.int32)
value[rng.random(N) < 0.01] = -1                             # pages without a host
T = len(build_table(value, a.hosts)[2])
eng = DeviceEngine(ix, device=0, max_queries=R, max_k=a.k, rerank_max_docs=0)
t0 = time.time()
eng.bind_facet(value, a.hosts)
bind_s = time.time() - t0
n_spans = (N + 8191) // 8192
rare = rng.permutation(np.nonzero((df >= 10) & (df < 1000))[0])
mid = rng.permutation(np.nonzero((df >= 1000) & (df < 10000))[0])
half = np.argsort(np.abs(df - N // 2), kind="stable")[:8]    # the terms nearest to half of the corpus
assert len(rare) >= 3 * R and len(mid) >= R
mixes = {
    "a_rare_3": [[int(t) for t in rare[3 * q:3 * q + 3]] for q in range(R)],
    "b_mid_1": [[int(mid[q])] for q in range(R)],
    "c_half_1": [[int(half[q % len(half)])] for q in range(R)],
}
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
I32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=dev)
top_share = float(np.bincount(value[value >= 0]).max()) / N
out = {"docs": N, "postings": int(off[-1]), "rows": R, "device": torch.cuda.get_device_name(0), "n_values": a.hosts, "T": T,
       "top_host_share": top_share, "bind_facet_s": bind_s, "half_df": [int(df[t]) for t in half[:2]]}
packed = eng.pack_queries([[int(mid[q]), 0] for q in range(R)])
out["bm25_ms"] = timed(lambda: eng.bm25_topk(None, k=a.k, packed=packed), a.iters)
need = int(eng.lib.msr_facet_scratch_bytes(eng.handle, R))
scratch = torch.empty((need // 8 + 2,), dtype=torch.int64, device=dev)
out["scratch_bytes"] = need
for name, lists in mixes.items():
    a_off = I32(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).tolist())
    a_terms = I32([t for l in lists for t in l])
    res = torch.empty((2 * R + 2 * R * a.limit,), dtype=torch.int32, device=dev)
    hits, n_hit = res[:R], res[R:2 * R]
    tv, tc = res[2 * R:2 * R + R * a.limit], res[2 * R + R * a.limit:]

    def call():
        rc = eng.lib.msr_facet_counts(eng.handle, R, P(a_off), P(a_terms), P(None), 0, 0, P(None), a.limit, P(hits), P(n_hit),
                                      P(tv), P(tc), P(None), 0, P(scratch), need, eng._stream())
        assert rc == 0, rc
    ms = timed(call, a.iters)
    engine_ms = host_timed(lambda: eng.facet_counts(lists, limit=a.limit), a.iters)
    got = eng.facet_counts(lists, limit=a.limit, counts=True)
    # the host route: a mask per row from the posting lists, np.bincount over it
    t = time.perf_counter()
    words = 0
    want_hits, want_counts = np.zeros(R, np.int64), np.zeros((R, a.hosts), np.int64)
    for q, l in enumerate(lists):
        m = np.zeros(N, bool)
        for x in l:
            m[post[off[x]:off[x + 1]]] = True
        sel = value[m]
        want_hits[q] = m.sum()
        want_counts[q] = np.bincount(sel[sel >= 0], minlength=a.hosts)
        pad = np.zeros((N + 31) // 32 * 32, bool)
        pad[:N] = m
        words += int(pad.reshape(-1, 32).any(axis=1).sum())
    host_ms = (time.perf_counter() - t) * 1e3
    same = bool((got[0] == want_hits).all() and (got[4] == want_counts).all())
    order = np.lexsort((np.arange(a.hosts), -want_counts[0]))[:a.limit]
    same = same and got[2][0].tolist() == [int(v) if want_counts[0][v] else -1 for v in order]
    read = 4 * sum(int(df[x]) for l in lists for x in l) + 2 * 32 * words + 2 * T * R
    write = 2 * T * R + 4 * n_spans * R
    out[name] = {"facet_counts_ms": ms, "engine_facet_counts_ms": engine_ms, "read_bytes": read, "write_bytes": write,
                 "model_gbs": (read + write) / ms / 1e6, "of_peak": (read + write) / ms / 1e6 / PEAK_GBS,
                 "host_bincount_ms": host_ms, "equal_to_host": same, "mean_hits": float(want_hits.mean())}
    log(name, json.dumps(out[name]))
    assert same, name
eng.close()
print(json.dumps(out))

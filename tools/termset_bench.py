#!/usr/bin/env python3
"""Cost of document sets built from posting lists (msr_term_sets, DESIGN K11) at the bench shape: synthetic_corpus 1 M
documents / 1 M terms (postings only), 256 queries with their own operators each.  Per operator mix
  (a) one mid-frequency must term,  (b) must = the city term + one mid-frequency term,
  (c) one must_not of a long list,  (d) 8 must_not terms
it reports the device time of msr_term_sets alone (events, one warm-up, median of --iters), the bytes of the byte model
(4 per posting of every listed term, 4 ceil(N / 32) written per row; what the early exit skips is NOT subtracted, so the
GB/s of a mix with an early exit is an upper bound of the real traffic) and the host route it replaces on the host clock:
numpy masks from the posting lists -> docset.pack_within -> upload.  Then bm25_topk within those sets against the
unrestricted bm25_topk.  Prints one JSON line.
    python tools/termset_bench.py [--docs 1000000] [--queries 256] [--iters 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.docset import DocSet, pack_within  # noqa: E402
from msretr.engine import DeviceEngine  # noqa: E402
from msretr.synthetic import SEED, synthetic_corpus  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=256)
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


t0 = time.time()
ix = synthetic_corpus(a.docs, n_chunks=0, n_terms=a.terms, seed=SEED, device=dev)
Q, N = a.queries, ix.n_docs
W = (N + 31) // 32
off = ix.term_off.cpu().numpy()
df = np.diff(off)
log(f"corpus {N} docs, {int(off[-1])} postings in {time.time() - t0:.1f}s")
eng = DeviceEngine(ix, device=0, max_queries=Q, max_k=a.k, rerank_max_docs=0)
rng = np.random.default_rng(1)
mid = np.nonzero((df >= 1000) & (df < 10000))[0]
long_ = np.argsort(-df, kind="stable")[1:33]                 # the longest lists behind the city's (term 0)
assert len(mid) >= 9 * Q, len(mid)
pick = rng.permutation(mid)
mixes = {
    "a_must_mid": ([[int(pick[q])] for q in range(Q)], [[] for _ in range(Q)]),
    "b_must_city_mid": ([[0, int(pick[q])] for q in range(Q)], [[] for _ in range(Q)]),
    "c_not_long": ([[] for _ in range(Q)], [[int(long_[q % len(long_)])] for q in range(Q)]),
    "d_not_8": ([[] for _ in range(Q)], [[int(t) for t in pick[Q + 8 * q:Q + 8 * q + 8]] for q in range(Q)]),
}
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
I32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=dev)
out = {"docs": N, "postings": int(off[-1]), "queries": Q, "device": torch.cuda.get_device_name(0), "city_df": int(df[0])}


def host_lists(ts):
    """The posting lists of the named terms on the host (what a caller of the host route needs in memory anyway)."""
    return {t: ix.post_doc[off[t]:off[t + 1]].cpu().numpy() for t in ts}


def host_route(must, must_not, lists):
    """numpy masks -> DocSets -> pack_within -> upload: (seconds, device words [n_sets, W], q_set)."""
    t = time.perf_counter()
    sets = []
    for q in range(Q):
        m = np.ones(N, bool)
        for x in must[q]:
            h = np.zeros(N, bool)
            h[lists[x]] = True
            m &= h
        for x in must_not[q]:
            m[lists[x]] = False
        sets.append(DocSet(ix, m))
    words, q_set, n_sets, stride = pack_within(sets, Q, ix)
    bits = torch.from_numpy(words.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    return time.perf_counter() - t, bits, q_set


q_off, q_terms, q_qtf, _ = packed = eng.pack_queries([[int(pick[q]), 0] for q in range(Q)])
out["bm25_ms"] = timed(lambda: eng.bm25_topk(None, k=a.k, packed=packed), a.iters)
for name, (must, must_not) in mixes.items():
    # the library call alone: one row per query, lists in the order given
    m_off = I32(np.concatenate([[0], np.cumsum([len(x) for x in must])]).tolist())
    x_off = I32(np.concatenate([[0], np.cumsum([len(x) for x in must_not])]).tolist())
    m, x = I32([t for l in must for t in l]), I32([t for l in must_not for t in l])
    bits = torch.empty((Q, W), dtype=torch.int32, device=dev)

    def call():
        rc = eng.lib.msr_term_sets(eng.handle, Q, P(m_off), P(m), P(x_off), P(x), P(None), 0, 0, P(None), P(bits), W, eng._stream())
        assert rc == 0, rc
    ms = timed(call, a.iters)
    read = 4 * sum(int(df[t]) for l in must + must_not for t in l)
    write = 4 * W * Q
    lists = host_lists({t for l in must + must_not for t in l})
    host_s, host_bits, host_q = host_route(must, must_not, lists)
    same = bool(torch.equal(host_bits[torch.from_numpy(host_q.astype(np.int64)).to(dev)], bits))
    facade = timed(lambda: eng.term_sets(must, must_not), a.iters)            # host packing included, shortest list first
    ds = eng.term_sets(must, must_not)
    within_ms = timed(lambda: eng.bm25_topk(None, k=a.k, packed=packed, within=ds), a.iters)
    out[name] = {"term_sets_ms": ms, "read_bytes": read, "write_bytes": write, "model_gbs": (read + write) / ms / 1e6,
                 "of_peak": (read + write) / ms / 1e6 / PEAK_GBS, "host_route_ms": host_s * 1e3, "equal_to_host_route": same,
                 "engine_term_sets_ms": facade, "bm25_within_ms": within_ms}
    log(name, json.dumps(out[name]))
    assert same, name
eng.close()
print(json.dumps(out))

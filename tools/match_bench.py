#!/usr/bin/env python3
"""Cost of match modes (msr_match_sets, DESIGN K19) at the bench shape: synthetic_corpus 1 M documents / 1 M terms (postings
only), 256 rows with their own words each.  Per mix
  (a) all of 3 mid-frequency words,  (b) 2 of 3,  (c) all of the city term + one mid-frequency word,  (d) 2 of 8,
  (e) one 16-term expansion group + 2 words, all,  (f) at least 1 of 3
it reports, from ONE process: the device time of msr_match_sets alone (events, one warm-up, median of --iters, min and max
beside it; the groups shortest first, as match.match_sets orders them), the bytes of the byte model (4 per posting of every
listed term, 4 ceil(N / 32) written per row; what the early exit skips is NOT subtracted, so the GB/s of a mix with an early
exit is an upper bound of the real traffic), for the all-of mixes of single words msr_term_sets on the same must lists (the
answer without this kernel), the host route on the host clock (numpy counts from the posting lists -> docset.pack_within ->
upload; its rows are asserted equal to the kernel's, every row), match.match_sets with its host packing, and bm25_topk within
the rows against the unrestricted bm25_topk.  Prints one JSON line.
    python tools/match_bench.py [--docs 1000000] [--queries 256] [--iters 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr import match as mt  # noqa: E402
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
    """(median, min, max) device time (ms) of fn() over iters calls, after one warm-up call."""
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


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
assert len(mid) >= 3 * Q, len(mid)
pick = rng.permutation(mid)
term = lambda i: int(pick[i % len(pick)])
words = lambda q, n: [[term(n * q + j)] for j in range(n)]
mixes = {
    "a_all_of_3": ([words(q, 3) for q in range(Q)], 3),
    "b_2_of_3": ([words(q, 3) for q in range(Q)], 2),
    "c_all_city_mid": ([[[0], [term(q)]] for q in range(Q)], 2),
    "d_2_of_8": ([words(q, 8) for q in range(Q)], 2),
    "e_all_exp16_2": ([[[term(18 * q + j) for j in range(16)], [term(18 * q + 16)], [term(18 * q + 17)]] for q in range(Q)], 3),
    "f_1_of_3": ([words(q, 3) for q in range(Q)], 1),
}
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
I32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=dev)
out = {"docs": N, "postings": int(off[-1]), "queries": Q, "device": torch.cuda.get_device_name(0), "city_df": int(df[0]),
       "iters": a.iters}


def host_route(rows, need, lists):
    """numpy counts -> DocSets -> pack_within -> upload: (seconds, device words [n_sets, W], q_set)."""
    t = time.perf_counter()
    sets = []
    for groups in rows:
        count = np.zeros(N, np.int8)
        for g in groups:
            h = np.zeros(N, bool)
            for x in g:
                h[lists[x]] = True
            count += h
        sets.append(DocSet(ix, count >= need))
    words_, q_set, n_sets, stride = pack_within(sets, Q, ix)
    bits = torch.from_numpy(words_.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    return time.perf_counter() - t, bits, q_set


spread = lambda t: {"ms": t[0], "min_ms": t[1], "max_ms": t[2]}
packed = eng.pack_queries([[term(q), 0] for q in range(Q)])
out["bm25"] = spread(timed(lambda: eng.bm25_topk(None, k=a.k, packed=packed), a.iters))
for name, (rows, need) in mixes.items():
    rows = [sorted(g, key=lambda ts: (sum(int(df[t]) for t in ts), ts)) for g in rows]       # shortest first, as match_sets does
    g_off = I32(np.concatenate([[0], np.cumsum([len(g) for g in rows])]).tolist())
    t_off = I32(np.concatenate([[0], np.cumsum([len(ts) for g in rows for ts in g])]).tolist())
    terms = I32([t for g in rows for ts in g for t in ts])
    needs = I32([need] * Q)
    bits = torch.empty((Q, W), dtype=torch.int32, device=dev)

    def call():
        rc = eng.lib.msr_match_sets(eng.handle, Q, P(g_off), P(t_off), P(terms), P(needs), P(None), 0, 0, P(None), P(bits), W,
                                    eng._stream())
        assert rc == 0, rc
    t = timed(call, a.iters)
    read = 4 * sum(int(df[t_]) for g in rows for ts in g for t_ in ts)
    write = 4 * W * Q
    res = {"match_sets": spread(t), "read_bytes": read, "write_bytes": write, "model_gbs": (read + write) / t[0] / 1e6,
           "of_peak": (read + write) / t[0] / 1e6 / PEAK_GBS}
    lists = {t_: ix.post_doc[off[t_]:off[t_ + 1]].cpu().numpy() for g in rows for ts in g for t_ in ts}
    host_s, host_bits, host_q = host_route(rows, need, lists)
    same = bool(torch.equal(host_bits[torch.from_numpy(host_q.astype(np.int64)).to(dev)], bits))
    res.update(host_route_ms=host_s * 1e3, equal_to_host_route=same)
    if need == len(rows[0]) and all(len(ts) == 1 for g in rows for ts in g):      # all of single words: what msr_term_sets answers
        m_off, m = g_off, terms
        x_off = I32([0] * (Q + 1))
        ts_bits = torch.empty((Q, W), dtype=torch.int32, device=dev)

        def ts_call():
            rc = eng.lib.msr_term_sets(eng.handle, Q, P(m_off), P(m), P(x_off), P(None), P(None), 0, 0, P(None), P(ts_bits), W,
                                       eng._stream())
            assert rc == 0, rc
        res["term_sets"] = spread(timed(ts_call, a.iters))
        res["equal_to_term_sets"] = bool(torch.equal(ts_bits, bits))
        assert res["equal_to_term_sets"], name
    res["engine_match_sets"] = spread(timed(lambda: mt.match_sets(eng, rows, [need] * Q), a.iters))    # host packing included
    ds = mt.match_sets(eng, rows, [need] * Q)
    res["bm25_within"] = spread(timed(lambda: eng.bm25_topk(None, k=a.k, packed=packed, within=ds), a.iters))
    out[name] = res
    log(name, json.dumps(res))
    assert same, name
eng.close()
print(json.dumps(out))

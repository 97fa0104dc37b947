#!/usr/bin/env python3
"""Cost of the near-duplicate collapse (msr_doc_signatures, msr_collapse_duplicates, DESIGN K18) on the corpus, generator and
seeds of tools/phrase_bench.py (a token-stream corpus built on the GPU with keep_tokens=True), with --copies further documents
behind the generator's draws, each a copy of a random page (every second one with one token replaced), and ONE document of
100 000 tokens behind those:
  signatures the build for all documents but the long one, for all of them, and for the long one alone (shingle 4) -- device
             events, one warm-up, median of --iters with the fastest and the slowest beside it; the byte model (4 bytes per
             token read, 256 written per document); a sample of documents and the long one against numpy on the host
             (tests/dedup_ref.signatures_fast), asserted equal
  collapse   msr_collapse_duplicates alone for 256 queries x 1000 fused rows of which 0 %, 10 % and 50 % are copies of a
             page further up the list (min_matches 58), the first --check queries against numpy on the host
             (tests/dedup_ref.collapse_lists, host clock), asserted equal; and DeviceEngine.collapse_duplicates with its
             allocations and the copy of the drop arrays to the host, on the host clock
  chunk      the lexical 256-query chunk of the same run (Retriever.final_lists) without and with the collapse, host clock
Prints one JSON line.
    python tools/dedup_bench.py [--docs 1000000] [--copies 20000] [--queries 256] [--rows 1000] [--iters 10] [--no-chunk]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dedup_ref import collapse_lists, signatures_fast  # noqa: E402
from msretr.engine import DeviceEngine  # noqa: E402
from msretr.index_build import bm25_index_from_token_ids  # noqa: E402
from msretr.query import Conditions, SearchOptions  # noqa: E402
from msretr.retriever import Retriever  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--terms", type=int, default=200_000)
ap.add_argument("--mean-len", type=float, default=120.0)
ap.add_argument("--copies", type=int, default=20_000)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--long-tokens", type=int, default=100_000)
ap.add_argument("--sample", type=int, default=20_000)
ap.add_argument("--check", type=int, default=16)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--no-chunk", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
PEAK_GBS = 6100.0                                            # streaming read the README measures (6.1 TB/s)
SHINGLE, MIN_MATCHES = 4, 58


def log(*x):
    print(*x, file=sys.stderr, flush=True)


def timed(fn, iters):
    """(median, fastest, slowest) device time (ms) of fn() over iters calls, after one warm-up call."""
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


def host_timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


# ---- the corpus of tools/phrase_bench.py: the same generator, the same seeds, the same order of draws
t0 = time.time()
g = torch.Generator(device=dev).manual_seed(7)
N0, V, R = a.docs, a.terms, 256
lens = torch.exp(np.log(a.mean_len) - 0.32 + 0.8 * torch.randn(N0, generator=g, device=dev)).clamp_(8, 5000).to(torch.int64)
off0 = torch.zeros(N0 + 1, dtype=torch.int64, device=dev)
off0[1:] = torch.cumsum(lens, 0)
T0 = int(off0[-1])
w = 1.0 / torch.arange(1, V, device=dev, dtype=torch.float64) ** 1.07
cdf = (torch.cumsum(w, 0) / w.sum()).to(torch.float32)
tok0 = (torch.searchsorted(cdf, torch.rand(T0, generator=g, device=dev)).clamp_(max=V - 2) + 1).to(torch.int32)
start = off0[:-1]
city = torch.rand(N0, generator=g, device=dev) < 0.85
tok0[start[city]] = 0                                        # the city: first token of 85 % of the documents
rare = V + torch.arange(7 * R, device=dev, dtype=torch.int32).reshape(R, 7)
for r in range(R):
    d = torch.randint(0, N0, (40,), generator=g, device=dev)
    for j in range(2):
        tok0[start[d[:20]] + 2 + j] = rare[r, j]
    for j in range(5):
        tok0[start[d[20:]] + 2 + j] = rare[r, 2 + j]
n_terms = V + 7 * R
# behind the generator's draws: the copies (distinct sources; every second one with its last token replaced), then the long document
NC = min(a.copies, N0 // 2)
src = torch.randperm(N0, generator=g, device=dev)[:NC]
c_len = lens[src]
c_off = torch.zeros(NC + 1, dtype=torch.int64, device=dev)
c_off[1:] = torch.cumsum(c_len, 0)
pos = torch.arange(int(c_off[-1]), device=dev) - torch.repeat_interleave(c_off[:-1], c_len) + torch.repeat_interleave(start[src], c_len)
c_tok = tok0[pos].clone()
edited = c_off[1:][1::2] - 1
c_tok[edited] = (c_tok[edited] % (V - 2)) + 1
long_tok = (torch.searchsorted(cdf, torch.rand(a.long_tokens, generator=g, device=dev)).clamp_(max=V - 2) + 1).to(torch.int32)
N = N0 + NC + 1
off = torch.cat([off0, off0[-1] + c_off[1:], (off0[-1] + c_off[-1] + a.long_tokens).reshape(1)])
tok = torch.cat([tok0, c_tok, long_tok])
T = int(off[-1])
ix = bm25_index_from_token_ids(np.arange(N, dtype=np.int64), off, tok, n_terms, device=dev, keep_tokens=True)
log(f"corpus {N} docs ({NC} copies), {T} tokens, {int(ix.post_doc.numel())} postings in {time.time() - t0:.1f}s")
Q, M = a.queries, a.rows
h_off, h_tok, h_src = off.cpu().numpy(), tok.cpu().numpy(), src.cpu().numpy()
rng = np.random.default_rng(1)
out = {"docs": N, "copies": NC, "tokens": T, "queries": Q, "rows": M, "shingle": SHINGLE, "min_matches": MIN_MATCHES,
       "iters": a.iters, "device": torch.cuda.get_device_name(0)}
P = lambda t: C.c_void_p(t.data_ptr())

eng = DeviceEngine(ix, device=0, max_queries=max(Q, 16), max_k=16, rerank_max_docs=0)
assert eng.has_tokens

# ---- signatures
sig = torch.empty((N, 64), dtype=torch.int32, device=dev)


def build(d0, d1):
    rc = eng.lib.msr_doc_signatures(eng.handle, d0, d1, SHINGLE, P(sig[d0:]), eng._stream())
    assert rc == 0, rc


res = {"without_long_document_ms": timed(lambda: build(0, N - 1), a.iters),
       "with_long_document_ms": timed(lambda: build(0, N), a.iters),
       "long_document_alone_ms": timed(lambda: build(N - 1, N), a.iters)}
res.update(read_bytes=4 * T, written_bytes=256 * N, of_peak=(4 * T + 256 * N) / res["with_long_document_ms"][0] / 1e6 / PEAK_GBS)
build(0, N)
h_sig = sig.cpu().numpy().view(np.uint32)
pick = np.unique(np.concatenate([rng.integers(0, N0, a.sample), N0 + rng.integers(0, NC, a.sample // 10), [N - 1]]))
t = time.perf_counter()
same = all((signatures_fast(h_off, h_tok, SHINGLE, int(d), int(d) + 1)[0] == h_sig[d]).all() for d in pick)
res.update(host_numpy_ms_per_document=(time.perf_counter() - t) * 1e3 / len(pick), checked_documents=int(len(pick)),
           equal_to_host=bool(same))
assert same
m_copy = (h_sig[N0:N0 + NC] == h_sig[h_src]).sum(axis=1)
res.update(copies_at_or_above_min_matches=int((m_copy >= MIN_MATCHES).sum()), copy_matches_min=int(m_copy.min()))
out["signatures"] = res
log("signatures", json.dumps(res))
eng.bind_signatures(sig)

# ---- the collapse alone: lists of M rows of which a share are copies of a page that is in the list too
good = np.nonzero(m_copy >= MIN_MATCHES)[0]                  # copies the collapse will find
is_src = np.zeros(N0, bool)
is_src[h_src] = True
plain_docs = np.nonzero(~is_src)[0]
need = int(eng.lib.msr_collapse_scratch_bytes(Q, M))
scratch = torch.empty((need // 8 + 2,), dtype=torch.int64, device=dev)
i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
outs = [i32(Q, M), f64(Q, M), f64(Q, M), i32(Q, M), i32(Q), i32(Q, M), i32(Q, M), i32(Q, M), i32(Q)]
out["collapse"] = {"scratch_bytes": need}
for share in (0.0, 0.1, 0.5):
    n_dup = int(round(share * M))
    doc = np.empty((Q, M), np.int32)
    for q in range(Q):
        c = rng.choice(good, n_dup, replace=False)
        row = np.concatenate([N0 + c, h_src[c], rng.choice(plain_docs, M - 2 * n_dup, replace=False)])
        doc[q] = rng.permutation(row)
    score = -np.sort(-rng.random((Q, M)), axis=1)
    orig, chunk, n = rng.random((Q, M)), doc.copy(), np.full(Q, M, np.int32)
    ins = [torch.from_numpy(x).to(dev) for x in (doc, score, orig, chunk, n)]

    def kernel():
        rc = eng.lib.msr_collapse_duplicates(eng.handle, Q, *map(P, ins), M, MIN_MATCHES, *map(P, outs), P(scratch), need,
                                             eng._stream())
        assert rc == 0, rc

    res = {"kernels_ms": timed(kernel, a.iters)}

    def engine_call():
        kept, drops = eng.collapse_duplicates(tuple(ins), MIN_MATCHES)
        return [x.cpu() for x in drops]

    res["engine_call_with_copies_ms"] = host_timed(engine_call, a.iters)
    kernel()
    got = [o.cpu().numpy() for o in outs]
    res["dropped_per_query"] = float(got[8].mean())
    k = min(a.check, Q)
    t = time.perf_counter()
    want = collapse_lists(doc[:k], score[:k], orig[:k], chunk[:k], n[:k], h_sig, MIN_MATCHES)
    res["host_numpy_ms_per_query"] = (time.perf_counter() - t) * 1e3 / k
    same = all(np.array_equal(x[:k], y) for x, y in zip(got, want))
    res.update(checked_queries=k, equal_to_host=bool(same))
    assert same, share
    assert abs(res["dropped_per_query"] - n_dup) <= 1, (share, res["dropped_per_query"])
    out["collapse"][f"{int(share * 100)}_percent"] = res
    log(f"collapse {share}", json.dumps(res))
eng.close()

if not a.no_chunk:
    # ---- the lexical 256-query chunk of the same run, without and with the collapse: one chunk vector per document
    def word(t):
        if t == 0:
            return "tübingen"
        s, t = "", int(t)
        while True:
            s = chr(ord("a") + t % 26) + s
            t //= 26
            if t == 0:
                return "w" + s

    t0 = time.time()
    ix.doc_off = torch.arange(N + 1, dtype=torch.int32)
    ix.chunk_ids = torch.arange(N, dtype=torch.int64)
    emb = torch.randn((N, 768), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    ix.emb = emb / emb.norm(dim=1, keepdim=True)
    del emb
    r = Retriever(indexer=DeviceEngine(ix, device=0, max_queries=Q, max_k=1000, rerank_max_docs=1000))
    log(f"retriever in {time.time() - t0:.1f}s")
    df = np.diff(ix.term_off.cpu().numpy())
    mid = np.nonzero((df >= 1000) & (df < 10000))[0]
    mid = mid[(mid < V) & (mid > 0)]
    ids = [[int(t) for t in rng.choice(mid, 3, replace=False)] for _ in range(Q)]
    qv = torch.randn((Q, 768), generator=torch.Generator().manual_seed(4)).numpy()
    on = SearchOptions(collapse_duplicates=True)
    t0 = time.perf_counter()
    r._ensure_signatures()
    torch.cuda.synchronize()
    res = {"first_use_build_and_bind_ms": (time.perf_counter() - t0) * 1e3}
    dd = {}
    res["chunk_ms"] = host_timed(lambda: r.final_lists(ids, qv, 1000), a.iters)
    res["chunk_with_collapse_ms"] = host_timed(
        lambda: r._final(ids, qv, 1000, None, None, on, Conditions(), None, None, None, dedup=dd), a.iters)
    res["dropped_per_query"] = float(np.mean([len(d) for d in dd["drops"]]))
    fused, _ = r._fused_chunk(ids, r.engine._dev(qv, torch.float32), 1000)
    res["fused_rows_per_query"] = float(fused[4].float().mean())
    res["collapse_kernels_on_the_chunk_ms"] = timed(lambda: r.engine.collapse_duplicates(fused, MIN_MATCHES), a.iters)
    out["chunk"] = res
    log("chunk", json.dumps(res))
    r.engine.close()
print(json.dumps(out))
